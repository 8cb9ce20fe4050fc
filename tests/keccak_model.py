"""Pure-Python Keccak-f[1600] and the 256-bit sponge over it (rate 136 bytes), with the domain byte as a parameter: 0x01 is
Keccak-256 as submitted, 0x06 is FIPS 202 SHA3-256.  The model the device kernels (csrc/keccak.h) are compared with; it is
itself pinned against hashlib.sha3_256 and published Keccak-256 vectors in tests/test_keccak_model_cpu.py.  Nothing here is
typed in: the round constants come from the LFSR of FIPS 202 (3.2.5), the rotations from the walk of 3.2.2."""

M64 = (1 << 64) - 1
RATE = 136
DOMAIN_KECCAK, DOMAIN_SHA3 = 0x01, 0x06


def _round_constants():
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            if r & 1:
                rc |= 1 << ((1 << j) - 1)
            r = ((r << 1) ^ (0x71 if r & 0x80 else 0)) & 0xff      # x^8 + x^6 + x^5 + x^4 + 1
        out.append(rc)
    return out


def _rotations():
    rot, (x, y) = [0] * 25, (1, 0)
    for t in range(24):
        rot[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return rot


RC, ROT = _round_constants(), _rotations()


def rotl(v, n):
    return ((v << n) | (v >> (64 - n))) & M64 if n else v


def keccak_f1600(a):
    """a: 25 lanes, a[x + 5 y]; returns the permuted state"""
    a = list(a)
    for rc in RC:
        c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
        d = [c[(x + 4) % 5] ^ rotl(c[(x + 1) % 5], 1) for x in range(5)]
        a = [a[i] ^ d[i % 5] for i in range(25)]
        b = [0] * 25
        for x in range(5):
            for y in range(5):
                b[y + 5 * ((2 * x + 3 * y) % 5)] = rotl(a[x + 5 * y], ROT[x + 5 * y])
        a = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & M64 & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
        a[0] ^= rc
    return a


def sponge256(msg: bytes, domain: int) -> bytes:
    pad = bytearray(RATE - len(msg) % RATE)
    pad[0] ^= domain
    pad[-1] ^= 0x80
    data, a = bytes(msg) + bytes(pad), [0] * 25
    for off in range(0, len(data), RATE):
        for i in range(RATE // 8):
            a[i] ^= int.from_bytes(data[off + 8 * i:off + 8 * i + 8], "little")
        a = keccak_f1600(a)
    return b"".join(v.to_bytes(8, "little") for v in a[:4])


def keccak256(msg: bytes) -> bytes:
    return sponge256(msg, DOMAIN_KECCAK)


def sha3_256(msg: bytes) -> bytes:
    return sponge256(msg, DOMAIN_SHA3)


def address(xy64: bytes) -> bytes:
    """the 20-byte address of a public key X || Y"""
    assert len(xy64) == 64
    return keccak256(xy64)[12:]
