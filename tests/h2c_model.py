"""Big-integer model of RFC 9380 for secp256k1: expand_message_xmd with SHA-256 (section 5.3.1, oversize tags 5.3.3),
hash_to_field, the simplified SWU map on the isogenous curve E' (section 6.6.2, affine, with its inversions), the 3-isogeny
(appendix E.1) and the two suites secp256k1_XMD:SHA-256_SSWU_RO_ / _NU_ (section 8.7).  Written from the RFC's text with
hashlib and Python integers; curve additions come from pyref.py.  It is the referee of the device kernels in csrc/h2c.hip,
which compute the same map in another shape (fractions, one exponentiation per mapped point, one inversion per record).
"""
import hashlib

import pyref
from pyref import P

L = 48                      # ceil((ceil(log2(p)) + k) / 8), k = 128
Z = P - 11
A_ISO = 0x3F8731ABDD661ADCA08A5558F0F5D272E953D363CB6F0E5D405447C01A444533
B_ISO = 1771
K1 = (0x8E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38DAAAAA8C7,
      0x07D3D4C80BC321D5B9F315CEA7FD44C5D595D2FC0BF63B92DFFF1044F17C6581,
      0x534C328D23F234E6E2A413DECA25CAECE4506144037C40314ECBD0B53D9DD262,
      0x8E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38E38DAAAAA88C)
K2 = (0xD35771193D94918A9CA34CCBB7B640DD86CD409542F8487D9FE6B745781EB49B,
      0xEDADC6F64383DC1DF7C4B2D51B54225406D36B641F5E41BBC52A56612A8C6D14)
K3 = (0x4BDA12F684BDA12F684BDA12F684BDA12F684BDA12F684BDA12F684B8E38E23C,
      0xC75E0C32D5CB7C0FA9D0A54B12A0A6D5647AB046D686DA6FDFFC90FC201D71A3,
      0x29A6194691F91A73715209EF6512E576722830A201BE2018A765E85A9ECEE931,
      0x2F684BDA12F684BDA12F684BDA12F684BDA12F684BDA12F684BDA12F38E38D84)
K4 = (0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFF93B,
      0x7A06534BB8BDB49FD5E9E6632722C2989467C1BFC8E8D978DFB425D2685C2573,
      0x6484AA716545CA2CF3A70C3FA8FE337E0A3D21162F0D6299A7BF8192BFD2A76F)


def dst_prime(dst: bytes) -> bytes:
    """DST || I2OSP(len(DST), 1); a tag of more than 255 bytes is hashed first (5.3.3).  An empty tag is refused (3.1)."""
    if len(dst) == 0:
        raise ValueError("empty domain separation tag")
    if len(dst) > 255:
        dst = hashlib.sha256(b"H2C-OVERSIZE-DST-" + dst).digest()
    return dst + bytes([len(dst)])


def expand_message_xmd(msg: bytes, dst: bytes, len_in_bytes: int) -> bytes:
    ell = (len_in_bytes + 31) // 32
    if len_in_bytes < 1 or ell > 255:
        raise ValueError("len_in_bytes out of range")
    dp = dst_prime(dst)
    b0 = hashlib.sha256(bytes(64) + msg + len_in_bytes.to_bytes(2, "big") + b"\0" + dp).digest()
    b = [hashlib.sha256(b0 + b"\x01" + dp).digest()]
    for i in range(2, ell + 1):
        b.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, b[-1])) + bytes([i]) + dp).digest())
    return b"".join(b)[:len_in_bytes]


def hash_to_field(msg: bytes, dst: bytes, count: int):
    ub = expand_message_xmd(msg, dst, count * L)
    return [int.from_bytes(ub[i * L:(i + 1) * L], "big") % P for i in range(count)]


def _inv0(x):
    """inv0 of the RFC: 1 / x, and 0 for 0"""
    x %= P
    return pow(x, -1, P) if x else 0


def map_to_curve_simple_swu(u: int):
    """6.6.2, on E': y^2 = x^3 + A' x + B'."""
    tv1 = _inv0((Z * Z * pow(u, 4, P) + Z * u * u) % P)
    x1 = (-B_ISO * _inv0(A_ISO)) % P * (1 + tv1) % P
    if tv1 == 0:
        x1 = B_ISO * _inv0(Z * A_ISO % P) % P
    gx1 = (pow(x1, 3, P) + A_ISO * x1 + B_ISO) % P
    x2 = Z * u * u % P * x1 % P
    gx2 = (pow(x2, 3, P) + A_ISO * x2 + B_ISO) % P
    x, y = x1, pyref.sqrt_p(gx1)            # (None: gx1 is not a square, then gx2 is)
    if y is None:
        x, y = x2, pyref.sqrt_p(gx2)
    assert y is not None
    if (u & 1) != (y & 1):
        y = P - y
    return x, y


def iso_map(x: int, y: int):
    """E.1; a vanishing denominator gives the identity (None)."""
    xn = (K1[3] * pow(x, 3, P) + K1[2] * x * x + K1[1] * x + K1[0]) % P
    xd = (x * x + K2[1] * x + K2[0]) % P
    yn = (K3[3] * pow(x, 3, P) + K3[2] * x * x + K3[1] * x + K3[0]) % P
    yd = (pow(x, 3, P) + K4[2] * x * x + K4[1] * x + K4[0]) % P
    if xd == 0 or yd == 0:
        return None
    return (xn * _inv0(xd) % P, y * yn % P * _inv0(yd) % P)


def map_to_curve(u: int):
    return iso_map(*map_to_curve_simple_swu(u % P))


def set_uniform_bytes(src: bytes):
    """map_to_curve(OS2IP(src) mod p) for 32..64 bytes."""
    if not 32 <= len(src) <= 64:
        raise ValueError("32..64 bytes")
    return map_to_curve(int.from_bytes(src, "big") % P)


def map_to_curve_sum(uniform: bytes, length: int, count: int):
    """what s2k_map_to_curve_batch computes for one item: the sum of `count` mapped points"""
    acc = None
    for j in range(count):
        acc = pyref.add(acc, set_uniform_bytes(uniform[j * length:(j + 1) * length]))
    return acc


def hash_to_curve(msg: bytes, dst: bytes):
    u = hash_to_field(msg, dst, 2)
    q0, q1 = map_to_curve(u[0]), map_to_curve(u[1])
    return pyref.add(q0, q1), u, (q0, q1)


def encode_to_curve(msg: bytes, dst: bytes):
    u = hash_to_field(msg, dst, 1)
    q = map_to_curve(u[0])
    return q, u, (q,)
