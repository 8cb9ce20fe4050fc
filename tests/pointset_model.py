"""Big-integer model of what k_ps_front (secp256k1_voi_amd/csrc/pointset.hip) does to a scalar: the endomorphism split
(the reference's splitGLV, point_mul_glv.go:59-117, as tests/test_glv_odd_model.py models it) and the carry-free signed
recoding of each 128-bit magnitude into 128 / c + 1 digits of c bits (c = 4 or 8):

    k + C,  C = the constant with bit c - 1 of every digit below 2^128 set,

has the c-bit digits d_p + 2^(c-1) with -2^(c-1) <= d_p < 2^(c-1), and its bit 128 is the last digit (the carry, 0 or 1):
k = sum_p d_p 2^(c p).  The device stores one 16-bit word per digit: |d| in bits 0-8 (it can be 2^(c-1) = 128 at c = 8), bit 15
set when the table entry is to be negated (digit sign times half-scalar sign), 0 for a zero digit."""
N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
LAM = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
A1 = 0x3086D221A7D46BCDE86C90E49284EB15
B1 = -0xE4437ED6010E88286F547FA90ABFE4C3
B2 = A1
G1 = 0x3086D221A7D46BCDE86C90E49284EB153DAA8A1471E8CA7FE893209A45DBB031
G2 = 0xE4437ED6010E88286F547FA90ABFE4C4221208AC9DF506C61571B4AE8AC47F71
NEG, MAG = 0x8000, 0x1FF


def positions(c):
    return 128 // c + 1


def add_constant(c):
    return sum(1 << (c * p + c - 1) for p in range(128 // c))


def recode(k, c):
    """The signed digits of a magnitude k < 2^128, lowest position first; the last one is the carry."""
    assert 0 <= k < 1 << 128 and c in (4, 8)
    v = k + add_constant(c)
    return [((v >> (c * p)) & ((1 << c) - 1)) - (1 << (c - 1)) for p in range(128 // c)] + [v >> 128]


def digit_word(d, neg):
    return 0 if d == 0 else abs(d) | (NEG if (d < 0) != neg else 0)


def split(k):
    """splitGLV of a reduced scalar: (|k1|, k1 < 0, |k2|, k2 < 0) with k = k1 + k2 lambda mod n."""
    c1 = (k * G1 + (1 << 383)) >> 384
    c2 = (k * G2 + (1 << 383)) >> 384
    k2 = (-c1 * B1 - c2 * B2) % N
    k1 = (k - k2 * LAM) % N
    k1 = k1 - N if k1 > N // 2 else k1
    k2 = k2 - N if k2 > N // 2 else k2
    return abs(k1), k1 < 0, abs(k2), k2 < 0


def reaches_carry(k, c):
    """Does a half scalar of k (any 256-bit value, reduced as SetBytes first) have a non-zero digit at the last position?"""
    m1, _, m2, _ = split(k % N)
    return recode(m1, c)[-1] == 1 or recode(m2, c)[-1] == 1


def boundary_pool():
    pool = [0, 1, 1 << 127, (1 << 128) - 1, int.from_bytes(b"\x80" * 16, "big"), int.from_bytes(b"\x7f" * 16, "big"),
            int.from_bytes(b"\xff" * 16, "big")]
    for c in (4, 8):
        t = (1 << 128) - add_constant(c)          # the smallest magnitude whose recoding carries
        pool += [t - 1, t, t + 1]
    return pool
