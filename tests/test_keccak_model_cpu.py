"""Pins tests/keccak_model.py, the model the device's Keccak kernels are compared with: with the domain byte 0x06 it is
hashlib.sha3_256 at every length that matters to a 136-byte sponge, and with 0x01 it gives the published Keccak-256
vectors (the empty string, "abc") and the address of the key of secret 1.  No device, no library."""
import hashlib

import keccak_model as K
import pyref as R


def _msg(n):
    return bytes((131 * i + 7 * n + 1) & 0xff for i in range(n))


def test_model_is_sha3_256_with_domain_06():
    for n in list(range(301)) + [407, 408, 409, 1000]:
        m = _msg(n)
        assert K.sponge256(m, 0x06) == hashlib.sha3_256(m).digest(), n
    assert K.sha3_256(b"abc") == hashlib.sha3_256(b"abc").digest()


def test_model_keccak256_vectors():
    assert K.sponge256(b"", 0x01).hex() == "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470"
    assert K.keccak256(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    g = R.b32(R.GX) + R.b32(R.GY)
    assert K.keccak256(g)[12:].hex() == K.address(g).hex() == "7e5f4552091a69125d5dfcb7b8c2659029395bdf"


def test_model_constants_are_generated():
    """the first and last round constants and two rotations, as FIPS 202 tabulates them"""
    assert K.RC[0] == 1 and K.RC[1] == 0x8082 and K.RC[23] == 0x8000000080008008 and len(set(K.RC)) == 22
    assert K.ROT[0] == 0 and K.ROT[1] == 1 and K.ROT[5] == 36 and K.ROT[24] == 14
