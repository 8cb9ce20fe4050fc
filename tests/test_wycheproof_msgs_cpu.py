"""The message fixture of the calls that hash on the device (tests/golden/wycheproof_ecdsa_msgs.json: tcId -> msg for the
reference's two Wycheproof ECDSA files) against the digest fixtures the other tests use: for every case the hash of the
message is the stored digest.  Data only; no device."""
import hashlib

import pytest

from conftest import load_golden


@pytest.mark.parametrize("name,hashfn,cases", [("sha256", hashlib.sha256, 463), ("sha512", hashlib.sha512, 533)])
def test_messages_hash_to_the_stored_digests(name, hashfn, cases):
    msgs = load_golden("wycheproof_ecdsa_msgs.json")[name]
    d = load_golden(f"wycheproof_ecdsa_{name}.json")["cases"]
    assert len(d) == cases and sorted(msgs, key=int) == [str(c["tcId"]) for c in sorted(d, key=lambda c: c["tcId"])]
    for c in d:
        assert hashfn(bytes.fromhex(msgs[str(c["tcId"])])).hexdigest() == c["digest"], c["tcId"]
