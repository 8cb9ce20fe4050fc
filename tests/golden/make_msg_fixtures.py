#!/usr/bin/env python3
"""The MESSAGES of the reference's two Wycheproof ECDSA files, as the small JSON fixture committed next to this script:
wycheproof_ecdsa_msgs.json = {"sha256": {tcId: msg hex}, "sha512": {tcId: msg hex}}.  make_fixtures.py stores each case's
digest (the reference's harness hashes first, secec/wycheproof_test.go:317-334); the calls that hash on the device start
from the message, so the tests of those need it.  Keys, signatures and expected results stay in the existing fixtures and
are joined by tcId.

Run in the authoring container only (it reads the reference checkout, which does not exist on the GPU box):
    python tests/golden/make_msg_fixtures.py

Sources (relative to the reference checkout):
  secec/testdata/wycheproof/ecdsa_secp256k1_sha256_test.json
  secec/testdata/wycheproof/ecdsa_secp256k1_sha512_test.json
Only data is emitted.  No reference source text is stored.
"""
import json
import os

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def messages(fn):
    d = json.load(open(os.path.join(REF, "secec/testdata/wycheproof", fn)))
    out = {}
    for g in d["testGroups"]:
        for t in g["tests"]:
            out[str(t["tcId"])] = t["msg"]
    assert len(out) == d["numberOfTests"]
    return out


def main():
    obj = {"source": "secec/testdata/wycheproof/ecdsa_secp256k1_sha{256,512}_test.json",
           "sha256": messages("ecdsa_secp256k1_sha256_test.json"), "sha512": messages("ecdsa_secp256k1_sha512_test.json")}
    p = os.path.join(OUT, "wycheproof_ecdsa_msgs.json")
    with open(p, "w") as f:
        json.dump(obj, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"wycheproof_ecdsa_msgs.json: {os.path.getsize(p)} bytes")


if __name__ == "__main__":
    main()
