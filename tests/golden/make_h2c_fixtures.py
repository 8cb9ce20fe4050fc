#!/usr/bin/env python3
"""Convert the reference's hash-to-curve test DATA (the RFC 9380 vectors it ships) into tests/golden/h2c.json.

Run in the authoring container only (it reads the reference tree, as make_fixtures.py does):
    python tests/golden/make_h2c_fixtures.py

Sources (relative to the reference): secec/h2c/testdata/
  secp256k1_XMD_SHA-256_SSWU_RO_.json, secp256k1_XMD_SHA-256_SSWU_NU_.json   (RFC 9380 J.8.1 / J.8.2; h2c_test.go)
  expand_message_xmd_SHA256_38.json, expand_message_xmd_SHA256_256.json       (RFC 9380 K.1 / K.2)
Only the fields a test reads are kept: tag, message, field elements, points, output length and bytes, DST_prime.
Strings are stored as hex of their bytes, integers as 64 hex digits.
"""
import json
import os

from make_fixtures import REF

OUT = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(REF, "secec/h2c/testdata")


def h64(s):
    return "%064x" % int(s, 16)


def pt(d):
    return [h64(d["x"]), h64(d["y"])]


def suite(fn, ro):
    d = json.load(open(os.path.join(SRC, fn)))
    assert d["randomOracle"] is ro and d["curve"] == "secp256k1" and d["hash"] == "sha256" and int(d["L"], 16) == 48
    vecs = []
    for v in d["vectors"]:
        e = {"msg": v["msg"].encode().hex(), "u": [h64(x) for x in v["u"]], "P": pt(v["P"])}
        if ro:
            e["Q0"], e["Q1"] = pt(v["Q0"]), pt(v["Q1"])
        else:
            e["Q"] = pt(v["Q"])
        vecs.append(e)
    return {"dst": d["dst"].encode().hex(), "suite": d["ciphersuite"], "vectors": vecs}


def expand(fn):
    d = json.load(open(os.path.join(SRC, fn)))
    assert d["hash"] == "SHA256" and d["name"] == "expand_message_xmd"
    tests = [{"msg": t["msg"].encode().hex(), "len_in_bytes": int(t["len_in_bytes"], 16), "uniform_bytes": t["uniform_bytes"],
              "DST_prime": t["DST_prime"]} for t in d["tests"]]
    return {"dst": d["DST"].encode().hex(), "tests": tests}


def main():
    obj = {
        "ro": suite("secp256k1_XMD_SHA-256_SSWU_RO_.json", True),
        "nu": suite("secp256k1_XMD_SHA-256_SSWU_NU_.json", False),
        "expand_short_dst": expand("expand_message_xmd_SHA256_38.json"),
        "expand_long_dst": expand("expand_message_xmd_SHA256_256.json"),
    }
    p = os.path.join(OUT, "h2c.json")
    with open(p, "w") as f:
        json.dump(obj, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print(f"h2c.json: {os.path.getsize(p)} bytes")


if __name__ == "__main__":
    main()
