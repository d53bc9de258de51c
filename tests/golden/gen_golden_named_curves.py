#!/usr/bin/env python3
"""Write tests/golden/ec_named.json: k G for eight scalars on each of the 19 distinct named curves of the reference
(demo/mixnet/.conf:151-176), computed by libcrypto (EC_POINT_mul) -- the curve constants too, so that the file pins them
independently of the product's tables.  Deterministic: the scalars come from a seeded generator.

    python3 tests/golden/gen_golden_named_curves.py
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from named_curves import library_table, openssl_curve, openssl_mul  # noqa: E402


def main():
    table, _ = library_table()
    out = {}
    for name in sorted(table):
        c = openssl_curve(name)
        assert c["h"] == 1
        rnd = random.Random("ec_named/" + name)
        ks = [1, 2, c["n"] - 1, c["n"] - 2] + [rnd.randrange(1, c["n"]) for _ in range(4)]
        hx = lambda v: "%x" % v
        out[name] = dict(p=hx(c["p"]), a=hx(c["a"]), b=hx(c["b"]), n=hx(c["n"]), g=[hx(c["gx"]), hx(c["gy"])],
                         cases=[dict(k=hx(k), kG=[hx(v) for v in openssl_mul(name, k)]) for k in ks])
    with open(os.path.join(HERE, "ec_named.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
