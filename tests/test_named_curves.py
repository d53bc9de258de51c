"""CPU suite: the named curves of the reference (demo/mixnet/.conf:151-176) -- the 26 names ECqPGroup accepts, 19 distinct
curves.  Their constants in the library's table (csrc/vmnhip.hip kCurves) and in the host scalars (ecscalar.py) are
libcrypto's, every one has cofactor 1, the limb count of every curve leaves the headroom the lazy bounds of the point
formulas need and has kernels instantiated for its kind, and the host-side arithmetic over a general a (ecscalar.py,
csrc/hostcurve.h) agrees with libcrypto's EC_POINT_mul."""
import os
import random
import re
import subprocess

import pytest

from named_curves import NAMES, ROOT, ecscalar, library_table, openssl_curve, openssl_mul

EC_NIST, EC_GENERAL = 0, 1


def entry_of(name):
    table, aliases = library_table()
    return table[aliases.get(name, name)]


def test_the_reference_names_26_curves_19_distinct():
    table, aliases = library_table()
    assert len(NAMES) == 26 and len(table) == 19
    assert set(NAMES) <= set(table) | set(aliases)
    assert all(v in table for v in aliases.values())
    assert len({(c["p"], c["a"] if c["a"] is not None else c["p"] - 3, c["b"]) for c in table.values()}) == 19
    es = ecscalar()
    assert set(es.CURVES) == set(table) and set(es.ALIASES) == set(aliases)
    assert all(es.ALIASES[k] == v for k, v in aliases.items())


@pytest.mark.parametrize("name", NAMES)
def test_constants_are_libcryptos(name):
    """p, a, b, G, n of the library's table and of ecscalar.py equal libcrypto's, and the cofactor is 1 (the group of points
    is the group of order n that the proofs work in)."""
    want = openssl_curve(name)
    assert want["h"] == 1
    c = entry_of(name)
    a = c["a"] if c["a"] is not None else c["p"] - 3
    assert (c["p"], a, c["b"], c["gx"], c["gy"], c["n"]) == tuple(want[k] for k in ("p", "a", "b", "gx", "gy", "n"))
    assert c["bits"] == want["p"].bit_length() and c["NW"] * 32 >= c["bits"]
    # Hasse: n = p + 1 - t with |t| <= 2 sqrt(p), so with cofactor 1 the order has the width of p or one bit more (secp224k1)
    assert abs(want["p"] + 1 - want["n"]) ** 2 <= 4 * want["p"]
    es = ecscalar()
    e = es.curve(name)
    assert (e["p"], es.curve_a(e), e["b"], e["gx"], e["gy"], e["n"]) == (c["p"], a, c["b"], c["gx"], c["gy"], c["n"])


def test_secp224k1_is_the_curve_with_the_wide_order_and_p_1_mod_4():
    """The two properties the kernels must meet for one curve only: an order one bit wider than p (exponents are sized by
    bits(n)) and p = 1 mod 4 (square roots by Tonelli-Shanks) -- besides P-224, which also has p = 1 mod 4."""
    table, _ = library_table()
    wide = [k for k, c in table.items() if c["n"].bit_length() > c["p"].bit_length()]
    one_mod_4 = [k for k, c in table.items() if c["p"] % 4 == 1]
    assert wide == ["secp224k1"] and sorted(one_mod_4) == ["P-224", "secp224k1"]


def stride_for_limbs(s):
    return (s + 3) // 4 * 4


@pytest.mark.parametrize("name", sorted(library_table()[0]))
def test_limb_counts_and_instances(name):
    """R / p >= 2^24 (the Montgomery limit of the lazy operands of the point formulas), a padding word behind the limbs for
    the infinity flag (ECfg: FW > S), the column bound of a carry-less sum at this limb count, and a (limbs, words, kind)
    that VMN_FOR_CURVES dispatches and ec_instances.h instantiates in a unit the build compiles."""
    c = entry_of(name)
    S, NW = c["S"], c["NW"]
    assert 28 * S - c["p"].bit_length() >= 24 and (1 << (28 * S)) >= (c["p"] << 24)
    assert stride_for_limbs(S) > S
    lazy, norm = (1 << 29) - 1, (1 << 28) - 1
    assert S * lazy * lazy + S * norm * norm + (1 << 40) < 1 << 64
    assert S * lazy * norm + (1 << 60) + S * norm * norm + (1 << 40) < 1 << 64
    # the kind: an entry that names a runs on the general kernels; one without (a = -3) on the NIST kernels, which have the
    # primes of 10 and 15 limbs compiled in (P-256, P-384) and take any prime at run time at 9 and 21 limbs
    kind = EC_GENERAL if c["a"] is not None else EC_NIST
    if kind == EC_NIST:
        assert S in (9, 21) or name in ("P-256", "P-384")
    src = open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "vmnhip.hip")).read()
    fc = src[src.index("#define VMN_FOR_CURVES(X)"):]
    fc = fc[:fc.index("\n\n")]
    dispatched = {(int(s), int(w), EC_NIST if k == "EC_NIST" else EC_GENERAL) for s, w, k in re.findall(r"X\((\d+), (\d+), (EC_\w+)\)", fc)}
    assert (S, NW, kind) in dispatched
    inst = open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "ec_instances.h")).read()
    units = {u: (int(s), int(w), EC_NIST if k == "NIST" else EC_GENERAL)
             for u, s, w, k in re.findall(r"#define (VMN_UNIT_\w+)\(KW\) VMN_EC_INSTANCES\(KW, (\d+), (\d+), vmn::EC_(\w+)\)", inst)}
    unit = [u for u, v in units.items() if v == (S, NW, kind)]
    assert len(unit) == 1
    import __graft_entry__
    built = re.findall(r'"(inst_\w+\.hip)"', open(__graft_entry__.__file__).read())
    assert any("%s(template)" % unit[0] in open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", u)).read() for u in built)


def general_a_names():
    table, _ = library_table()
    return sorted(k for k, c in table.items() if c["a"] is not None)


@pytest.mark.parametrize("name", general_a_names())
def test_ecscalar_agrees_with_libcrypto(name):
    es = ecscalar()
    c = es.curve(name)
    a, G = es.curve_a(c), (c["gx"], c["gy"])
    rnd = random.Random(name)
    for k in (1, 2, 3, c["n"] - 1, rnd.randrange(c["n"]), rnd.randrange(c["n"])):
        assert es.mul(k, G, c["p"], c["n"], a) == openssl_mul(name, k), k
    assert es.mul(c["n"], G, c["p"], c["n"], a) is None
    P = es.mul(5, G, c["p"], c["n"], a)
    assert es.add(P, P, c["p"], a) == openssl_mul(name, 10)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hostcurve") / "hostcurve_harness")
    subprocess.run(["g++", "-std=c++17", "-O2", "-o", exe, os.path.join(ROOT, "tests", "hostcurve_harness.cpp")], check=True)
    return exe


@pytest.mark.parametrize("name", general_a_names())
def test_host_curve_with_a_general_a_agrees_with_libcrypto(name, harness):
    """csrc/hostcurve.h with `a` set (the O(1) points of a proof over these curves, vmnproofs.cpp): k G, 2 k G, k G + G."""
    es = ecscalar()
    c = es.curve(name)
    a = es.curve_a(c)
    cb = (c["p"].bit_length() + 7) // 8
    dec = lambda h: None if h == "ff" * (2 * cb) else (int(h[:2 * cb], 16), int(h[2 * cb:], 16))
    rnd = random.Random("host" + name)
    for k in (1, 2, c["n"] - 1, rnd.randrange(c["n"]), rnd.randrange(c["n"])):
        out = subprocess.run([harness] + ["%0*x" % (2 * cb, v) for v in (c["p"], a, c["gx"], c["gy"])] + ["%x" % k],
                             check=True, capture_output=True, text=True).stdout.split()
        assert [dec(h) for h in out] == [openssl_mul(name, k), openssl_mul(name, 2 * k % c["n"]), openssl_mul(name, (k + 1) % c["n"])], k


def test_golden_file_matches_the_table_and_the_host_scalars():
    """tests/golden/ec_named.json (libcrypto's k G, gen_golden_named_curves.py) against the library's table and ecscalar.py."""
    import json
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "ec_named.json")))
    table, _ = library_table()
    assert set(rec) == set(table)
    es = ecscalar()
    for name, r in rec.items():
        c = table[name]
        a = c["a"] if c["a"] is not None else c["p"] - 3
        assert [int(r[k], 16) for k in ("p", "a", "b", "n")] == [c["p"], a, c["b"], c["n"]] and [int(v, 16) for v in r["g"]] == [c["gx"], c["gy"]]
        for case in r["cases"][:3]:
            k = int(case["k"], 16)
            assert es.mul(k, (c["gx"], c["gy"]), c["p"], c["n"], a) == tuple(int(v, 16) for v in case["kG"]), (name, k)
