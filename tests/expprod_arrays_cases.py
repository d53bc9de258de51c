"""The cases of vmn_garray_expprod_arrays (pGroup.expProd(bases[], integers[], bitLength): out[i] = prod_j bases[j][i]^(c_j)) and
their expected values on Python integers and affine points.  tests/test_expprod_arrays_catalogue.py checks the list itself on the
CPU, tests/test_gpu_expprod_arrays.py runs it on the GPU, tests/test_expprod_schedule_host.py feeds its exponent sets to the host's
schedule builder.

A case: name, group (a key of GROUPS), n, `bases` (indices into the group's pool of arrays: an index may repeat), `ints` (signed,
one per base), `tags` (the situations the case stands for), `both_geometries` (run with the small-array threshold 0 and huge)."""
import os
import re
from functools import lru_cache

from conftest import ROOT
from oracle import pyref

import wide_decrypt_ref as W

EPB = 256              # elements per workgroup of the one-lane 2048-bit geometry (BLOCK / 1)
POOL = 9               # arrays per group: the launch limit + 1
MODP = {"g14": 2048, "g15": 3072, "g16": 4096, "g17": 6144}
CURVES = {"P-256": "P-256", "P-384": "P-384", "bp256": "brainpoolp256r1"}
CURVE_N = 4


def launch_limit():
    """EXPPROD_BASES as the kernels' header states it."""
    src = open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "modp_shared_exp.h")).read()
    return int(re.search(r"constexpr int EXPPROD_BASES = (\d+);", src).group(1))


@lru_cache(maxsize=None)
def group(key):
    """{"kind", "p", "q", "g" ...} of a group of the catalogue."""
    if key in MODP:
        p, q, g = pyref.modp_group(MODP[key])
        return dict(kind="modp", p=p, q=q, g=g)
    if key == "sub1024":
        from test_bytetree import group_descriptions
        d = group_descriptions()["ModPGroup_1024_256"]
        return dict(kind="modp", p=d["p"], q=d["q"], g=d["g"])
    from named_curves import ref_curve
    c = ref_curve(CURVES[key])
    return dict(kind="curve", curve=c, name=CURVES[key], q=c.n, p=c.p)


@lru_cache(maxsize=None)
def pool(key, n):
    """POOL arrays of n elements of the group.  Modular: squares mod p (for sub1024: powers of g), with 1 and p - 1 = -1 at index 0
    of arrays 0 and 1 (p - 1 is no subgroup element, but expProd does not ask).  Curves: multiples of g, with an infinity row in
    arrays 0 and 2, and array 1 holding -(array 0) at index 1: P and -P at the same index of two bases."""
    G = group(key)
    if G["kind"] == "modp":
        p = G["p"]
        if key == "sub1024":
            xs = [[pow(G["g"], e, p) for e in pyref.stream_ints(b"expprod/%s/%d" % (key.encode(), c), n, G["q"])] for c in range(POOL)]
        else:
            xs = [[pow(1 + v % (p - 1), 2, p) for v in pyref.stream_ints(b"expprod/%s/%d" % (key.encode(), c), n, p)] for c in range(POOL)]
        xs[0][0], xs[1][0] = 1, p - 1
        return xs
    c = G["curve"]
    xs = [[c.mul(1 + e % (c.n - 1), c.g) for e in pyref.stream_ints(b"expprod/%s/%d" % (key.encode(), a), n, c.n)] for a in range(POOL)]
    xs[0][0] = None
    xs[2][n - 1] = None
    xs[1][1] = c.neg(xs[0][1])
    return xs


def expected(case):
    """out[i] = prod_j bases[j][i]^(c_j) on Python integers (pow takes a negative exponent) resp. affine points."""
    G, xs = group(case["group"]), pool(case["group"], case["n"])
    out = []
    for i in range(case["n"]):
        if G["kind"] == "modp":
            acc = 1
            for b, c in zip(case["bases"], case["ints"]):
                acc = acc * pow(xs[b][i], c, G["p"]) % G["p"]
        else:
            cur, acc = G["curve"], None
            for b, c in zip(case["bases"], case["ints"]):
                P = cur.mul(abs(c) % cur.n, xs[b][i])
                acc = cur.add(acc, cur.neg(P) if c < 0 else P)
        out.append(acc)
    return out


def _case(name, grp, n, ints, tags, bases=None, both=False):
    return dict(name=name, group=grp, n=n, ints=list(ints), bases=list(bases) if bases is not None else list(range(len(ints))),
                tags=set(tags), both_geometries=both)


def _full(key, count):
    """`count` exponents of exactly bits(q) bits, signs alternating"""
    q = group(key)["q"]
    top = 1 << (q.bit_length() - 1)
    vals = [(v % top) | top for v in pyref.stream_ints(b"expprod/full/" + key.encode(), count, q)]
    return [v if j % 2 == 0 else -v for j, v in enumerate(vals)]


def lagrange_cases(key, n):
    """parties {1,2}, {1,3}, {2,3} of 3 at threshold 2: the integers combineDecryptionFactors uses"""
    q = group(key)["q"]
    out = []
    for name, correct in (("12", [0, 1, 1, 0]), ("13", [0, 1, 0, 1]), ("23", [0, 0, 1, 1])):
        ints = W.lagrange_integers(q, correct, 3, 2)
        out.append(_case("lagrange_%s_%s" % (name, key), key, n, ints, {"lagrange"}))
    return out


@lru_cache(maxsize=None)
def catalogue():
    L = launch_limit()
    spread = [3 + 2 * j if j % 3 else -(5 + 2 * j) for j in range(POOL)]          # small odd integers of both signs
    wide64 = [(v | (1 << 63)) * (-1 if j % 2 else 1) for j, v in enumerate(pyref.stream_ints(b"expprod/64", POOL, 1 << 63))]
    cases = []
    # sizes per geometry
    for n in (1, EPB - 1, EPB, EPB + 1):
        cases.append(_case("g14_n%d" % n, "g14", n, (2, -1), {"size_2048_n%d" % n, "benchmark_2_-1"}, both=True))
    cases.append(_case("g15_n65", "g15", 65, (2, -1, 3), {"size_3072_n65"}, both=True))
    cases.append(_case("g16_n65", "g16", 65, (2, -1, 3), {"size_4096_n65"}))
    cases.append(_case("g17_n3", "g17", 3, (2, -1, 3), {"size_8192_n3"}))
    cases.append(_case("sub1024_n5", "sub1024", 5, (_full("sub1024", 1)[0], -3, 2), {"group_1024_256"}))
    # exponent sets, over group 14 and every curve
    for key in ("g14",) + tuple(CURVES):
        n = 5 if key == "g14" else CURVE_N
        q = group(key)["q"]
        add = lambda name, ints, tags, bases=None: cases.append(_case("%s_%s" % (name, key), key, n, ints, tags, bases))
        add("copy", (1,), {"k1_copy", "one_bit"})
        add("inverse", (-1,), {"k1_inverse", "one_bit"})
        if key != "g14":
            add("two_minus_one", (2, -1), {"benchmark_2_-1", "infinity_rows", "p_and_minus_p"})
        add("all_positive", (3, 5, 7), {"all_positive"})
        add("all_negative", (-3, -5, -7), {"all_negative"})
        add("k4", wide64[:4], {"k4"})
        add("k5", wide64[:5], {"k5"})
        add("k_limit", spread[:L], {"k_limit"})
        add("k_limit_plus_1", spread[:L + 1], {"k_limit_plus_1"})
        add("zero_in_the_middle", (3, 0, -2), {"zero_in_the_middle"})
        add("all_zero", (0, 0), {"all_zero"})
        add("zero_run", ((1 << 40) + 1, -((1 << 35) + 1), 1 << 33), {"zero_run_above_32", "one_bit"})
        add("same_array_twice", (3, -2), {"same_array_twice"}, bases=(3, 3))
        add("same_array_equal_exponents", (5, 5, -1), {"same_array_equal_exponents"}, bases=(3, 3, 4))
        add("length_gap", (1 << (q.bit_length() - 1), 1), {"length_gap", "one_bit"})
        cases.append(_case("full_length_%s" % key, key, 3, _full(key, 3), {"full_length_3"}))
    cases += lagrange_cases("g14", 17) + lagrange_cases("P-256", CURVE_N)
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


# every situation the GPU suite must meet, by tag
REQUIRED_TAGS = ["size_2048_n1", "size_2048_n%d" % (EPB - 1), "size_2048_n%d" % EPB, "size_2048_n%d" % (EPB + 1), "size_3072_n65",
                 "size_4096_n65", "size_8192_n3", "group_1024_256", "k1_copy", "k1_inverse", "benchmark_2_-1", "all_positive",
                 "all_negative", "k4", "k5", "k_limit", "k_limit_plus_1", "zero_in_the_middle", "all_zero", "zero_run_above_32",
                 "full_length_3", "same_array_twice", "same_array_equal_exponents", "infinity_rows", "p_and_minus_p", "lagrange",
                 "one_bit", "length_gap"]
