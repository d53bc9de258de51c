"""GPU suite: vmn_garray_expprod_arrays -- pGroup.expProd(bases[], integers[], bitLength), out[i] = prod_j bases[j][i]^(c_j) with
signed integers c_j, one chain of squarings (doublings) for all bases (k_modpow_expprod, k_ec_expprod).  Every case of
tests/expprod_arrays_cases.py bit for bit against Python's pow resp. the affine curve reference; the argument errors; the
Lagrange cases against the host sequence the call replaces (exp_scalar / mul / inv); vmn_combine_decryption_factors_wide at
width 2 against tests/wide_decrypt_ref.py with its launches counted; plaintext recovery as one call.

Wall time on an MI355X: 4 s for the module's 94 tests, the slowest 0.9 s."""
import ctypes as C

import pytest

import expprod_arrays_cases as X
import wide_decrypt_ref as W

pytestmark = pytest.mark.gpu

DEFAULT_WIDE = 40960
CASES = X.catalogue()
RUNS = [(c["name"], g) for c in CASES for g in (("narrow", "wide") if c["both_geometries"] else ("default",))]
BY_NAME = {c["name"]: c for c in CASES}


@pytest.fixture(scope="module")
def groups(vmn, gpu_ctx):
    made = {}

    def get(key):
        if key not in made:
            G = X.group(key)
            made[key] = vmn.ModPGroup(gpu_ctx, G["p"], G["q"], G["g"]) if G["kind"] == "modp" else vmn.ECqPGroup(gpu_ctx, G["name"])
        return made[key]
    return get


@pytest.fixture(scope="module")
def nat(entry):
    import mirror
    return mirror.load(entry, ("native",))["native"]


def upload(groups, key, n, bases):
    G, xs = groups(key), X.pool(key, n)
    arrs = {b: G.toElementArray(xs[b], checked=False) for b in set(bases)}
    return [arrs[b] for b in bases]


@pytest.mark.parametrize("name,geometry", RUNS)
def test_case_matches_python_bit_for_bit(name, geometry, groups, gpu_ctx):
    case = BY_NAME[name]
    G = groups(case["group"])
    bases = upload(groups, case["group"], case["n"], case["bases"])
    if geometry != "default":
        gpu_ctx.set_small_array_threshold(0 if geometry == "narrow" else 2 ** 63)
    try:
        got = G.expProd(bases, case["ints"]).toInts()
        tight = G.expProd(bases, case["ints"], max(1, max(abs(c).bit_length() for c in case["ints"]))).toInts()
    finally:
        gpu_ctx.set_small_array_threshold(DEFAULT_WIDE)
    assert got == X.expected(case), name
    assert tight == got, name


def raw(vmn, arrays, abs_ints, neg, ebytes, bitlen, k=None):
    k = len(arrays) if k is None else k
    hs = (C.c_void_p * max(1, len(arrays)))(*[a._h for a in arrays])
    out = C.c_void_p(0x5a5a)
    rc = vmn.lib().vmn_garray_expprod_arrays(hs, C.c_size_t(k), b"".join(v.to_bytes(ebytes, "big") for v in abs_ints), C.c_size_t(ebytes),
                                             (C.c_int * max(1, len(neg)))(*neg), C.c_int(bitlen), C.byref(out))
    return rc, out.value


def test_argument_errors_leave_the_output_untouched(vmn, groups):
    A = upload(groups, "g14", 5, [0, 1])
    B = upload(groups, "g15", 5, [0])
    S = upload(groups, "g14", 17, [0])
    ERR_ARG = -1
    assert raw(vmn, [A[0], B[0]], [2, 1], [0, 1], 8, 0) == (ERR_ARG, 0x5a5a)              # two groups
    assert raw(vmn, [A[0], S[0]], [2, 1], [0, 1], 8, 0) == (ERR_ARG, 0x5a5a)              # two sizes
    assert raw(vmn, A, [2, 1], [0, 1], 8, 0, k=0) == (ERR_ARG, 0x5a5a)                    # no arrays
    assert raw(vmn, A, [4, 1], [0, 1], 8, 2) == (ERR_ARG, 0x5a5a)                         # bitlen one below the true length
    assert raw(vmn, A, [2, 1], [0, 1], 8, 65) == (ERR_ARG, 0x5a5a)                        # bitlen > 8 * ebytes
    rc, h = raw(vmn, A, [4, 1], [0, 1], 8, 3)
    assert rc == 0 and h not in (0, 0x5a5a)
    vmn.PGroupElementArray(groups("g14"), C.c_void_p(h)).free()


def test_empty_arrays_give_an_empty_array(groups):
    G = groups("g14")
    E = G.toElementArray([])
    assert G.expProd([E, E], [2, -1]).toInts() == []


@pytest.mark.parametrize("name", [c["name"] for c in CASES if "lagrange" in c["tags"]])
def test_lagrange_cases_equal_the_host_sequence_they_replace(name, groups):
    case = BY_NAME[name]
    G = groups(case["group"])
    bases = upload(groups, case["group"], case["n"], case["bases"])
    pos = neg = None
    for b, c in zip(bases, case["ints"]):
        if c == 0:
            continue
        t = b.exp(abs(c))
        if c > 0:
            pos = t if pos is None else pos.mul(t)
        else:
            neg = t if neg is None else neg.mul(t)
    old = pos if neg is None else (neg.inv() if pos is None else pos.mul(neg.inv()))
    assert G.expProd(bases, case["ints"]).toBytes() == old.toBytes() and old.toInts() == X.expected(case), name


@pytest.mark.parametrize("key", ["g14", "P-256"])
def test_combine_is_one_launch_per_component_and_equals_the_restatement(key, groups, nat, gpu_ctx):
    n, k, thr, width = 17, 3, 2, 2
    G, info = groups(key), X.group(key)
    K = W.adapter_modp(info["p"], info["q"]) if info["kind"] == "modp" else W.adapter_curve(info["curve"])
    xs = X.pool(key, n)
    factors = [None] + [[xs[(l - 1) * width + c] for c in range(width)] for l in range(1, k + 1)]
    if info["kind"] == "modp":
        factors[1][1] = [xs[8][0]] + xs[1][1:]          # (the reference reduces the integers mod q: subgroup elements only, no p - 1)
    F = [None] + [[G.toElementArray(a, checked=False) for a in factors[l]] for l in range(1, k + 1)]
    for correct in ([0, 1, 1, 0], [0, 1, 0, 1], [0, 0, 1, 1], [0, 1, 1, 1]):
        want = W.combine_decryption_factors(K, factors, correct, k, thr)
        gpu_ctx.timing_enable(True)
        try:
            gpu_ctx.timing_reset()
            got = nat.combineDecryptionFactors(F, correct, k, thr, info["q"])
            launches, powers = gpu_ctx.timing_get("expprod_arrays")[0], gpu_ctx.timing_get("modpow")[0]
        finally:
            gpu_ctx.timing_enable(False)
            gpu_ctx.timing_reset()
        assert [a.toInts() for a in got] == want, correct
        assert (launches, powers) == (width, 0), (correct, launches, powers)


@pytest.mark.parametrize("key", ["g14", "P-256"])
def test_plaintext_recovery_is_the_same_call_with_v_under_exponent_one(key, groups):
    G, q, n = groups(key), X.group(key)["q"], (17 if key == "g14" else X.CURVE_N)
    lam = W.lagrange_integers(q, [0, 1, 1, 0], 3, 2)
    v, f1, f2 = upload(groups, key, n, [5, 0, 1])
    one_call = G.expProd([v, f1, f2], [1] + lam)
    assert one_call.toBytes() == v.mul(G.expProd([f1, f2], lam)).toBytes()
