"""GPU suite: vmn_garray_exp_scalar_multi -- k arrays of one size raised to ONE exponent, over a modular group in one launch
per eight arrays (csrc/modp_shared_exp.h: global tile T = array T / ntiles, tile T % ntiles).  Bit-exact against the GMP
oracle per array, at the sizes where the index arithmetic can go wrong: one element, one short of / exactly / one past a
tile (256 elements per tile at 512 bits), two tiles with a ragged second one; one, two, three and nine arrays (nine = a launch
of eight and one of one); phases that cross array boundaries on a "device" of one or two workgroup slots.

Wall time on an MI355X: not measured yet, for this module and for the existing GPU modules beside it."""
import pytest

from conftest import load_golden
from oracle import pyref

pytestmark = pytest.mark.gpu

KMAX, NMAX = 9, 300


@pytest.fixture(scope="module")
def small(vmn, gpu_ctx, oracle_for):
    """The 512-bit group, nine arrays of 300 elements and their powers under the five exponents (computed once: a power of a
    prefix of an array is the prefix of the array's powers)."""
    grp, _ = load_golden(512)
    p, q, g = grp["p"], grp["q"], grp["g"]
    orc = oracle_for(p, q)
    xs = [[pow(1 + v % (p - 1), 2, p) for v in pyref.stream_ints(b"multi/x%d" % c, NMAX, p)] for c in range(KMAX)]
    xs[0][0], xs[1][0] = 1, p - 1
    full = pyref.stream_ints(b"multi/e", 1, q)[0] | (1 << (q.bit_length() - 2))
    exps = {"full": full, "q-1": q - 1, "1<<200": 1 << 200, "(1<<33)+1": (1 << 33) + 1, "short": 0xC0FFEE11}
    want = {name: [orc.exp_scalar(x, e) for x in xs] for name, e in exps.items()}
    return dict(G=vmn.ModPGroup(gpu_ctx, p, q, g), p=p, q=q, g=g, xs=xs, exps=exps, want=want, full=full)


def upload(S, k, n):
    return [S["G"].toElementArray(S["xs"][c][:n], checked=False) for c in range(k)]


def launches(ctx, fn):
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        out = fn()
        return out, ctx.timing_get("modpow")[0]
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 300])
@pytest.mark.parametrize("k", [1, 2, 3, 9])
def test_k_arrays_under_one_exponent_match_the_oracle_per_array(k, n, small, vmn):
    S = small
    X = upload(S, k, n)
    for name, e in S["exps"].items():
        got = vmn.PGroupElementArray.expMulti(X, e)
        assert len(got) == k
        for c in range(k):
            assert got[c].toInts() == S["want"][name][c][:n], (name, k, n, c)


@pytest.mark.parametrize("n", [7, 300])
def test_2048_bits_three_arrays(n, vmn, gpu_ctx, oracle_for):
    """k n = 21 elements: the total chooses the widest geometry (eight lanes per element); 900: four lanes per element."""
    p, q, g = pyref.modp_group(2048)
    orc = oracle_for(p, q)
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    xs = [[pow(1 + v % (p - 1), 2, p) for v in pyref.stream_ints(b"multi2048/x%d" % c, n, p)] for c in range(3)]
    full = pyref.stream_ints(b"multi2048/e", 1, q)[0] | (1 << (q.bit_length() - 2))
    X = [G.toElementArray(x, checked=False) for x in xs]
    got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMulti(X, full))
    assert count == 1
    for c in range(3):
        assert got[c].toInts() == orc.exp_scalar(xs[c], full), (n, c)


@pytest.mark.parametrize("max_blocks", ["2", "1"])
@pytest.mark.parametrize("n", [200, 300])
def test_phases_cross_array_boundaries(n, max_blocks, small, vmn, monkeypatch):
    """Three arrays on a "device" of two (one) workgroup slots.  n = 200: one tile per array -- no array alone would be phased,
    the three together are; n = 300: two tiles per array, the units of a phase run through all six."""
    S = small
    X = upload(S, 3, n)
    monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", max_blocks)
    for name in ("full", "q-1", "1<<200", "(1<<33)+1"):
        got = vmn.PGroupElementArray.expMulti(X, S["exps"][name])
        for c in range(3):
            assert got[c].toInts() == S["want"][name][c][:n], (name, n, max_blocks, c)


def test_the_same_array_twice(small, vmn):
    S = small
    A, B = upload(S, 2, 257)
    got = vmn.PGroupElementArray.expMulti([A, B, A], S["full"])
    assert [r.toInts() for r in got] == [S["want"]["full"][0][:257], S["want"]["full"][1][:257], S["want"]["full"][0][:257]]


def test_witness_launch_counts_fused_and_separate(small, vmn, gpu_ctx, monkeypatch):
    S = small
    n = 257
    X = upload(S, KMAX, n)
    want = [S["want"]["full"][c][:n] for c in range(KMAX)]
    for k, fused_launches in ((1, 1), (2, 1), (3, 1), (8, 1), (9, 2)):
        got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMulti(X[:k], S["full"]))
        assert count == fused_launches, (k, count)
        assert [r.toInts() for r in got] == want[:k]
    monkeypatch.setenv("VMN_EXP_MULTI_FUSED", "0")                      # (read per call) the parent's way: one launch per array
    for k in (3, 9):
        got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMulti(X[:k], S["full"]))
        assert count == k, (k, count)
        assert [r.toInts() for r in got] == want[:k]
    monkeypatch.delenv("VMN_EXP_MULTI_FUSED")
    # exponents of at most 32 bits: the fixed-window kernel, array by array
    got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMulti(X[:3], S["exps"]["short"]))
    assert count == 3 and [r.toInts() for r in got] == [S["want"]["short"][c][:n] for c in range(3)]


def test_bad_arguments_and_live_bytes(small, vmn, gpu_ctx):
    S = small
    G = S["G"]
    A, B = upload(S, 2, 300)
    short = G.toElementArray(S["xs"][2][:299], checked=False)
    other = vmn.ModPGroup(gpu_ctx, S["p"], S["q"], S["g"])
    foreign = other.toElementArray(S["xs"][2][:300], checked=False)
    for r in vmn.PGroupElementArray.expMulti([A, B], S["full"]):      # (warm: scratch and pool blocks of these sizes exist)
        r.free()
    live0 = gpu_ctx.memory_stats()["live_bytes"]
    res = vmn.PGroupElementArray.expMulti([A, B, A], S["full"])
    assert gpu_ctx.memory_stats()["live_bytes"] > live0
    for r in res:
        r.free()
    assert gpu_ctx.memory_stats()["live_bytes"] == live0
    for arrays in ([A, short], [A, B, foreign]):
        with pytest.raises(vmn.VmnError) as ei:
            vmn.PGroupElementArray.expMulti(arrays, S["full"])
        assert ei.value.status == -1                                   # VMN_ERR_ARG
        assert gpu_ctx.memory_stats()["live_bytes"] == live0
    with pytest.raises(ValueError):
        vmn.PGroupElementArray.expMulti([], S["full"])
    import ctypes as C
    outs = (C.c_void_p * 1)()
    assert vmn.lib().vmn_garray_exp_scalar_multi((C.c_void_p * 1)(A._h), C.c_size_t(0), b"\x05", C.c_size_t(1), outs) == -1      # k = 0
    assert gpu_ctx.memory_stats()["live_bytes"] == live0


def test_p256_three_arrays_against_the_affine_curve(vmn, gpu_ctx):
    import random
    from oracle.pyref_ec import Curve
    c = Curve("P-256")
    G = vmn.ECqPGroup(gpu_ctx, "P-256")
    rnd = random.Random(256)
    pts = [[c.mul(rnd.randrange(1, c.n), c.g) for _ in range(24)] for _ in range(3)]
    pts[1][3] = None
    e = rnd.randrange(1 << 250, c.n)
    X = [G.toElementArray(x) for x in pts]
    got = vmn.PGroupElementArray.expMulti(X, e)
    for a in range(3):
        assert got[a].toInts() == [c.mul(e, P) if P is not None else None for P in pts[a]], a
