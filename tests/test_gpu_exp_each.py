"""GPU suite: vmn_garray_exp_scalars_multi -- k arrays of one size, each raised to an exponent of its OWN, over a modular group
in one launch per eight arrays (csrc/modp_shared_exp.h, EachArrays: every array walks its own schedule of steps, the window
width and the phase count are the launch's).  Bit-exact against the GMP oracle per array, at the sizes of
tests/test_gpu_exp_multi.py (one element, one short of / exactly / one past a tile of 256 elements, two tiles with a ragged
second one; one, two, three and nine arrays) with neighbouring arrays whose schedules differ in length by two orders of
magnitude; phases on a "device" of one or two workgroup slots where the short schedules have fewer steps than the launch
has phases, first and last in the launch.

Wall time on an MI355X: not measured yet, for this module and for the existing GPU modules beside it."""
import pytest

from conftest import load_golden
from oracle import pyref

pytestmark = pytest.mark.gpu

KMAX, NMAX = 9, 300
NAMES = ["full", "q-1", "1<<200", "(1<<33)+1"]


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


def check(S, got, names, n, note):
    assert len(got) == len(names)
    for c, name in enumerate(names):
        assert got[c].toInts() == S["want"][name][c][:n], (note, c, name)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 300])
@pytest.mark.parametrize("k", [1, 2, 3, 9])
def test_k_arrays_each_under_its_own_exponent_match_the_oracle_per_array(k, n, small, vmn):
    S = small
    X = upload(S, k, n)
    for shift in (0, 1):
        names = [NAMES[(c + shift) % 4] for c in range(k)]
        got = vmn.PGroupElementArray.expMultiEach(X, [S["exps"][name] for name in names])
        check(S, got, names, n, (k, n, shift))


def test_equal_exponents_give_what_one_exponent_for_all_gives(small, vmn):
    S = small
    X = upload(S, 3, 257)
    for name in NAMES:
        each = vmn.PGroupElementArray.expMultiEach(X, [S["exps"][name]] * 3)
        multi = vmn.PGroupElementArray.expMulti(X, S["exps"][name])
        assert [r.toInts() for r in each] == [r.toInts() for r in multi] == [S["want"][name][c][:257] for c in range(3)], name


@pytest.mark.parametrize("max_blocks", ["2", "1"])
@pytest.mark.parametrize("n", [200, 300])
def test_phases_across_arrays_with_schedules_of_different_lengths(n, max_blocks, small, vmn, monkeypatch):
    """Three arrays on a "device" of two (one) workgroup slots: the launch is cut into phases by its longest schedule, and the
    schedules of 1 << 200 and (1 << 33) + 1 have two steps -- one step of the main loop, so all but one of their phases are
    empty (load, store, hand over).  In both orders: the two-step schedule last and first in the launch."""
    S = small
    X = upload(S, 3, n)
    monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", max_blocks)
    order = ["full", "1<<200", "(1<<33)+1"]
    for names in (order, order[::-1]):
        got = vmn.PGroupElementArray.expMultiEach(X, [S["exps"][name] for name in names])
        check(S, got, names, n, (n, max_blocks, names))


@pytest.mark.parametrize("n", [7, 300])
def test_2048_bits_three_arrays_three_exponents_one_launch(n, vmn, gpu_ctx, oracle_for):
    """k n = 21 elements: the total chooses the widest geometry (eight lanes per element); 900: four lanes per element."""
    p, q, g = pyref.modp_group(2048)
    orc = oracle_for(p, q)
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    xs = [[pow(1 + v % (p - 1), 2, p) for v in pyref.stream_ints(b"multi2048/x%d" % c, n, p)] for c in range(3)]
    es = [v | (1 << (q.bit_length() - 2)) for v in pyref.stream_ints(b"each2048/e", 3, q)]
    assert len(set(es)) == 3
    X = [G.toElementArray(x, checked=False) for x in xs]
    got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMultiEach(X, es))
    assert count == 1
    for c in range(3):
        assert got[c].toInts() == orc.exp_scalar(xs[c], es[c]), (n, c)


def test_witness_launch_counts_fused_separate_and_short(small, vmn, gpu_ctx, monkeypatch):
    S = small
    n = 257
    X = upload(S, KMAX, n)
    names = [NAMES[c % 4] for c in range(KMAX)]
    es = [S["exps"][name] for name in names]
    for k, fused_launches in ((2, 1), (3, 1), (8, 1), (9, 2)):
        got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMultiEach(X[:k], es[:k]))
        assert count == fused_launches, (k, count)
        check(S, got, names[:k], n, k)
    monkeypatch.setenv("VMN_EXP_MULTI_FUSED", "0")                      # (read per call) one launch per array
    for k in (3, 9):
        got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMultiEach(X[:k], es[:k]))
        assert count == k, (k, count)
        check(S, got, names[:k], n, k)
    monkeypatch.delenv("VMN_EXP_MULTI_FUSED")
    # one exponent of at most 32 bits in the call: every array as vmn_garray_exp_scalar runs it, one after the other
    mixed = ["full", "short", "q-1"]
    got, count = launches(gpu_ctx, lambda: vmn.PGroupElementArray.expMultiEach(X[:3], [S["exps"][name] for name in mixed]))
    assert count == 3
    check(S, got, mixed, n, "short")


def test_bad_arguments_and_live_bytes(small, vmn, gpu_ctx):
    import ctypes as C
    S = small
    G = S["G"]
    A, B = upload(S, 2, 300)
    short = G.toElementArray(S["xs"][2][:299], checked=False)
    other = vmn.ModPGroup(gpu_ctx, S["p"], S["q"], S["g"])
    foreign = other.toElementArray(S["xs"][2][:300], checked=False)
    es = [S["full"], S["exps"]["q-1"], S["exps"]["1<<200"]]
    for r in vmn.PGroupElementArray.expMultiEach([A, B], es[:2]):      # (warm: scratch and pool blocks of these sizes exist)
        r.free()
    live0 = gpu_ctx.memory_stats()["live_bytes"]
    res = vmn.PGroupElementArray.expMultiEach([A, B, A], es)
    assert gpu_ctx.memory_stats()["live_bytes"] > live0
    for r in res:
        r.free()
    assert gpu_ctx.memory_stats()["live_bytes"] == live0
    for arrays in ([A, short], [A, B, foreign]):
        with pytest.raises(vmn.VmnError) as ei:
            vmn.PGroupElementArray.expMultiEach(arrays, es[:len(arrays)])
        assert ei.value.status == -1                                   # VMN_ERR_ARG
        assert gpu_ctx.memory_stats()["live_bytes"] == live0
    with pytest.raises(ValueError):
        vmn.PGroupElementArray.expMultiEach([], [])
    fn = vmn.lib().vmn_garray_exp_scalars_multi
    outs = (C.c_void_p * 2)()
    hs = (C.c_void_p * 2)(A._h, B._h)
    assert fn(hs, C.c_size_t(0), b"\x05", C.c_size_t(1), outs) == -1                  # k = 0
    assert fn(hs, C.c_size_t(2), None, C.c_size_t(1), outs) == -1                     # NULL es_be
    assert gpu_ctx.memory_stats()["live_bytes"] == live0


def test_p256_three_arrays_three_scalars_against_the_affine_curve(vmn, gpu_ctx):
    import random
    from oracle.pyref_ec import Curve
    c = Curve("P-256")
    G = vmn.ECqPGroup(gpu_ctx, "P-256")
    rnd = random.Random(256)
    pts = [[c.mul(rnd.randrange(1, c.n), c.g) for _ in range(24)] for _ in range(3)]
    pts[1][3] = None
    es = [rnd.randrange(1 << 250, c.n) for _ in range(3)]
    assert len(set(es)) == 3
    X = [G.toElementArray(x) for x in pts]
    got = vmn.PGroupElementArray.expMultiEach(X, es)
    for a in range(3):
        assert got[a].toInts() == [c.mul(es[a], P) if P is not None else None for P in pts[a]], a
