"""GPU suite: curve powers under ONE scalar -- vmn_garray_exp_scalar, vmn_garray_exp_scalar_multi and
vmn_garray_exp_scalars_multi over ECqPGroup through k_ec_mulshared (csrc/ec_kernels.h): the scalar recoded into signed odd digits
on the host (csrc/ec_shared_schedule.h), a table of 2^(w-2) odd multiples per lane slot, the arrays of a call in one launch.

Every value is compared with affine arithmetic on Python integers (oracle.pyref_ec.Curve; tests/named_curves.py for the curves
with a general a), never with the code under test; the A/B arm VMN_EC_SHARED=0 (k_ec_mulvar, array by array) is compared as
bytes on top of that.  The reference multiplies by a scalar through a table of 4-bit windows of the base built with Curve.add
(FixedBase below, pinned against Curve.mul), because the catalogue holds some fifty scalars: the points of an array are small
multiples of the generator and of one seeded point, so a scalar costs two such multiplications per curve.

Wall time on an MI355X: about 10 s for the module, of which the two decryption sessions take 4.3 s and 2.5 s (their Python
restatements); no other test above half a second."""
import random

import pytest

from oracle.pyref_ec import Curve
from tape import Tape

import ec_shared_cases as X
import keyed_decrypt_ref as KD
import wide_decrypt_ref as W
from named_curves import ref_curve

pytestmark = pytest.mark.gpu

# one curve per instance of VMN_FOR_CURVES (csrc/vmnhip.hip): (limbs, kind) -> name
INSTANCES = {(9, "nist"): "P-224", (10, "nist"): "P-256", (15, "nist"): "P-384", (21, "nist"): "P-521",
             (9, "general"): "brainpoolp224r1", (10, "general"): "brainpoolp256r1", (13, "general"): "brainpoolp320r1",
             (15, "general"): "brainpoolp384r1", (21, "general"): "brainpoolp512r1"}


def curve(name):
    return Curve(name) if name in ("P-224", "P-256", "P-384", "P-521") else ref_curve(name)


class FixedBase:
    """e * B for many scalars e: the table d 16^i B (d < 16) by Curve.add, then one addition per 4-bit window."""

    def __init__(self, c, B):
        self.c, self.rows = c, []
        for _ in range((c.n.bit_length() + 3) // 4):
            row = [None]
            for _ in range(15):
                row.append(c.add(row[-1], B))
            self.rows.append(row)
            B = c.add(row[15], B)

    def mul(self, e):
        e %= self.c.n
        R = None
        for i, row in enumerate(self.rows):
            R = self.c.add(R, row[(e >> (4 * i)) & 15])
        return R


_cases = {}


def case(name):
    """(curve, 24 points, {scalar: their multiples}) -- the points: infinity, G, -G, a seeded point B twice, j G (j = 2 ... 10),
    j B (j = 2 ... 11); the reference of e (j B) is j (e B)."""
    if name not in _cases:
        c = curve(name)
        rnd = random.Random("ec-shared/" + name)
        B = c.mul(rnd.randrange(1, c.n), c.g)
        small = [(0, 0), (1, 1), (1, -1), (2, 1), (2, 1)] + [(1, j) for j in range(2, 11)] + [(2, j) for j in range(2, 12)]
        base = {1: c.g, 2: B}
        pts = [None if which == 0 else (c.mul(j, base[which]) if j > 0 else c.neg(base[which])) for which, j in small]
        assert len(pts) == 24 and pts.count(B) == 2
        fixed = {1: FixedBase(c, c.g), 2: FixedBase(c, B)}
        probe = rnd.randrange(1, c.n)
        assert fixed[2].mul(probe) == c.mul(probe, B)                     # (the helper against the oracle's own multiplication)
        want = {}

        def multiples(e):
            if e not in want:
                R = {which: fixed[which].mul(e) for which in (1, 2)}
                want[e] = [None if which == 0 else (c.mul(j, R[which]) if j > 0 else c.neg(R[which])) for which, j in small]
            return want[e]
        _cases[name] = (c, pts, multiples)
    return _cases[name]


_groups = {}


@pytest.fixture
def ecgroup(vmn, gpu_ctx):
    def get(name):
        if name not in _groups:
            _groups[name] = vmn.ECqPGroup(gpu_ctx, name)
        return _groups[name]
    return get


@pytest.fixture(autouse=True)
def nothing_left_on_the_device():
    """Arrays that a test leaves in a reference cycle (a caught exception's traceback holds the frame that holds them, the
    sessions hold their instance) would be freed whenever Python next collects cycles -- inside a later module's test that
    counts live bytes.  Collect them here."""
    yield
    import gc
    gc.collect()


def launches(ctx, fn):
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        out = fn()
        return out, ctx.timing_get("modpow")[0]
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()


# ---- every instance, every window ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [INSTANCES[k] for k in sorted(INSTANCES)])
def test_every_catalogue_scalar_on_every_instance(name, ecgroup):
    c, pts, multiples = case(name)
    G = ecgroup(name)
    Xs = G.toElementArray(pts)
    for label, e in X.catalogue(c.n):
        assert Xs.exp(e).toInts() == multiples(e), (name, label)


@pytest.mark.parametrize("w", list(X.WINDOWS))
@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1"])
def test_every_catalogue_scalar_under_every_forced_window(name, w, ecgroup, monkeypatch):
    c, pts, multiples = case(name)
    G = ecgroup(name)
    Xs = G.toElementArray(pts)
    monkeypatch.setenv("VMN_EC_SHARED_WINDOW", str(w))
    for label, e in X.catalogue(c.n):
        assert Xs.exp(e).toInts() == multiples(e), (name, w, label)


# ---- tiles and arrays ----------------------------------------------------------------------------------------------------
N_TILES = 261                                   # one full tile of 256 points and a ragged one


@pytest.fixture(scope="module")
def tiled():
    """Three arrays of 261 points over P-256, array a the progression B_a + i D_a (additions only), so that e (B_a + i D_a) =
    e B_a + i (e D_a) costs the reference two multiplications per array and scalar."""
    c = Curve("P-256")
    rnd = random.Random("ec-shared/tiles")
    arrays, starts = [], []
    for a in range(3):
        B, D = c.mul(rnd.randrange(1, c.n), c.g), c.mul(rnd.randrange(1, c.n), c.g)
        pts = [B]
        for _ in range(N_TILES - 1):
            pts.append(c.add(pts[-1], D))
        arrays.append(pts)
        starts.append((B, D))
    pos = [sorted(set(rnd.sample(range(N_TILES), 24)) | set(range(255, 261))) for _ in range(3)]
    full = [rnd.randrange(1 << 255, c.n) for _ in range(2)]
    return dict(c=c, arrays=arrays, starts=starts, pos=pos, full=full, want={})


def want_at(T, a, e, i):
    c = T["c"]
    if (a, e) not in T["want"]:
        B, D = T["starts"][a]
        T["want"][(a, e)] = (c.mul(e % c.n, B), c.mul(e % c.n, D))
    eB, eD = T["want"][(a, e)]
    return c.add(eB, c.mul(i, eD))


@pytest.mark.parametrize("max_blocks", [None, "2", "1"])
def test_three_arrays_of_two_tiles_on_one_and_two_workgroup_slots(max_blocks, tiled, ecgroup, vmn, monkeypatch):
    """VMN_MODPOW_MAX_BLOCKS = 1: one workgroup slot walks all six tiles and rebuilds its table across arrays; an array under
    the scalar 0 lies first in the launch, one under 1 (a schedule of one step) last."""
    T = tiled
    c, G = T["c"], ecgroup("P-256")
    Xs = [G.toElementArray(pts) for pts in T["arrays"]]
    q = c.n
    calls = [("multi", [T["full"][0]] * 3), ("each", [T["full"][0], 1 << 200, q - 1]), ("each", [0, T["full"][1], 1])]
    if max_blocks is not None:
        monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", max_blocks)
    for kind, es in calls:
        run = (lambda: vmn.PGroupElementArray.expMulti(Xs, es[0])) if kind == "multi" else (lambda: vmn.PGroupElementArray.expMultiEach(Xs, es))
        got, count = launches(G.ctx, run)
        assert count == 1, (kind, es, count)
        ints = [r.toInts() for r in got]
        for a in range(3):
            assert len(ints[a]) == N_TILES
            for i in T["pos"][a]:
                assert ints[a][i] == want_at(T, a, es[a], i), (max_blocks, kind, a, i)
        monkeypatch.setenv("VMN_EC_SHARED", "0")                          # the parent's path: the same call, every position
        old, old_count = launches(G.ctx, run)
        monkeypatch.delenv("VMN_EC_SHARED")
        assert old_count == 3
        assert [r.toBytes() for r in got] == [r.toBytes() for r in old], (max_blocks, kind)


# ---- launch witnesses ----------------------------------------------------------------------------------------------------
def test_witness_one_launch_per_eight_arrays(ecgroup, vmn, monkeypatch):
    c, pts, multiples = case("P-256")
    G = ecgroup("P-256")
    rnd = random.Random("ec-shared/witness")
    es = [rnd.randrange(1 << 255, c.n) for _ in range(9)]
    Xs = [G.toElementArray(pts[a:] + pts[:a]) for a in range(9)]
    rot = lambda vals, a: vals[a:] + vals[:a]

    def check(got, scalars, note):
        for a, r in enumerate(got):
            assert r.toInts() == rot(multiples(scalars[a]), a), (note, a)

    for k, fused in ((1, 1), (2, 1), (3, 1), (8, 1), (9, 2)):
        got, count = launches(G.ctx, lambda: vmn.PGroupElementArray.expMultiEach(Xs[:k], es[:k]))
        assert count == fused, ("each", k, count)
        check(got, es[:k], ("each", k))
        got, count = launches(G.ctx, lambda: vmn.PGroupElementArray.expMulti(Xs[:k], es[0]))
        assert count == fused, ("multi", k, count)
        check(got, [es[0]] * k, ("multi", k))
    got, count = launches(G.ctx, lambda: Xs[0].exp(es[1]))
    assert count == 1 and got.toInts() == multiples(es[1])
    for knob in ("VMN_EXP_MULTI_FUSED", "VMN_EC_SHARED"):                  # (both read per call) one launch per array
        monkeypatch.setenv(knob, "0")
        for k in (1, 2, 3, 8, 9):
            got, count = launches(G.ctx, lambda: vmn.PGroupElementArray.expMultiEach(Xs[:k], es[:k]))
            assert count == k, (knob, "each", k, count)
            check(got, es[:k], (knob, "each", k))
            got, count = launches(G.ctx, lambda: vmn.PGroupElementArray.expMulti(Xs[:k], es[0]))
            assert count == k, (knob, "multi", k, count)
            check(got, [es[0]] * k, (knob, "multi", k))
        monkeypatch.delenv(knob)
    # every scalar = 0 modulo the order: no launch, arrays of infinity
    q = c.n
    for run in (lambda: vmn.PGroupElementArray.expMultiEach(Xs[:3], [0, q, 2 * q]), lambda: vmn.PGroupElementArray.expMulti(Xs[:3], q),
                lambda: [Xs[0].exp(0)]):
        got, count = launches(G.ctx, run)
        assert count == 0
        for r in got:
            assert r.toInts() == [None] * 24
    # nine arrays whose second launch holds a zero scalar only: that launch is not made
    got, count = launches(G.ctx, lambda: vmn.PGroupElementArray.expMultiEach(Xs, es[:8] + [q]))
    assert count == 1
    check(got, es[:8] + [0], "zero tail")


# ---- decryption ----------------------------------------------------------------------------------------------------------
NE, NV = 100, 100


@pytest.fixture(scope="module")
def nat(entry):
    import mirror
    return mirror.load(entry, ("native",))["native"]


def test_a_partys_factors_at_width_three_are_one_launch(nat, ecgroup, vmn):
    from test_gpu_wide_decrypt import gpu_session, ints_of
    c = Curve("P-256")
    G, K, q, g = ecgroup("P-256"), W.adapter_curve(c), c.n, c.g
    n, k, thr, width = 40, 2, 2, 3
    t = Tape(b"ec-shared/wide", q)
    coeffs = t.ring_array(thr)
    xs = [None] + [sum(cf * pow(j, d, q) for d, cf in enumerate(coeffs)) % q for j in range(1, k + 1)]
    ys = [None] + [K.exp(g, xj) for xj in xs[1:]]
    y = K.exp(g, coeffs[0])
    u = [K.exp_fixed(g, t.ring_array(n)) for _ in range(width)]
    I = dict(G=G, q=q, xs=xs, ys=ys, e=t.int_array(n, NE), chal=t.int_array(1, NV)[0])
    U = [G.toElementArray(col) for col in u]
    F, f_o = [None], [None]
    for j in range(1, k + 1):
        f, count = launches(G.ctx, lambda: nat.decryptionFactors(U, xs[j], q, k))
        assert count == 1, (j, count)
        f_o.append(W.decryption_factors(K, u, xs[j], k))
        assert ints_of(f) == f_o[j], j
        F.append(f)
    seed = b"ec-shared/party/"
    ref = W.run_session(K, g, u, ys, xs, f_o, I["e"], I["chal"], k, thr, lambda j: Tape(seed + b"%d" % j, q))
    got = gpu_session(nat, I, U, F, k, thr, seed)
    for j in range(1, k + 1):
        assert got["commit"][j] == ref["commit"][j] and got["reply"][j] == ref["reply"][j], j
        assert got["verifier"].verify(j, I["chal"]) == ref["verifier"].verify(j, I["chal"]) == True, j
    assert not got["verifier"].verify(1, I["chal"] + 1)
    correct = [False] + [True] * k
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    assert ints_of(comb) == W.combine_decryption_factors(K, f_o, correct, k, thr)
    got["verifier"].combine(correct, y, comb)
    got["verifier"].batchCombined()
    assert got["verifier"].verifyCombined(I["chal"]) and not got["verifier"].verifyCombined(I["chal"] + 1)


def test_a_partys_factors_under_a_key_of_width_two_are_one_launch(nat, ecgroup, vmn):
    from test_gpu_keyed_decrypt import gpu_session, ints_of
    c = Curve("P-256")
    G, K, q, g = ecgroup("P-256"), W.adapter_curve(c), c.n, c.g
    n, k, thr, kw, omega = 40, 2, 2, 2, 2
    t = Tape(b"ec-shared/keyed", q)
    xs, ys, y = KD.shamir_keys(K, g, t, kw, k, thr)
    msgs, u, v = KD.encrypt(K, g, y, t, kw, omega, n)
    I = dict(G=G, q=q, kw=kw, xs=xs, ys=ys, e=t.int_array(n, NE), chal=t.int_array(1, NV)[0])
    U = [G.toElementArray(col) for col in u]
    assert len(U) == 4 and len(set(xs[1])) == 2                          # four arrays under two secrets
    F, f_o = [None], [None]
    for j in range(1, k + 1):
        f, count = launches(G.ctx, lambda: nat.decryptionFactors(U, list(xs[j]), q, k))
        assert count == 1, (j, count)
        f_o.append(KD.decryption_factors(K, kw, u, xs[j], k))
        assert ints_of(f) == f_o[j], j
        F.append(f)
    seed = b"ec-shared/keyed-party/"
    ref = KD.run_session(K, g, kw, u, ys, xs, f_o, I["e"], I["chal"], k, thr, lambda j: Tape(seed + b"%d" % j, q))
    got = gpu_session(nat, I, U, F, k, thr, seed)
    for j in range(1, k + 1):
        assert got["commit"][j] == ref["commit"][j] and got["reply"][j] == ref["reply"][j], j
        assert got["verifier"].verify(j, I["chal"]) == ref["verifier"].verify(j, I["chal"]) == True, j
    correct = [False] + [True] * k
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    assert ints_of(comb) == KD.combine_decryption_factors(K, f_o, correct, k, thr)
    assert ints_of(nat.plaintexts([G.toElementArray(col) for col in v], comb)) == msgs
    got["verifier"].combine(correct, y, comb)
    got["verifier"].batchCombined()
    assert got["verifier"].verifyCombined(I["chal"]) and not got["verifier"].verifyCombined(I["chal"] + 1)


# ---- arguments and memory ------------------------------------------------------------------------------------------------
def test_bad_arguments_and_live_bytes(ecgroup, vmn, gpu_ctx):
    import ctypes as C
    c, pts, multiples = case("P-256")
    G = ecgroup("P-256")
    A, B = G.toElementArray(pts), G.toElementArray(pts[::-1])
    short = G.toElementArray(pts[:23])
    foreign = vmn.ECqPGroup(gpu_ctx, "P-256").toElementArray(pts)
    es = [c.n - 2, (c.n + 1) // 2, 1 << 200]
    for r in vmn.PGroupElementArray.expMultiEach([A, B], es[:2]) + vmn.PGroupElementArray.expMulti([A, B], es[0]):
        r.free()                                                        # (warm: scratch and pool blocks of these sizes exist)
    live0 = gpu_ctx.memory_stats()["live_bytes"]
    res = vmn.PGroupElementArray.expMultiEach([A, B, A], es) + vmn.PGroupElementArray.expMulti([A, B, A], es[0]) + [A.exp(es[1])]
    assert gpu_ctx.memory_stats()["live_bytes"] > live0
    for r in res:
        r.free()
    assert gpu_ctx.memory_stats()["live_bytes"] == live0
    for arrays in ([A, short], [A, B, foreign]):
        for call in (lambda: vmn.PGroupElementArray.expMultiEach(arrays, es[:len(arrays)]), lambda: vmn.PGroupElementArray.expMulti(arrays, es[0])):
            with pytest.raises(vmn.VmnError) as ei:
                call()
            assert ei.value.status == -1                                # VMN_ERR_ARG
            assert gpu_ctx.memory_stats()["live_bytes"] == live0
    outs = (C.c_void_p * 2)()
    hs = (C.c_void_p * 2)(A._h, B._h)
    assert vmn.lib().vmn_garray_exp_scalars_multi(hs, C.c_size_t(0), b"\x05", C.c_size_t(1), outs) == -1      # k = 0
    assert vmn.lib().vmn_garray_exp_scalar_multi(hs, C.c_size_t(0), b"\x05", C.c_size_t(1), outs) == -1
    assert gpu_ctx.memory_stats()["live_bytes"] == live0
    for r in (A, B, short, foreign):                                    # (the caught errors' tracebacks hold this frame in a cycle)
        r.free()
