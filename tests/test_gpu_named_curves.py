"""GPU suite: ECqPGroup over the reference's other named curves (demo/mixnet/.conf:151-176) -- the general-a kernels
(ec_kernels.h EC_GENERAL: dbl-2007-bl, the prime taken at run time) at each of their limb counts (9, 10, 13, 15, 21),
secp224k1 (p = 1 mod 4: Tonelli-Shanks; an order one bit wider than p: exponents sized by bits(n)), secp256k1 (a = 0),
prime239v1 (a = -3 on a 10-limb prime other than P-256's) and P-192 (the NIST kernels of P-224 with 24-byte coordinates),
against the oracle's affine curve over the same constants (tests/named_curves.py ref_curve) and libcrypto's golden points.
Small arrays: the affine Python reference costs bits^3."""
import json
import os
import random

import pytest

from named_curves import ROOT, ref_curve

pytestmark = pytest.mark.gpu

CURVES = ["brainpoolp192r1", "secp224k1", "P-192", "prime239v1", "brainpoolp256r1", "secp256k1", "brainpoolp320r1",
          "brainpoolp384r1", "brainpoolp512r1"]


@pytest.fixture(scope="module", params=CURVES)
def ecg(request, vmn, gpu_ctx):
    return vmn.ECqPGroup(gpu_ctx, request.param), ref_curve(request.param)


@pytest.fixture(params=["normalised", "as they are"])
def first_level_rows(request, monkeypatch):
    """The two first levels of a multi-exponentiation over a curve (vmnhip.hip VMN_EC_NORMALISE_MIN): normalised rows with
    the mixed additions, or the rows as they are with full additions (small calls)."""
    monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "0" if request.param == "normalised" else "1000000000")
    return request.param


def sz(c, n):
    return n if c.p.bit_length() <= 256 else max(8, n // 2)


def pts(c, seed, n):
    rnd = random.Random(seed)
    return [c.mul(rnd.randrange(1, c.n), c.g) for _ in range(n)]


@pytest.mark.parametrize("name", ["brainpoolP256r1", "secp256r1", "prime256v1", "secp192r1", "prime192v1", "secp224r1",
                                  "secp384r1", "secp521r1"])
def test_aliases_are_the_same_group(name, vmn, gpu_ctx):
    from named_curves import ecscalar
    es = ecscalar()
    G = vmn.ECqPGroup(gpu_ctx, name)
    c = es.curve(name)
    assert (G.p, G.q, G.a, G.g) == (c["p"], c["n"], es.curve_a(c), (c["gx"], c["gy"]))
    X = G.exp(G.g, G.ringArray([1, 2, 3]))
    assert X.toInts() == [es.mul(k, G.g, G.p, G.q, G.a) for k in (1, 2, 3)]


def test_import_export_and_curve_check(ecg):
    G, c = ecg
    assert G.exp_bytes == (c.n.bit_length() + 7) // 8 and G.nbytes == c.nbytes
    xs = pts(c, 1, 24) + [None, c.g, c.neg(c.g)]
    X = G.toElementArray(xs)
    assert X.toInts() == xs and X.size() == 27
    bad = (c.g[0], (c.g[1] + 1) % c.p)                     # not on the curve
    arr = G.toElementArray([c.g, bad, (c.p, 5)], checked=False)
    assert arr.all_in_range is False
    assert arr.toInts() == [c.g, None, None]
    with pytest.raises(ValueError):
        G.toElementArray([bad])
    if c.a != c.p - 3:
        # a point of y^2 = x^3 - 3x + b (the NIST check's curve) is refused by the check with the curve's own a
        from oracle.pyref_prg import sqrt_mod
        x = 5
        while pow((x ** 3 - 3 * x + c.b) % c.p, (c.p - 1) // 2, c.p) != 1 or c.on_curve((x, sqrt_mod((x ** 3 - 3 * x + c.b) % c.p, c.p))):
            x += 1
        other = (x, sqrt_mod((x ** 3 - 3 * x + c.b) % c.p, c.p))
        assert G.toElementArray([other, c.g], checked=False).toInts() == [None, c.g]


def test_pointwise_group_operation_with_exceptional_cases(ecg):
    G, c = ecg
    a = pts(c, 2, 16) + [c.g, c.g, None, c.g, None]
    b = pts(c, 3, 16) + [c.g, c.neg(c.g), c.g, None, None]
    A, B = G.toElementArray(a), G.toElementArray(b)
    assert A.mul(B).toInts() == c.mul_arrays(a, b)           # equal points double through the addition
    assert A.inv().toInts() == [c.neg(P) for P in a]
    assert A.mul(A.inv()).toInts() == [None] * len(a)
    assert A.prod() == c.prod(a)
    # Jacobian rows (Z != 1) and negated rows meeting their equals and opposites
    J = A.exp(3)
    assert J.mul(J).toInts() == [c.mul(6, P) for P in a]
    assert J.mul(J.inv()).toInts() == [None] * len(a)


def test_scalar_multiplication_variable_fixed_and_shared(ecg):
    G, c = ecg
    rnd = random.Random(4)
    n = sz(c, 40)
    xs = pts(c, 5, n)
    es = [rnd.randrange(c.n) for _ in range(n)]
    es[0], es[1], es[2], es[3] = 0, 1, c.n - 1, 2
    X, E = G.toElementArray(xs), G.ringArray(es)
    assert X.exp(E).toInts() == c.exp_array(xs, es)
    assert G.exp(c.g, E).toInts() == c.exp_fixed(c.g, es)
    k = rnd.randrange(1 << 50)
    assert X.exp(k).toInts() == [c.mul(k, P) for P in xs]
    assert X.exp(0).toInts() == [None] * n
    e612 = [rnd.randrange(1 << 612) for _ in range(n)]
    assert X.expInts(e612, 612).toInts() == c.exp_array(xs, e612)


def test_two_scalar_multiplications_on_one_chain_of_doublings(ecg):
    G, c = ecg
    rnd = random.Random(44)
    n = sz(c, 30)
    xs, ys = pts(c, 45, n), pts(c, 46, n)
    xs[3], ys[4] = None, None
    ys[5] = c.neg(xs[5])
    qbits = c.n.bit_length()
    X, Y = G.toElementArray(xs), G.toElementArray(ys)
    for e, fbits in ((rnd.randrange(1 << 256), qbits), (0, qbits), (c.n + 5, 40), (c.n - 1, qbits)):
        fs = [rnd.randrange(1 << fbits) % c.n for _ in range(n)]
        fs[0], fs[1] = 0, c.n - 1 if fbits == qbits else (1 << fbits) - 1
        fs[5] = e % c.n if (e % c.n).bit_length() <= fbits else fs[5]
        want = [c.add(c.mul(e % c.n, x), c.mul(f, y)) for x, y, f in zip(xs, ys, fs)]
        assert X.exp2(e, Y, G.ringArray(fs), fbits).toInts() == want, (e.bit_length(), fbits)


def test_multi_exponentiation(ecg, first_level_rows):
    G, c = ecg
    rnd = random.Random(8)
    for n in (1, 2, 33):
        xs = pts(c, 100 + n, n)
        es = [rnd.randrange(c.n) for _ in range(n)]
        assert G.toElementArray(xs).expProd(G.ringArray(es)) == c.exp_prod(xs, es), n
    assert G.toElementArray([c.g] * 40).expProd(G.ringArray([12345] * 40)) == c.mul(40 * 12345, c.g)
    base = pts(c, 900, 8)
    xs = base + [c.neg(p) for p in base] + [None, None, c.g, c.g, c.neg(c.g)]
    es = [777] * 16 + [5, 777, 777, 777, 777]
    assert G.toElementArray(xs).expProd(G.ringArray(es)) == c.exp_prod(xs, es)
    J = G.toElementArray(base).exp(G.ringArray([3 + k for k in range(8)])).mul(G.toElementArray(base))      # Jacobian rows
    js = [c.mul(4 + k, p) for k, p in enumerate(base)]
    es = [rnd.randrange(c.n) for _ in range(8)]
    assert J.expProd(G.ringArray(es)) == c.exp_prod(js, es)


def test_independent_generators(ecg):
    from oracle import pyref_prg
    G, c = ecg
    seed = pyref_prg.random_oracle(b"named-curve-generators", 256, "sha256")
    for n, rbitlen in ((1, 100), (40, 50)):
        want = pyref_prg.ec_generators(seed, n, c, rbitlen, "sha256")
        assert G.elementArrayFromPRG(seed, n, rbitlen).toInts() == want, (n, rbitlen)
        assert all(c.on_curve(P) for P in want)


def test_golden_points_of_libcrypto(ecg):
    """tests/golden/ec_named.json (tests/golden/gen_golden_named_curves.py, libcrypto's EC_POINT_mul): k G as a fixed-base
    and as a variable-base power."""
    G, c = ecg
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "ec_named.json")))[c.name]
    assert (int(rec["p"], 16), int(rec["a"], 16), int(rec["b"], 16), int(rec["n"], 16)) == (c.p, c.a % c.p, c.b, c.n)
    ks = [int(k["k"], 16) for k in rec["cases"]]
    want = [tuple(int(v, 16) for v in k["kG"]) for k in rec["cases"]]
    assert G.exp(c.g, G.ringArray(ks)).toInts() == want
    assert G.toElementArray([c.g] * len(ks)).exp(G.ringArray(ks)).toInts() == want


@pytest.mark.parametrize("curve_name", ["brainpoolp256r1", "secp256k1"])
def test_proof_of_shuffle_and_ccpos_match_the_oracle(curve_name, vmn, gpu_ctx, entry, first_level_rows):
    """PoS and CCPoS over a general-a curve: the C++ provers' messages equal the group-generic Python restatement on the same
    tape (the O(1) points of the proof on the host: hostcurve.h with `a`); verifiers accept; a tampered reply is rejected."""
    from oracle import pyref_proofs as P
    from tape import Tape
    import mirror
    mods = mirror.load(entry, ("mixnet", "native"))
    hv, mx = mods["native"], mods["mixnet"]
    c = ref_curve(curve_name)
    K = P.ECAdapter(c)
    G = vmn.ECqPGroup(gpu_ctx, curve_name)
    NV, NE, NR = 128, 128, 64
    n = 24
    t = Tape(b"ecnamed", c.n)
    g = c.g
    h = [c.mul(x, g) for x in t.ring_array(n)]
    y = c.mul(t.ring_element(), g)
    pkey = [g, y]
    er = t.ring_array(n)
    w = [c.exp_fixed(g, er), c.mul_arrays([c.mul(m, g) for m in t.ring_array(n)], c.exp_fixed(y, er))]
    pi = t.permutation(n)
    s = [t.ring_array(n)]
    e = t.int_array(n, NE)
    v = t.int_array(1, NV)[0]
    ints = lambda x: x.toInts() if hasattr(x, "toInts") else x

    def same(a, b):
        assert set(a) == set(b)
        for k in a:
            assert ints(a[k]) == ints(b[k]), k

    o = P.GPoS(K, NV, NE, NR, rand=Tape(b"prover", c.n))
    o.precompute(g, h, pi)
    wp_o = P.g_reencrypt(K, w, P.g_reenc_factors(K, pkey, s), pi)
    o.setInstance(pkey, w, wp_o, s)
    o.setBatchVector(e)
    com_o, rep_o = o.commit(), o.reply(v)
    H = G.toElementArray(h)
    W = [G.toElementArray(col) for col in w]
    S = [G.ringArray(s[0])]
    pr = hv.PoSBasicTW(G, NV, NE, NR, rand=Tape(b"prover", c.n))
    pr.precompute(g, H, pi)
    assert pr.u.toInts() == o.u
    WP = hv.reencrypt_native(G, pkey, W, S, pi)
    assert [col.toInts() for col in WP] == wp_o
    pr.setInstance(pkey, W, WP, S)
    pr.setBatchVector(e)
    com, rep = pr.commit(), pr.reply(v)
    same(com, com_o)
    same(rep, rep_o)
    ver = hv.PoSBasicTW(G, NV, NE, NR)
    ver.precompute(g, H)
    ver.setPermutationCommitment(pr.u)
    ver.setInstance(pkey, W, WP)
    ver.setBatchVector(e)
    ver.computeAF()
    ver.setCommitment(com)
    ver.setChallenge(v)
    assert ver.verify(rep)
    bad = dict(rep)
    bad["k_F"] = [(x + 1) % c.n for x in rep["k_F"]]
    assert not ver.verify(bad) and ver.verdicts == (True, True, True, True, False)
    r = t.ring_array(n)
    u_o = P.g_permutation_commitment(K, g, h, r, pi)
    pc = mx.PermutationCommitment(G, H)
    U = pc.precompute(r, pi)
    assert U.toInts() == u_o
    oc = P.GCCPoS(K, NV, NE, NR, rand=Tape(b"cc", c.n))
    oc.setInstance(g, h, u_o, pkey, w, wp_o, r, pi, s)
    oc.setBatchVector(e)
    cc_o, cr_o = oc.commit(), oc.reply(v)
    cp = hv.CCPoSBasicW(G, NV, NE, NR, rand=Tape(b"cc", c.n))
    cp.setInstance(g, H, U, pkey, W, WP, pc.exponents, pi, S)
    cp.setBatchVector(e)
    cc, cr = cp.commit(), cp.reply(v)
    same(cc, cc_o)
    same(cr, cr_o)
    cv = hv.CCPoSBasicW(G, NV, NE, NR)
    cv.setInstance(g, H, U, pkey, W, WP)
    cv.setBatchVector(e)
    cv.setCommitment(cc)
    cv.setChallenge(v)
    cv.computeAB()
    assert cv.verify(cr)
    bad = dict(cr)
    bad["k_A"] = (cr["k_A"] + 1) % c.n
    assert not cv.verify(bad)


def test_properties_at_1e5_points_brainpoolp256r1(vmn, gpu_ctx):
    """10^5 points of brainpoolp256r1 through the large-array paths (normalised first level, fixed-base tables), pinned by
    algebraic relations plus a few spot checks against the reference."""
    import numpy as np
    c = ref_curve("brainpoolp256r1")
    G = vmn.ECqPGroup(gpu_ctx, "brainpoolp256r1")
    n = 100_000
    rng = np.random.Generator(np.random.PCG64(2025))

    def block(clear_top_bits):
        a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        a[:, 0] &= 0xFF >> clear_top_bits
        return a
    eb, fb = block(2), block(2)                        # exponents < 2^254 < n / 2: e + f < n, no wrap
    E, F = G.ringArray(eb.tobytes()), G.ringArray(fb.tobytes())
    X = G.exp(c.g, G.ringArray(block(2).tobytes()))
    XE, XF = X.exp(E), X.exp(F)
    assert XE.mul(XF).equals(X.exp(E.add(F)))          # e P + f P = (e + f) P
    Gs = G.toElementArray(G.enc_el(c.g) * n)
    assert G.exp(c.g, E).equals(Gs.exp(E))             # fixed-base table path = variable-base path
    assert X.expProd(E) == XE.prod()                   # Pippenger = sum of the individual multiples
    assert X.mul(X.inv()).equals(G.toElementArray(G.enc_el(None) * n))
    for i in (0, 77_777, 99_999):
        e = int.from_bytes(eb[i].tobytes(), "big")
        assert XE.get(i) == c.mul(e, X.get(i))
