"""GPU suite, K11: the elliptic-curve group kernels (one point per lane, Jacobian rows) against the Python
curve reference — every array operation the proofs use, with the exceptional cases of the addition."""
import random

import pytest

from oracle.pyref_ec import Curve

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["P-224", "P-256", "P-384", "P-521"])
def ecg(request, vmn, gpu_ctx):
    return vmn.ECqPGroup(gpu_ctx, request.param), Curve(request.param)


@pytest.fixture(params=["normalised", "as they are"])
def first_level_rows(request, monkeypatch):
    """A multi-exponentiation over a curve normalises its input rows (Z := 1) and adds them with the mixed formulas -- or, for
    small calls, adds the rows as they are with full additions (vmnhip.hip: VMN_EC_NORMALISE_MIN points, default 131072).
    The cases below are small: without this fixture only the second path would ever meet them."""
    monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "0" if request.param == "normalised" else "1000000000")
    return request.param


def sz(c, n):
    """The affine Python reference costs bits^3: the 521-bit curve runs the same cases on a third of the points."""
    return n if c.p.bit_length() <= 384 else max(8, n // 3)


def pts(c, seed, n):
    rnd = random.Random(seed)
    return [c.mul(rnd.randrange(1, c.n), c.g) for _ in range(n)]


def test_import_export_and_curve_check(ecg, vmn):
    G, c = ecg
    xs = pts(c, 1, 70) + [None, c.g, c.neg(c.g)]
    X = G.toElementArray(xs)
    assert X.toInts() == xs and X.size() == 73
    bad = (c.g[0], (c.g[1] + 1) % c.p)                     # not on the curve
    arr = G.toElementArray([c.g, bad, (c.p, 5)], checked=False)
    assert arr.all_in_range is False
    assert arr.toInts() == [c.g, None, None]               # offending entries replaced by the identity
    with pytest.raises(ValueError):
        G.toElementArray([bad])


def test_export_of_a_large_array_normalises_its_rows_first(ecg, monkeypatch):
    """The export kernel inverts Z with one Fermat power per point; from VMN_EC_EXPORT_NORMALISE_MIN points on (default 262144)
    the rows go through the batched inversion of the multi-exponentiations first and are exported as they are.  Same bytes."""
    G, c = ecg
    base = pts(c, 31, sz(c, 60))
    X = G.toElementArray(base + [None, c.g])
    J = X.exp(7).mul(X)                                    # Jacobian rows with Z != 1: 8 P; the identity stays the identity
    want = [c.mul(8, p) for p in base] + [None, c.mul(8, c.g)]
    assert J.toInts() == want
    monkeypatch.setenv("VMN_EC_EXPORT_NORMALISE_MIN", "1")
    assert J.toInts() == want
    assert X.toInts() == base + [None, c.g]                # rows that already have Z = 1


def test_pointwise_group_operation_with_exceptional_cases(ecg):
    G, c = ecg
    a = pts(c, 2, 40)
    b = pts(c, 3, 40)
    # equal points (doubling through the addition), opposite points, identity on either side
    a += [c.g, c.g, None, c.g, None]
    b += [c.g, c.neg(c.g), c.g, None, None]
    A, B = G.toElementArray(a), G.toElementArray(b)
    assert A.mul(B).toInts() == c.mul_arrays(a, b)
    assert A.inv().toInts() == [c.neg(P) for P in a]
    assert A.mul(A.inv()).toInts() == [None] * len(a)
    assert A.prod() == c.prod(a)
    assert G.toElementArray([]).prod() is None


def test_scalar_multiplication_variable_fixed_and_shared(ecg):
    G, c = ecg
    rnd = random.Random(4)
    n = sz(c, 150)
    xs = pts(c, 5, n)
    es = [rnd.randrange(c.n) for _ in range(n)]
    es[0], es[1], es[2], es[3] = 0, 1, c.n - 1, 2
    X, E = G.toElementArray(xs), G.ringArray(es)
    assert X.exp(E).toInts() == c.exp_array(xs, es)
    assert G.exp(c.g, E).toInts() == c.exp_fixed(c.g, es)
    k = rnd.randrange(1 << 50)
    assert X.exp(k).toInts() == [c.mul(k, P) for P in xs]
    assert X.exp(0).toInts() == [None] * n
    e612 = [rnd.randrange(1 << 612) for _ in range(n)]    # long integer exponents act through their residue mod n
    assert X.expInts(e612, 612).toInts() == c.exp_array(xs, e612)


def test_two_scalar_multiplications_on_one_chain_of_doublings(ecg):
    """vmn_garray_exp2 over a curve (k_ec_mulvar2, round 4): e * x[i] + f[i] * y[i] with a shared scalar e and per-point
    scalars f -- the form a verifier's check (B) takes for large arrays (B_i^v (B_{i-1}^-1)^{k_E,i}).  Edge cases: zero
    scalars on either side (the identity's table entry), e larger than the group order (acts through its residue), scalars
    of unequal length, y = -x with f = e (everything cancels), points at infinity as bases."""
    G, c = ecg
    rnd = random.Random(44)
    n = sz(c, 120)
    xs, ys = pts(c, 45, n), pts(c, 46, n)
    xs[3], ys[4] = None, None
    ys[5] = c.neg(xs[5])
    qbits = c.n.bit_length()
    X, Y = G.toElementArray(xs), G.toElementArray(ys)
    for e, fbits in ((rnd.randrange(1 << 256), qbits), (0, qbits), (1, 1), (c.n + 5, 40), (c.n - 1, qbits), (rnd.randrange(1 << 128), 64)):
        fs = [rnd.randrange(1 << fbits) % c.n for _ in range(n)]
        fs[0], fs[1] = 0, (1 << fbits) - 1 if fbits < qbits else c.n - 1
        fs[5] = e % c.n if (e % c.n).bit_length() <= fbits else fs[5]
        want = [c.add(c.mul(e % c.n, x), c.mul(f, y)) for x, y, f in zip(xs, ys, fs)]
        assert X.exp2(e, Y, G.ringArray(fs), fbits).toInts() == want, (e.bit_length(), fbits)


def test_check_b_in_its_combined_form_over_a_curve(vmn, gpu_ctx, entry, monkeypatch):
    """Large arrays over a curve verify check (B) as (B_i^v (B_{i-1}^-1)^{k_E,i}) B'_i = g^{k_B,i} through k_ec_mulvar2
    (VMN_COMBINED_MIN=1 forces that form at test size): transcript, verdicts and the verifier's intermediates as in the
    separate form; a reply tampered in ONE k_B fails check (B) only."""
    import mirror
    from oracle import pyref_proofs as P
    from proof_cases import check_pos, make_instance
    from tape import Tape
    monkeypatch.setenv("VMN_COMBINED_MIN", "1")
    mods = mirror.load(entry, ("native", "mixnet", "hvzk", "elgamal"))
    c = Curve("P-256")
    K = P.ECAdapter(c)
    G = vmn.ECqPGroup(gpu_ctx, "P-256")
    n, width = 70, 1
    h, pkey, w, t = make_instance(K, c.g, n, width, b"ec-combined")
    H, W, WP, wp_o, s, S, pi = check_pos("native", mods, G, K, c.g, h, pkey, w, t, (128, 128, 64))
    nat = mods["native"]
    e, v = t.int_array(n, 128), t.int_array(1, 128)[0]
    pr = nat.PoSBasicTW(G, 128, 128, 64, rand=Tape(b"ec-combined-prover", c.n))
    pr.precompute(c.g, H, pi)
    pr.setInstance(pkey, W, WP, S)
    pr.setBatchVector(e)
    com, rep = pr.commit(), pr.reply(v)
    ver = nat.PoSBasicTW(G, 128, 128, 64)
    ver.precompute(c.g, H)
    ver.setPermutationCommitment(pr.u)
    ver.setInstance(pkey, W, WP)
    ver.setBatchVector(e)
    ver.computeAF()
    ver.setCommitment(com)
    ver.setChallenge(v)
    assert ver.verify(rep) and ver.verdicts == (True,) * 5
    bad = dict(rep)
    kb = rep["k_B"].toInts()
    kb[n // 2] = (kb[n // 2] + 1) % c.n
    bad["k_B"] = G.ringArray(kb)
    assert not ver.verify(bad) and ver.verdicts == (True, False, True, True, True)


def test_equality_is_of_group_elements_not_of_representations(ecg):
    G, c = ecg
    rnd = random.Random(6)
    n = sz(c, 90)
    xs = pts(c, 7, n)
    a = [rnd.randrange(c.n) for _ in range(n)]
    b = [rnd.randrange(c.n) for _ in range(n)]
    X = G.toElementArray(xs)
    A, B = G.ringArray(a), G.ringArray(b)
    left = X.exp(A).exp(B)                                 # Jacobian rows with unrelated Z coordinates
    right = X.exp(A.mul(B))
    assert left.equals(right)
    ys = list(xs)
    ys[n - 1] = c.g
    assert not X.equals(G.toElementArray(ys))
    assert X.exp(A).mul(X.exp(B)).equals(X.exp(A.add(B)))


def test_multi_exponentiation_and_movement(ecg, first_level_rows):
    G, c = ecg
    rnd = random.Random(8)
    for n in (1, 2, 33, sz(c, 300)):
        xs = pts(c, 100 + n, n)
        es = [rnd.randrange(c.n) for _ in range(n)]
        e256 = [rnd.randrange(1 << 128) for _ in range(n)]
        X = G.toElementArray(xs)
        assert X.expProd(G.ringArray(es)) == c.exp_prod(xs, es), n
        assert X.expProd(e256, 128) == c.exp_prod(xs, e256), n
        perm = list(range(n))
        rnd.shuffle(perm)
        assert X.permute(perm).toInts() == [xs[j] for j in perm]
        assert X.shiftPush(c.g).toInts() == ([c.g] + xs[:-1])
        assert X.get(n - 1) == xs[n - 1]
    # all-equal bases and exponents: one bucket per window, equal-point additions inside the tree
    xs = [c.g] * 64
    es = [12345] * 64
    assert G.toElementArray(xs).expProd(G.ringArray(es)) == c.mul(64 * 12345, c.g)
    assert G.toElementArray([]).expProd(G.ringArray([])) is None
    # the first bucket level adds NORMALISED rows with the mixed addition: opposite points and the identity inside one
    # bucket, inputs that arrive with Z != 1 (results of earlier operations), an all-identity array
    base = pts(c, 900, 12)
    xs = base + [c.neg(p) for p in base] + [None, None, c.g, c.g, c.neg(c.g)]
    es = [777] * 24 + [5, 777, 777, 777, 777]
    assert G.toElementArray(xs).expProd(G.ringArray(es)) == c.exp_prod(xs, es)
    J = G.toElementArray(base).exp(G.ringArray([3 + k for k in range(12)])).mul(G.toElementArray(base))      # Jacobian rows
    js = [c.mul(4 + k, p) for k, p in enumerate(base)]
    assert J.toInts() == js
    es = [rnd.randrange(c.n) for _ in range(12)]
    assert J.expProd(G.ringArray(es)) == c.exp_prod(js, es)
    assert G.toElementArray([None] * 9).expProd(G.ringArray(list(range(9)))) is None
    # fixed-base table (normalised entries, identity rows for zero digits): exponents with zero windows
    es = [0, 1, 1 << 16, (1 << 200) + 1, c.n - 1, 1 << 255 if (1 << 255) < c.n else 1 << 200]
    assert G.exp(base[0], G.ringArray(es)).toInts() == [c.mul(e, base[0]) for e in es]


def test_signed_window_recoding_of_the_multi_exponentiation(ecg, first_level_rows):
    """Curves sort the exponents by SIGNED window digits (light_kernels.h signed_digit): exponents whose digits sit on the
    recoding's edges for every window width the library may pick -- every digit exactly 2^(c-1) (a carry arrives or not), one
    above and one below, all ones (a carry through every window), the top bits of the order -- against the oracle.
    The width that RUNS is picked from the size of the array, not from the exponents: the two arrays below are recoded at the
    two or three widths of their sizes (3 and 6 bits over P-256).  Every width 2 ... 17 at its own edges:
    test_gpu_schedules.py::test_multi_exponentiation_at_every_window_width_curves."""
    G, c = ecg
    rnd = random.Random(77)
    nbits = c.n.bit_length()
    es = [0, 1, 2, c.n - 1, c.n - 2, (1 << (nbits - 1)) - 1, 1 << (nbits - 1)]
    for w in range(2, 18):
        half = sum((1 << (w - 1)) << (w * k) for k in range(nbits // w + 1))
        ones = (1 << (w * (nbits // w))) - 1
        for e in (half, half + 1, half - 1, half << 1, ones, ones - (1 << (w - 1)), half ^ (1 << (w * 3 + w - 1))):
            es.append(e % c.n)
    xs = pts(c, 4242, len(es))
    want = c.exp_prod(xs, es)
    X, E = G.toElementArray(xs), G.ringArray(es)
    assert X.expProd(E) == want
    # many more elements than buckets, so that the library picks a wide window; the edge exponents among random ones
    n = 3000
    more = es + [rnd.randrange(c.n) for _ in range(n - len(es))]
    base = pts(c, 4243, 16)
    ys = [base[i % 16] for i in range(n)]
    coeff = [0] * 16
    for i, e in enumerate(more):
        coeff[i % 16] = (coeff[i % 16] + e) % c.n
    assert G.toElementArray(ys).expProd(G.ringArray(more)) == c.exp_prod(base, coeff)


def test_scalar_field_arrays(ecg):
    G, c = ecg
    rnd = random.Random(9)
    n = 77
    a = [rnd.randrange(c.n) for _ in range(n)]
    b = [rnd.randrange(c.n) for _ in range(n)]
    A, B = G.ringArray(a), G.ringArray(b)
    assert A.mul(B).toInts() == [x * y % c.n for x, y in zip(a, b)]
    assert A.innerProduct(B) == sum(x * y for x, y in zip(a, b)) % c.n
    x, d = A.recLin(B)
    want, acc = [], 0
    for i in range(n):
        acc = a[i] % c.n if i == 0 else (acc * b[i] + a[i]) % c.n
        want.append(acc)
    assert x.toInts() == want and d == want[-1]


@pytest.mark.parametrize("impl,curve_name", [("native", "P-256"), ("native", "P-384"), ("native", "P-224"), ("native", "P-521")])
def test_proof_of_shuffle_and_ccpos_over_p256_match_the_oracle(impl, curve_name, vmn, gpu_ctx, entry, first_level_rows):
    """PoS and CCPoS with ECqPGroup P-256 (the reference's default group): the GPU provers' messages equal the
    group-generic Python restatement on the same tape; verifiers accept; a tampered reply is rejected."""
    import importlib.util, os, sys
    from oracle import pyref_proofs as P
    from tape import Tape
    import mirror
    mods = mirror.load(entry, ("hvzk", "mixnet", "native"))
    hv, mx = mods["hvzk" if impl == "python" else "native"], mods["mixnet"]      # Python mirror or the C++ drivers
    c = Curve(curve_name)
    K = P.ECAdapter(c)
    G = vmn.ECqPGroup(gpu_ctx, curve_name)
    NV, NE, NR = 128, 128, 64
    n, width = sz(c, 40), 1
    t = Tape(b"ecgpu", c.n)
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

    # ---- PoS
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
    assert pr.u.toInts() == o.u and getattr(pr, "Ap", o.Ap) == o.Ap
    WP = mx.reencrypt(W, mx.reencFactors(G, pkey, S), pi) if impl == "python" else hv.reencrypt_native(G, pkey, W, S, pi)
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
    # ---- CCPoS on a permutation commitment
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


@pytest.mark.parametrize("impl", ["native"])
def test_threshold_decryption_over_p256(impl, vmn, gpu_ctx, entry):
    """Row A6 over the curve group: factors, Lagrange combination (negative integers = point negation), plaintext
    recovery and the batched proofs."""
    import importlib.util, os, sys
    from tape import Tape
    import mirror
    modname = "elgamal" if impl == "python" else "native"
    eg = mirror.load(entry, (modname,))[modname]
    c = Curve("P-256")
    G = vmn.ECqPGroup(gpu_ctx, "P-256")
    kw = {} if impl == "python" else {"group": G}          # the C++ helpers take the group instead of a bare q
    q, g = c.n, c.g
    n, k, thr = 50, 5, 3
    t = Tape(b"ecdec", q)
    coeffs = t.ring_array(thr)
    share = lambda j: sum(cf * pow(j, d, q) for d, cf in enumerate(coeffs)) % q
    xs = [None] + [share(j) for j in range(1, k + 1)]
    ys = [None] + [c.mul(xj, g) for xj in xs[1:]]
    y = c.mul(coeffs[0], g)
    msgs = [c.mul(m, g) for m in t.ring_array(n)]
    rs = t.ring_array(n)
    u = c.exp_fixed(g, rs)
    v = c.mul_arrays(msgs, c.exp_fixed(y, rs))
    correct = [False, True, False, True, True, True]
    U, V = G.toElementArray(u), G.toElementArray(v)
    F = [None] + [eg.decryptionFactors(U, xs[j], q, k) for j in range(1, k + 1)]
    inv_c = pow(eg.prodFactor(q, k, **kw), -1, q)
    for j in range(1, k + 1):
        assert F[j].toInts() == [c.mul((-xs[j]) * inv_c % q, P) for P in u]
    assert any(ci < 0 for ci in eg.modifiedLagrangeCoefficients(q, correct, k, thr, **kw))
    comb = eg.combineDecryptionFactors(F, correct, k, thr, q)
    assert eg.plaintexts(V, comb).toInts() == msgs
    e = t.int_array(n, 100)
    chal = t.int_array(1, 100)[0]
    ver = eg.DistrElGamalSessionBasic(G, 1, k, thr, 100)
    ver.setInstance(U, ys, F)
    ver.setBatchVector(e)
    ver.batchInput()
    for j in range(1, k + 1):
        pr = eg.DistrElGamalSessionBasic(G, j, k, thr, 100, rand=Tape(b"p%d" % j, q))
        pr.setInstance(U, ys, F)
        pr.setBatchVector(e)
        pr.batchInput()
        ver.setCommitment(j, *pr.commit(xs[j]))
        ver.setReply(j, pr.reply(chal))
    for j in range(1, k + 1):
        ver.batch(j)
        assert ver.verify(j, chal)
    ver.combine(correct, y, comb)
    ver.batchCombined()
    assert ver.verifyCombined(chal)
    ver.setReply(3, (ver.k_x[3] + 1) % q)
    assert not ver.verify(3, chal)


def test_properties_at_full_baseline_size_p256(vmn, gpu_ctx):
    """BASELINE.json configs[4] size (10^6 points of P-256): the affine Python reference would need hours, so the
    result is pinned through size-independent properties plus spot checks against the reference."""
    import numpy as np
    c = Curve("P-256")
    G = vmn.ECqPGroup(gpu_ctx, "P-256")
    n = 1_000_000
    rng = np.random.Generator(np.random.PCG64(2024))

    def block(clear_top_bits):
        a = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        a[:, 0] &= 0xFF >> clear_top_bits
        return a
    eb, fb = block(2), block(2)                        # exponents < 2^254: e + f < n, no wrap
    E, F = G.ringArray(eb.tobytes()), G.ringArray(fb.tobytes())
    X = G.exp(c.g, G.ringArray(block(1).tobytes()))    # random points (fixed-base path)
    XE, XF = X.exp(E), X.exp(F)
    assert XE.mul(XF).equals(X.exp(E.add(F)))          # e P + f P = (e + f) P, point-wise over 10^6 points
    Gs = G.toElementArray(G.enc_el(c.g) * n)
    assert G.exp(c.g, E).equals(Gs.exp(E))             # fixed-base table path = variable-base path
    assert X.expProd(E) == XE.prod()                   # Pippenger = sum of the individual multiples
    assert X.mul(X.inv()).equals(G.toElementArray(G.enc_el(None) * n))       # P + (-P) = infinity everywhere
    for i in (0, 1, 499_999, 999_999):
        e = int.from_bytes(eb[i].tobytes(), "big")
        assert XE.get(i) == c.mul(e, X.get(i))
