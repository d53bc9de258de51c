"""GPU suite, row A6 at width omega: the C++ decryption drivers (vmn_decryption_factors_wide, vmn_combine_decryption_factors_wide,
vmn_decproof_* after vmn_decproof_set_instance_wide) through verificatum_vmn_amd.native against the restatement of
DistrElGamalSessionBasic over G^omega (tests/wide_decrypt_ref.py).  Both sides draw from the same tape, so factors, combined
factors, commitments (y', B'), replies, verdicts and plaintexts compare exactly.

Wall time on an MI355X: not measured yet, for this module and for the existing GPU modules beside it."""
import pytest

from conftest import load_golden
from oracle.pyref_ec import Curve
from tape import Tape

import wide_decrypt_ref as W

pytestmark = pytest.mark.gpu

NE, NV = 100, 100
CASES = [("modp", 512, 40, 3, 2, 2, ()), ("modp", 2048, 130, 5, 3, 3, (2,)), ("P-256", 256, 24, 3, 2, 3, ())]


@pytest.fixture(scope="module")
def nat(entry):
    import mirror
    return mirror.load(entry, ("native",))["native"]


def make_instance(kind, bits, n, k, thr, width, vmn, gpu_ctx):
    """Group, adapter, Shamir shares of the key, a width-omega list of ciphertexts and their plaintexts."""
    if kind == "modp":
        grp, _ = load_golden(bits)
        p, q, g = grp["p"], grp["q"], grp["g"]
        G, K = vmn.ModPGroup(gpu_ctx, p, q, g), W.adapter_modp(p, q)
        bad_element = p - 1                                         # in range, no quadratic residue (p = 2q + 1 = 3 mod 4)
    else:
        c = Curve(kind)
        q, g = c.n, c.g
        G, K = vmn.ECqPGroup(gpu_ctx, kind), W.adapter_curve(c)
        bad_element = (c.g[0], (c.g[1] + 1) % c.p)                  # not on the curve
    t = Tape(b"wide-dec/%s%d" % (kind.encode(), bits), q)
    coeffs = t.ring_array(thr)
    share = lambda j: sum(cf * pow(j, d, q) for d, cf in enumerate(coeffs)) % q
    xs = [None] + [share(j) for j in range(1, k + 1)]
    ys = [None] + [K.exp(g, xj) for xj in xs[1:]]
    y = K.exp(g, coeffs[0])
    msgs = [K.exp_fixed(g, t.ring_array(n)) for _ in range(width)]
    rs = [t.ring_array(n) for _ in range(width)]
    u = [K.exp_fixed(g, r) for r in rs]
    v = [K.mul_arrays(m, K.exp_fixed(y, r)) for m, r in zip(msgs, rs)]
    return dict(G=G, K=K, q=q, g=g, xs=xs, ys=ys, y=y, msgs=msgs, u=u, v=v, e=t.int_array(n, NE), chal=t.int_array(1, NV)[0],
                bad_element=bad_element)


def ints_of(arrays):
    return [a.toInts() for a in arrays]


def gpu_session(nat, I, U, F, k, thr, seed):
    """Every party's prover and one verifier (party 1) on the GPU: {"commit", "reply", "verifier"} as W.run_session."""
    G = I["G"]
    ver = nat.DistrElGamalSessionBasic(G, 1, k, thr, NE)
    ver.setInstance(U, I["ys"], F)
    ver.setBatchVector(I["e"])
    ver.batchInput()
    out = {"commit": {}, "reply": {}, "verifier": ver}
    for j in range(1, k + 1):
        pr = nat.DistrElGamalSessionBasic(G, j, k, thr, NE, rand=Tape(seed + b"%d" % j, I["q"]))
        pr.setInstance(U, I["ys"], F)
        pr.setBatchVector(I["e"])
        pr.batchInput()
        out["commit"][j] = pr.commit(I["xs"][j])
        out["reply"][j] = pr.reply(I["chal"])
        ver.setCommitment(j, *out["commit"][j])
        ver.setReply(j, out["reply"][j])
        ver.batch(j)
    return out


@pytest.mark.parametrize("kind,bits,n,k,thr,width,bad", CASES)
def test_wide_threshold_decryption_equals_the_restatement(kind, bits, n, k, thr, width, bad, nat, vmn, gpu_ctx):
    I = make_instance(kind, bits, n, k, thr, width, vmn, gpu_ctx)
    G, K, q, g, chal = I["G"], I["K"], I["q"], I["g"], I["chal"]
    correct = [False] + [j not in bad for j in range(1, k + 1)]
    U = [G.toElementArray(c) for c in I["u"]]
    V = [G.toElementArray(c) for c in I["v"]]
    # every party's factors in every component
    f_o = [None] + [W.decryption_factors(K, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    F = [None] + [nat.decryptionFactors(U, I["xs"][j], q, k) for j in range(1, k + 1)]
    for j in range(1, k + 1):
        assert isinstance(F[j], list) and ints_of(F[j]) == f_o[j], j
    # the combined factors and the plaintexts
    comb_o = W.combine_decryption_factors(K, f_o, correct, k, thr)
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    assert ints_of(comb) == comb_o
    plain = nat.plaintexts(V, comb)
    assert ints_of(plain) == W.plaintexts(K, I["v"], comb_o) == I["msgs"]
    # (y', B') and the reply of every party: the same tape on both sides
    seed = b"wide-party/"
    ref = W.run_session(K, g, I["u"], I["ys"], I["xs"], f_o, I["e"], chal, k, thr, lambda j: Tape(seed + b"%d" % j, q))
    got = gpu_session(nat, I, U, F, k, thr, seed)
    ver, ver_o = got["verifier"], ref["verifier"]
    for j in range(1, k + 1):
        assert got["commit"][j] == ref["commit"][j] and len(got["commit"][j][1]) == width, j
        assert got["reply"][j] == ref["reply"][j], j
    # per-party and combined verdicts
    for j in range(1, k + 1):
        assert ver.verify(j, chal) == ver_o.verify(j, chal) == True, j
    ver.combine(correct, I["y"], comb)
    ver.batchCombined()
    ver_o.combine(correct, I["y"], comb_o)
    ver_o.batchCombined()
    assert ver.verifyCombined(chal) == ver_o.verifyCombined(chal) == True
    assert not ver.verifyCombined(chal + 1) and not ver_o.verifyCombined(chal + 1)
    # a reply >= q is no field element: verdict false, on both sides
    big = got["reply"][1] + q                                          # the same class mod q where the wire width holds it
    if big >= 1 << (8 * G.exp_bytes):
        big = q
    ver.setReply(1, big)
    ver_o.setReply(1, big)
    assert ver.verify(1, chal) == ver_o.verify(1, chal) == False
    ver.setReply(1, got["reply"][1])
    assert ver.verify(1, chal)
    # B' whose second row is no group element: the whole commitment is refused
    yp2, Bp2 = got["commit"][2]
    with pytest.raises(vmn.VmnError) as ei:
        ver.setCommitment(2, yp2, (Bp2[0], I["bad_element"]) + tuple(Bp2[2:]))
    assert ei.value.status == -4                                       # VMN_ERR_FORMAT
    assert ver.verify(2, chal)                                         # (the commitment set before stands)


def test_a_wrong_component_of_one_party_fails_that_party_only(nat, vmn, gpu_ctx):
    kind, bits, n, k, thr, width = "modp", 512, 40, 3, 2, 3
    I = make_instance(kind, bits, n, k, thr, width, vmn, gpu_ctx)
    G, K, q, g, chal = I["G"], I["K"], I["q"], I["g"], I["chal"]
    U = [G.toElementArray(c) for c in I["u"]]
    V = [G.toElementArray(c) for c in I["v"]]
    f_o = [None] + [W.decryption_factors(K, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    f_o[2][1] = list(f_o[2][1])
    f_o[2][1][17] = K.mul(f_o[2][1][17], g)                            # one element of ONE component of party 2
    F = [None] + [nat.decryptionFactors(U, I["xs"][j], q, k) for j in range(1, k + 1)]
    F[2] = [F[2][0], G.toElementArray(f_o[2][1]), F[2][2]]
    seed = b"wide-bad/"
    ref = W.run_session(K, g, I["u"], I["ys"], I["xs"], f_o, I["e"], chal, k, thr, lambda j: Tape(seed + b"%d" % j, q))
    got = gpu_session(nat, I, U, F, k, thr, seed)
    ver, ver_o = got["verifier"], ref["verifier"]
    verdicts = [ver.verify(j, chal) for j in range(1, k + 1)]
    assert verdicts == [ver_o.verify(j, chal) for j in range(1, k + 1)] == [True, False, True]
    correct = [False, True, False, True]
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    comb_o = W.combine_decryption_factors(K, f_o, correct, k, thr)
    assert ints_of(comb) == comb_o
    ver.combine(correct, I["y"], comb)
    ver.batchCombined()
    assert ver.verifyCombined(chal)
    assert ints_of(nat.plaintexts(V, comb)) == I["msgs"]
    # with party 2 counted as correct the combination is wrong and its proof fails
    wrong = nat.combineDecryptionFactors(F, [False, True, True, True], k, thr, q)
    ver.combine([False, True, True, True], I["y"], wrong)
    ver.batchCombined()
    assert not ver.verifyCombined(chal)


def test_width_one_through_the_wide_entry_points_is_the_width_one_path(nat, vmn, gpu_ctx):
    kind, bits, n, k, thr = "modp", 512, 40, 3, 2
    I = make_instance(kind, bits, n, k, thr, 1, vmn, gpu_ctx)
    G, q, chal = I["G"], I["q"], I["chal"]
    U = G.toElementArray(I["u"][0])
    correct = [False] + [True] * k
    F1 = [None] + [nat.decryptionFactors(U, I["xs"][j], q, k) for j in range(1, k + 1)]
    Fw = [None] + [nat.decryptionFactors([U], I["xs"][j], q, k) for j in range(1, k + 1)]
    for j in range(1, k + 1):
        assert Fw[j][0].toBytes() == F1[j].toBytes()
    c1 = nat.combineDecryptionFactors(F1, correct, k, thr, q)
    cw = nat.combineDecryptionFactors(Fw, correct, k, thr, q)
    assert cw[0].toBytes() == c1.toBytes()
    seed = b"wide-one/"
    I1 = dict(I)
    s1 = gpu_session(nat, I1, U, F1, k, thr, seed)
    sw = gpu_session(nat, I, [U], Fw, k, thr, seed)
    for j in range(1, k + 1):
        yp1, Bp1 = s1["commit"][j]
        ypw, Bpw = sw["commit"][j]
        assert ypw == yp1 and Bpw == (Bp1,) and sw["reply"][j] == s1["reply"][j]
        assert sw["verifier"].verify(j, chal) and s1["verifier"].verify(j, chal)
    s1["verifier"].combine(correct, I["y"], c1)
    sw["verifier"].combine(correct, I["y"], cw)
    for s in (s1, sw):
        s["verifier"].batchCombined()
        assert s["verifier"].verifyCombined(chal) and not s["verifier"].verifyCombined(chal ^ 1)


def test_witness_batch_input_sorts_the_digits_once_at_any_width(nat, vmn, gpu_ctx):
    """batch_input over three components is ONE multi-exponentiation: the expprod_sort family is launched as often as at width 1
    (the digits of e are sorted once), not three times as often."""
    I = make_instance("modp", 512, 300, 3, 2, 3, vmn, gpu_ctx)
    G = I["G"]
    U = [G.toElementArray(c) for c in I["u"]]
    counts = {}
    for width in (1, 3):
        ver = nat.DistrElGamalSessionBasic(G, 1, 3, 2, NE)
        ver.setInstance(U[:width] if width > 1 else U[0], I["ys"], [None] * 4)
        ver.setBatchVector(I["e"])
        gpu_ctx.timing_enable(True)
        try:
            gpu_ctx.timing_reset()
            ver.batchInput()
            counts[width] = gpu_ctx.timing_get("expprod_sort")[0]
        finally:
            gpu_ctx.timing_enable(False)
            gpu_ctx.timing_reset()
    assert counts[1] > 0 and counts[3] == counts[1], counts
