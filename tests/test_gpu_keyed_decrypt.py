"""GPU suite, row A6 under a public key of width kappa: the C++ decryption drivers (vmn_decryption_factors_keyed,
vmn_combine_decryption_factors_wide, vmn_decproof_* after vmn_decproof_set_instance_keyed) through verificatum_vmn_amd.native
against the restatement of DistrElGamalSessionBasic over (G^kappa)^omega (tests/keyed_decrypt_ref.py).  Both sides draw from
the same tape, so factors, combined factors, commitments (y', B'), replies, verdicts and plaintexts compare exactly.  The last
test takes the whole path of a list mixed under a key of width 2: re-encrypted and permuted under the wide key whose y-rows
repeat with period kappa, proved, verified, and opened.

Wall time on an MI355X: not measured yet, for this module and for the existing GPU modules beside it."""
import pytest

from conftest import load_golden
from oracle import pyref, pyref_proofs as P
from oracle.pyref_ec import Curve
from tape import Tape

import keyed_decrypt_ref as KD
import wide_decrypt_ref as W

pytestmark = pytest.mark.gpu

NE, NV = 100, 100
CASES = [("modp", 512, 40, 3, 2, 2, 1, ()), ("modp", 2048, 130, 5, 3, 3, 2, (2,)), ("P-256", 256, 24, 3, 2, 2, 2, ())]


@pytest.fixture(scope="module")
def nat(entry):
    import mirror
    return mirror.load(entry, ("native",))["native"]


def make_instance(kind, bits, n, k, thr, kw, omega, vmn, gpu_ctx):
    """Group, adapter, kappa independent Shamir sharings of the key, a list of n ciphertexts of (G^kappa)^omega and their
    plaintexts."""
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
    t = Tape(b"keyed-dec/%s%d/%d%d" % (kind.encode(), bits, kw, omega), q)
    xs, ys, y = KD.shamir_keys(K, g, t, kw, k, thr)
    msgs, u, v = KD.encrypt(K, g, y, t, kw, omega, n)
    return dict(G=G, K=K, q=q, g=g, kw=kw, xs=xs, ys=ys, y=y, msgs=msgs, u=u, v=v, e=t.int_array(n, NE), chal=t.int_array(1, NV)[0],
                bad_element=bad_element)


def ints_of(arrays):
    return [a.toInts() for a in arrays]


def gpu_session(nat, I, U, F, k, thr, seed, keyed=True, cls=None):
    """Every party's prover and one verifier (party 1) on the GPU: {"commit", "reply", "verifier"} as KD.run_session.
    keyed = False (key width 1 only): the same through the scalars of the interface without a key width."""
    G, kw = I["G"], I["kw"]
    ys = I["ys"] if keyed else [None] + [y[0] for y in I["ys"][1:]]
    def session(j, rand=None):
        s = (cls or nat.DistrElGamalSessionBasic)(G, j, k, thr, NE, rand=rand)
        if keyed:
            s.setInstance(U, ys, F, keywidth=kw)
        else:
            s.setInstance(U, ys, F)
        s.setBatchVector(I["e"])
        s.batchInput()
        return s
    ver = session(1)
    out = {"commit": {}, "reply": {}, "verifier": ver}
    for j in range(1, k + 1):
        pr = session(j, rand=Tape(seed + b"%d" % j, I["q"]))
        out["commit"][j] = pr.commit(I["xs"][j] if keyed else I["xs"][j][0])
        out["reply"][j] = pr.reply(I["chal"])
        ver.setCommitment(j, *out["commit"][j])
        ver.setReply(j, out["reply"][j])
        ver.batch(j)
    return out


def keyed_call(nat, fn, U, kw, *args):
    """The keyed entry points at ANY key width, 1 included (the Python surface routes key width 1 to the older entry points)."""
    import ctypes as C
    return fn(U[0].group._h, C.c_size_t(kw), C.c_size_t(len(U) // kw), nat._opt_ptr_array(U), *args)


@pytest.mark.parametrize("kind,bits,n,k,thr,kw,omega,bad", CASES)
def test_keyed_threshold_decryption_equals_the_restatement(kind, bits, n, k, thr, kw, omega, bad, nat, vmn, gpu_ctx):
    I = make_instance(kind, bits, n, k, thr, kw, omega, vmn, gpu_ctx)
    G, K, q, g, chal, width = I["G"], I["K"], I["q"], I["g"], I["chal"], kw * omega
    correct = [False] + [j not in bad for j in range(1, k + 1)]
    U = [G.toElementArray(c) for c in I["u"]]
    V = [G.toElementArray(c) for c in I["v"]]
    # every party's factors in every component
    f_o = [None] + [KD.decryption_factors(K, kw, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    F = [None] + [nat.decryptionFactors(U, list(I["xs"][j]), q, k) for j in range(1, k + 1)]
    for j in range(1, k + 1):
        assert isinstance(F[j], list) and ints_of(F[j]) == f_o[j], j
    # the combined factors and the plaintexts
    comb_o = KD.combine_decryption_factors(K, f_o, correct, k, thr)
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    assert ints_of(comb) == comb_o
    plain = nat.plaintexts(V, comb)
    assert ints_of(plain) == KD.plaintexts(K, I["v"], comb_o) == I["msgs"]
    # (y', B') and the reply of every party: the same tape on both sides
    seed = b"keyed-party/"
    ref = KD.run_session(K, g, kw, I["u"], I["ys"], I["xs"], f_o, I["e"], chal, k, thr, lambda j: Tape(seed + b"%d" % j, q))
    got = gpu_session(nat, I, U, F, k, thr, seed)
    ver, ver_o = got["verifier"], ref["verifier"]
    for j in range(1, k + 1):
        assert got["commit"][j] == ref["commit"][j], j
        assert len(got["commit"][j][0]) == kw and len(got["commit"][j][1]) == width, j
        assert got["reply"][j] == ref["reply"][j] and len(got["reply"][j]) == kw, j
    # per-party and combined verdicts
    for j in range(1, k + 1):
        assert ver.verify(j, chal) == ver_o.verify(j, chal) == True, j
    ver.combine(correct, I["y"], comb)
    ver.batchCombined()
    ver_o.combine(correct, I["y"], comb_o)
    ver_o.batchCombined()
    assert ver.verifyCombined(chal) == ver_o.verifyCombined(chal) == True
    assert not ver.verifyCombined(chal + 1) and not ver_o.verifyCombined(chal + 1)
    # a reply whose SECOND row is >= q is no element of Z_q^kappa: verdict false, on both sides
    good = got["reply"][1]
    big = good[1] + q                                                  # the same class mod q where the wire width holds it
    if big >= 1 << (8 * G.exp_bytes):
        big = q
    bad_reply = (good[0], big) + tuple(good[2:])
    ver.setReply(1, bad_reply)
    ver_o.setReply(1, bad_reply)
    assert ver.verify(1, chal) == ver_o.verify(1, chal) == False
    ver.setReply(1, good)
    ver_o.setReply(1, good)
    assert ver.verify(1, chal) == ver_o.verify(1, chal) == True
    # y' whose second row is no group element: the whole commitment is refused
    yp2, Bp2 = got["commit"][2]
    with pytest.raises(vmn.VmnError) as ei:
        ver.setCommitment(2, (yp2[0], I["bad_element"]) + tuple(yp2[2:]), Bp2)
    assert ei.value.status == -4                                       # VMN_ERR_FORMAT
    assert ver.verify(2, chal)                                         # (the commitment set before stands)


def test_a_share_wrong_under_one_key_fails_that_party_only(nat, vmn, gpu_ctx):
    kind, bits, n, k, thr, kw, omega = "modp", 512, 40, 3, 2, 2, 2
    I = make_instance(kind, bits, n, k, thr, kw, omega, vmn, gpu_ctx)
    G, K, q, g, chal = I["G"], I["K"], I["q"], I["g"], I["chal"]
    U = [G.toElementArray(c) for c in I["u"]]
    V = [G.toElementArray(c) for c in I["v"]]
    shares = [None] + [list(x) for x in I["xs"][1:]]
    shares[2][1] = (shares[2][1] + 1) % q                              # party 2: a wrong share under key 1 only
    f_o = [None] + [KD.decryption_factors(K, kw, I["u"], shares[j], k) for j in range(1, k + 1)]
    F = [None] + [nat.decryptionFactors(U, shares[j], q, k) for j in range(1, k + 1)]
    for j in range(1, k + 1):
        assert ints_of(F[j]) == f_o[j], j
    seed = b"keyed-bad/"
    ref = KD.run_session(K, g, kw, I["u"], I["ys"], I["xs"], f_o, I["e"], chal, k, thr, lambda j: Tape(seed + b"%d" % j, q))
    got = gpu_session(nat, I, U, F, k, thr, seed)
    ver, ver_o = got["verifier"], ref["verifier"]
    verdicts = [ver.verify(j, chal) for j in range(1, k + 1)]
    assert verdicts == [ver_o.verify(j, chal) for j in range(1, k + 1)] == [True, False, True]
    correct = [False, True, False, True]
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    assert ints_of(comb) == KD.combine_decryption_factors(K, f_o, correct, k, thr)
    ver.combine(correct, I["y"], comb)
    ver.batchCombined()
    assert ver.verifyCombined(chal)
    assert ints_of(nat.plaintexts(V, comb)) == I["msgs"]
    # with party 2 counted as correct the combination is wrong and its proof fails
    wrong = nat.combineDecryptionFactors(F, [False, True, True, True], k, thr, q)
    ver.combine([False, True, True, True], I["y"], wrong)
    ver.batchCombined()
    assert not ver.verifyCombined(chal)


def counted(ctx, names, fn):
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        out = fn()
        return out, {name: ctx.timing_get(name)[0] for name in names}
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()


def test_key_width_one_through_the_keyed_entry_points_is_the_wide_path(nat, vmn, gpu_ctx):
    """vmn_decryption_factors_keyed and vmn_decproof_set_instance_keyed with keywidth = 1 (called directly: the Python surface
    routes key width 1 to the older entry points): the transcript of set_instance_wide, the modpow launches of
    vmn_decryption_factors_wide and the expprod launches of a wide session."""
    import ctypes as C
    kind, bits, n, k, thr, omega = "modp", 512, 40, 3, 2, 3
    I = make_instance(kind, bits, n, k, thr, 1, omega, vmn, gpu_ctx)
    G, q, chal = I["G"], I["q"], I["chal"]
    U = [G.toElementArray(c) for c in I["u"]]
    correct = [False] + [True] * k
    xs1 = [None] + [x[0] for x in I["xs"][1:]]

    def keyed_factors(j):
        outs = (C.c_void_p * omega)()
        nat._check(keyed_call(nat, nat.plib().vmn_decryption_factors_keyed, U, 1, nat.int_to_be(xs1[j] % q, G.exp_bytes), C.c_int(k), outs))
        return [vmn.PGroupElementArray(G, C.c_void_p(h)) for h in outs]

    Fw, Fk = [None], [None]
    for j in range(1, k + 1):
        fw, cw = counted(gpu_ctx, ("modpow",), lambda: nat.decryptionFactors(U, xs1[j], q, k))
        fk, ck = counted(gpu_ctx, ("modpow",), lambda: keyed_factors(j))
        assert ck == cw and cw["modpow"] == 1, (cw, ck)
        assert [a.toBytes() for a in fk] == [a.toBytes() for a in fw]
        Fw.append(fw)
        Fk.append(fk)
    comb = nat.combineDecryptionFactors(Fw, correct, k, thr, q)

    # the Python surface with keywidth = 1 is the older interface: a subclass that sets its instance through set_instance_keyed
    class KeyedOne(nat.DistrElGamalSessionBasic):
        def setInstance(self, u, y, f, keywidth=1):
            ybuf = b"".join(self.G.enc_el(el) if el is not None else bytes(self.G.elem_bytes) for el in y)
            self._keep, self.width, self.keywidth = [u, f], len(u), 1
            self._call("set_instance_keyed", C.c_size_t(1), C.c_size_t(len(u)), nat._opt_ptr_array(u), ybuf, nat._wide_factor_table(f, len(u)))

    def run(cls, F):
        def body():
            s = gpu_session(nat, I, U, F, k, thr, b"keyed-one/", keyed=False, cls=cls)
            verdicts = [s["verifier"].verify(j, chal) for j in range(1, k + 1)]
            s["verifier"].combine(correct, I["y"][0], comb)
            s["verifier"].batchCombined()
            return s, verdicts + [s["verifier"].verifyCombined(chal), s["verifier"].verifyCombined(chal ^ 1)]
        return counted(gpu_ctx, ("expprod", "expprod_agg", "expprod_sort"), body)

    (sw, vw), cw = run(nat.DistrElGamalSessionBasic, Fw)
    (sk, vk), ck = run(KeyedOne, Fk)
    assert plib_keywidth(nat, sk["verifier"]) == 1 and plib_width(nat, sk["verifier"]) == omega
    assert vw == vk == [True] * k + [True, False]
    assert ck == cw and cw["expprod_sort"] > 0, (cw, ck)
    for j in range(1, k + 1):
        assert sk["commit"][j] == sw["commit"][j] and sk["reply"][j] == sw["reply"][j], j


def plib_keywidth(nat, session):
    return nat.plib().vmn_decproof_keywidth(session._h)


def plib_width(nat, session):
    return nat.plib().vmn_decproof_width(session._h)


def test_witness_one_partys_factors_under_six_components_are_one_launch(nat, vmn, gpu_ctx):
    """2048 bits, kappa omega = 6 component arrays under three different secrets: ONE modpow launch."""
    kind, bits, n, k, thr, kw, omega = "modp", 2048, 130, 5, 3, 3, 2
    I = make_instance(kind, bits, n, k, thr, kw, omega, vmn, gpu_ctx)
    G, K, q = I["G"], I["K"], I["q"]
    U = [G.toElementArray(c) for c in I["u"]]
    f, counts = counted(gpu_ctx, ("modpow",), lambda: nat.decryptionFactors(U, list(I["xs"][1]), q, k))
    assert counts["modpow"] == 1, counts
    assert ints_of(f) == KD.decryption_factors(K, kw, I["u"], I["xs"][1], k)
    ver = nat.DistrElGamalSessionBasic(G, 1, k, thr, NE)
    ver.setInstance(U, I["ys"], [None] * (k + 1), keywidth=kw)
    assert plib_keywidth(nat, ver) == kw and plib_width(nat, ver) == kw * omega


def test_a_list_mixed_under_a_key_of_width_two_is_shuffled_proved_and_opened(nat, vmn, gpu_ctx):
    """The path of the reference's keywidth32 run at N = 12, kappa = 2, omega = 2.  The shuffle side takes the key as 2 W rows
    (g repeated, then y_0, y_1, y_0, y_1) and needs nothing for the key width; the decryption side opens the output with the
    keyed entry points: the plaintexts are the permuted messages."""
    kind, bits, n, k, thr, kw, omega = "modp", 512, 12, 3, 2, 2, 2
    NVp, NEp, NRp = 100, 100, 50
    I = make_instance(kind, bits, n, k, thr, kw, omega, vmn, gpu_ctx)
    G, K, q, g, chal, width = I["G"], I["K"], I["q"], I["g"], I["chal"], kw * omega
    p = K.p
    t = Tape(b"keyed-mix", q)
    pkey = [g] * width + [I["y"][c % kw] for c in range(width)]
    w = I["u"] + I["v"]
    h = pyref.exp_fixed(g, t.ring_array(n), p)
    pi, s, e, v = t.permutation(n), [t.ring_array(n) for _ in range(width)], t.int_array(n, NEp), t.int_array(1, NVp)[0]
    # re-encrypt and permute; prove; the transcript against the oracle under the same key rows
    o = P.PoS(p, q, NVp, NEp, NRp, rand=Tape(b"keyed-mix/prover", q))
    o.precompute(g, h, pi)
    wp_o = P.reencrypt(w, P.reenc_factors(pkey, s, p), pi, p)
    o.setInstance(pkey, w, wp_o, s)
    o.setBatchVector(e)
    com_o, rep_o = o.commit(), o.reply(v)
    H, Wd, S = G.toElementArray(h), [G.toElementArray(c) for c in w], [G.ringArray(c) for c in s]
    WP = nat.reencrypt_native(G, pkey, Wd, S, pi)
    assert ints_of(WP) == wp_o
    pr = nat.PoSBasicTW(G, NVp, NEp, NRp, rand=Tape(b"keyed-mix/prover", q))
    pr.precompute(g, H, pi)
    pr.setInstance(pkey, Wd, WP, S)
    pr.setBatchVector(e)
    com, rep = pr.commit(), pr.reply(v)
    val = lambda x: x.toInts() if hasattr(x, "toInts") else x
    assert {key: val(x) for key, x in com.items()} == com_o and {key: val(x) for key, x in rep.items()} == rep_o
    ver = nat.PoSBasicTW(G, NVp, NEp, NRp)
    ver.precompute(g, H)
    ver.setPermutationCommitment(pr.u)
    ver.setInstance(pkey, Wd, WP)
    ver.setBatchVector(e)
    ver.computeAF()
    ver.setCommitment(com)
    ver.setChallenge(v)
    assert ver.verify(rep)
    # open the output
    U2, V2 = WP[:width], WP[width:]
    u2 = wp_o[:width]
    F = [None] + [nat.decryptionFactors(U2, list(I["xs"][j]), q, k) for j in range(1, k + 1)]
    f_o = [None] + [KD.decryption_factors(K, kw, u2, I["xs"][j], k) for j in range(1, k + 1)]
    for j in range(1, k + 1):
        assert ints_of(F[j]) == f_o[j], j
    I2 = dict(I)
    seed = b"keyed-mix/party"
    got = gpu_session(nat, I2, U2, F, k, thr, seed)
    ref = KD.run_session(K, g, kw, u2, I["ys"], I["xs"], f_o, I["e"], chal, k, thr, lambda j: Tape(seed + b"%d" % j, q))
    dver = got["verifier"]
    for j in range(1, k + 1):
        assert got["commit"][j] == ref["commit"][j] and got["reply"][j] == ref["reply"][j], j
        assert dver.verify(j, chal), j
    correct = [False, True, True, False]
    comb = nat.combineDecryptionFactors(F, correct, k, thr, q)
    dver.combine(correct, I["y"], comb)
    dver.batchCombined()
    assert dver.verifyCombined(chal)
    inverse = P.inv_perm(pi)
    assert ints_of(nat.plaintexts(V2, comb)) == [pyref.permute(m, inverse) for m in I["msgs"]]
