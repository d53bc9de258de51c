"""CPU suite: the restatement of threshold decryption under a key of width kappa (tests/keyed_decrypt_ref.py) against the
width-omega restatement (tests/wide_decrypt_ref.py) at kappa = 1 on the same tape, and against itself at (kappa, omega) =
(2, 1) and (3, 2): decryption recovers the plaintexts, the honest proofs verify per party and combined, and a share that is
wrong under ONE key fails its party and nobody else.  Over the 512-bit golden group and over P-256."""
import pytest

from conftest import load_golden
from oracle.pyref_ec import Curve
from tape import Tape

import keyed_decrypt_ref as KD
import wide_decrypt_ref as W

K_PARTIES, THR = 3, 2
GROUPS = [("modp", 6), ("P-256", 4)]


def group(kind):
    if kind == "modp":
        grp, _ = load_golden(512)
        return W.adapter_modp(grp["p"], grp["q"]), grp["g"]
    c = Curve(kind)
    return W.adapter_curve(c), c.g


def instance(kind, n, kw, omega, seed):
    K, g = group(kind)
    t = Tape(seed, K.q)
    xs, ys, y = KD.shamir_keys(K, g, t, kw, K_PARTIES, THR)
    msgs, u, v = KD.encrypt(K, g, y, t, kw, omega, n)
    return dict(K=K, g=g, q=K.q, xs=xs, ys=ys, y=y, msgs=msgs, u=u, v=v, e=t.int_array(n, 100), chal=t.int_array(1, 100)[0])


@pytest.mark.parametrize("kind,n", GROUPS)
def test_key_width_one_is_the_wide_restatement_on_the_same_tape(kind, n):
    k, thr, omega = K_PARTIES, THR, 2
    I = instance(kind, n, 1, omega, b"keyed-ref-1/" + kind.encode())
    K, g, q, chal = I["K"], I["g"], I["q"], I["chal"]
    xs1 = [None] + [x[0] for x in I["xs"][1:]]
    ys1 = [None] + [y[0] for y in I["ys"][1:]]
    f = [None] + [KD.decryption_factors(K, 1, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    f_w = [None] + [W.decryption_factors(K, I["u"], xs1[j], k) for j in range(1, k + 1)]
    assert f == f_w
    correct = [False, True, False, True]
    comb = KD.combine_decryption_factors(K, f, correct, k, thr)
    assert comb == W.combine_decryption_factors(K, f_w, correct, k, thr)
    assert KD.plaintexts(K, I["v"], comb) == W.plaintexts(K, I["v"], comb) == I["msgs"]
    tape_of = lambda j: Tape(b"keyed-ref-1/party%d" % j, q)
    s = KD.run_session(K, g, 1, I["u"], I["ys"], I["xs"], f, I["e"], chal, k, thr, tape_of)
    s_w = W.run_session(K, g, I["u"], ys1, xs1, f_w, I["e"], chal, k, thr, tape_of)
    for j in range(1, k + 1):
        (yp,), Bp = s["commit"][j]
        assert (yp, Bp) == s_w["commit"][j] and s["reply"][j] == (s_w["reply"][j],), j
        assert s["verifier"].verify(j, chal) == s_w["verifier"].verify(j, chal) == True
    s["verifier"].combine(correct, I["y"], comb)
    s_w["verifier"].combine(correct, I["y"][0], comb)
    for ver in (s["verifier"], s_w["verifier"]):
        ver.batchCombined()
    assert s["verifier"].combinedyp == [s_w["verifier"].combinedyp] and s["verifier"].combinedBp == s_w["verifier"].combinedBp
    assert s["verifier"].combinedk_x == [s_w["verifier"].combinedk_x]
    assert s["verifier"].verifyCombined(chal) == s_w["verifier"].verifyCombined(chal) == True
    assert s["verifier"].verifyCombined(chal + 1) == s_w["verifier"].verifyCombined(chal + 1) == False


@pytest.mark.parametrize("kw,omega", [(2, 1), (3, 2)])
@pytest.mark.parametrize("kind,n", GROUPS)
def test_an_honest_run_verifies_and_decrypts(kind, n, kw, omega):
    k, thr = K_PARTIES, THR
    I = instance(kind, n, kw, omega, b"keyed-ref/%s/%d%d" % (kind.encode(), kw, omega))
    K, g, q, chal = I["K"], I["g"], I["q"], I["chal"]
    f = [None] + [KD.decryption_factors(K, kw, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    s = KD.run_session(K, g, kw, I["u"], I["ys"], I["xs"], f, I["e"], chal, k, thr, lambda j: Tape(b"keyed-ref/party%d" % j, q))
    ver = s["verifier"]
    for j in range(1, k + 1):
        yp, Bp = s["commit"][j]
        assert len(yp) == kw and len(Bp) == kw * omega and len(s["reply"][j]) == kw
        assert ver.verify(j, chal), j
    for correct in ([False, True, True, True], [False, False, True, True]):
        comb = KD.combine_decryption_factors(K, f, correct, k, thr)
        assert KD.plaintexts(K, I["v"], comb) == I["msgs"]
        ver.combine(correct, I["y"], comb)
        ver.batchCombined()
        assert ver.verifyCombined(chal) and not ver.verifyCombined(chal + 1)
    # a reply with one row that is no field element costs the party its verdict; restored, the verdict is back
    good = s["reply"][1]
    ver.setReply(1, good[:-1] + (good[-1] + q,))
    assert not ver.verify(1, chal) and ver.k_x[1] == (0,) * kw
    ver.setReply(1, good)
    assert ver.verify(1, chal)


@pytest.mark.parametrize("kw,omega", [(2, 1), (3, 2)])
@pytest.mark.parametrize("kind,n", GROUPS)
def test_a_share_wrong_under_one_key_fails_its_party_only(kind, n, kw, omega):
    k, thr = K_PARTIES, THR
    I = instance(kind, n, kw, omega, b"keyed-ref-bad/%s/%d%d" % (kind.encode(), kw, omega))
    K, g, q, chal = I["K"], I["g"], I["q"], I["chal"]
    f = [None] + [KD.decryption_factors(K, kw, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    wrong = list(I["xs"][2])
    wrong[kw - 1] = (wrong[kw - 1] + 1) % q                               # party 2 uses a wrong share under the last key only
    f[2] = KD.decryption_factors(K, kw, I["u"], tuple(wrong), k)
    honest = KD.decryption_factors(K, kw, I["u"], I["xs"][2], k)
    assert [c for c in range(kw * omega) if f[2][c] != honest[c]] == [c for c in range(kw * omega) if c % kw == kw - 1]
    s = KD.run_session(K, g, kw, I["u"], I["ys"], I["xs"], f, I["e"], chal, k, thr, lambda j: Tape(b"keyed-ref-bad/party%d" % j, q))
    ver = s["verifier"]
    assert [ver.verify(j, chal) for j in range(1, k + 1)] == [True, False, True]
    correct = [False, True, False, True]
    comb = KD.combine_decryption_factors(K, f, correct, k, thr)
    assert KD.plaintexts(K, I["v"], comb) == I["msgs"]
    ver.combine(correct, I["y"], comb)
    ver.batchCombined()
    assert ver.verifyCombined(chal)
