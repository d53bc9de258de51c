"""CPU suite: the width-omega restatement of DistrElGamalSessionBasic (tests/wide_decrypt_ref.py) against the width-1 oracle
(oracle/pyref_proofs.py) at omega = 1, and against itself at omega = 3: decryption recovers the plaintexts and the honest
proofs verify, per party and combined; a wrong factor component, a wrong reply and a reply >= q do not."""
from conftest import load_golden
from oracle import pyref, pyref_proofs as P
from tape import Tape

import wide_decrypt_ref as W


def instance(bits, n, k, thr, width, seed):
    grp, _ = load_golden(bits)
    p, q, g = grp["p"], grp["q"], grp["g"]
    t = Tape(seed, q)
    coeffs = t.ring_array(thr)                                     # Shamir sharing of x = coeffs[0] over Z_q
    share = lambda j: sum(c * pow(j, d, q) for d, c in enumerate(coeffs)) % q
    xs = [None] + [share(j) for j in range(1, k + 1)]
    ys = [None] + [pow(g, xj, p) for xj in xs[1:]]
    y = pow(g, coeffs[0], p)
    msgs = [pyref.exp_fixed(g, t.ring_array(n), p) for _ in range(width)]
    rs = [t.ring_array(n) for _ in range(width)]
    u = [pyref.exp_fixed(g, r, p) for r in rs]
    v = [pyref.mul(m, pyref.exp_fixed(y, r, p), p) for m, r in zip(msgs, rs)]
    return dict(p=p, q=q, g=g, xs=xs, ys=ys, y=y, msgs=msgs, u=u, v=v, e=t.int_array(n, 100), chal=t.int_array(1, 100)[0])


def test_width_one_is_the_width_one_oracle():
    k, thr = 3, 2
    I = instance(512, 12, k, thr, 1, b"wide-ref-1")
    p, q = I["p"], I["q"]
    K = W.adapter_modp(p, q)
    for kk in (1, 2, 3, 5, 7, 9, 16, 27):
        assert W.prod_factor(q, kk) == P.prod_factor(q, kk), kk
    f = [None] + [W.decryption_factors(K, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    for j in range(1, k + 1):
        assert f[j] == [P.decryption_factors(I["u"][0], I["xs"][j], p, q, k)]
    for bad in ((), (1,), (2,), (3,)):
        correct = [False] + [j not in bad for j in range(1, k + 1)]
        assert W.lagrange_integers(q, correct, k, thr) == P.lagrange_integers(q, correct, k, thr)
        got = W.combine_decryption_factors(K, f, correct, k, thr)
        assert got == [P.combine_decryption_factors([None] + [fj[0] for fj in f[1:]], correct, k, thr, p, q)]
        assert W.plaintexts(K, I["v"], got) == I["msgs"]


def test_width_three_decrypts_and_its_proofs_verify():
    k, thr, width = 3, 2, 3
    I = instance(512, 10, k, thr, width, b"wide-ref-3")
    p, q, g, chal = I["p"], I["q"], I["g"], I["chal"]
    K = W.adapter_modp(p, q)
    f = [None] + [W.decryption_factors(K, I["u"], I["xs"][j], k) for j in range(1, k + 1)]
    correct = [False] + [True] * k
    comb = W.combine_decryption_factors(K, f, correct, k, thr)
    assert W.plaintexts(K, I["v"], comb) == I["msgs"]
    s = W.run_session(K, g, I["u"], I["ys"], I["xs"], f, I["e"], chal, k, thr, lambda j: Tape(b"party%d" % j, q))
    ver = s["verifier"]
    assert len(ver.A) == width and all(len(s["commit"][j][1]) == width for j in range(1, k + 1))
    assert all(ver.verify(j, chal) for j in range(1, k + 1))
    ver.combine(correct, I["y"], comb)
    ver.batchCombined()
    assert ver.verifyCombined(chal)
    # a wrong reply, a reply that is no field element
    ver.setReply(1, (s["reply"][1] + 1) % q)
    assert not ver.verify(1, chal)
    ver.setReply(1, s["reply"][1] + q)
    assert not ver.verify(1, chal)
    ver.setReply(1, s["reply"][1])
    assert ver.verify(1, chal)
    # one element of ONE component of party 2's factors is wrong: party 2 fails, the others and their combination do not
    f[2][1] = list(f[2][1])
    f[2][1][4] = f[2][1][4] * g % p
    ver.batch(2)
    assert not ver.verify(2, chal) and ver.verify(1, chal) and ver.verify(3, chal)
    correct[2] = False
    comb2 = W.combine_decryption_factors(K, f, correct, k, thr)
    assert W.plaintexts(K, I["v"], comb2) == I["msgs"]
    ver.combine(correct, I["y"], comb2)
    ver.batchCombined()
    assert ver.verifyCombined(chal)
