"""Test infrastructure: verifiable threshold decryption under a public key of width kappa, in Python integers / affine points.

A restatement of the reference's elgamal/DistrElGamalSession.java:365-389 and DistrElGamalSessionBasic.java:524-540, 595-613,
642-727 with the key group G^kappa (ProtocolElGamal.getKeyPGroup) and the plaintext group (G^kappa)^omega: W = kappa * omega
component arrays, component c = l * kappa + j the key j of plaintext component l.  The secret key, the randomizer r and the reply
k_x are kappa field elements, a public key and y' kappa group elements, key 0 first; an exponent of Z_q^kappa acts on component
c through its entry c mod kappa.  g = (g, ..., g), and the challenge stays one field element.

Written against the group adapter K of oracle/pyref_proofs.py, like tests/wide_decrypt_ref.py, whose threshold integers this
module uses; with kappa = 1 every value here is the 1-tuple of that module's value.  A keyed array is a list of W lists."""
from wide_decrypt_ref import lagrange_integers, prod_factor


def decryption_factors(K, kw: int, u, x_j, k: int):
    """f_c = u_c^(-x_{c mod kappa} / c_k); x_j: the kappa secrets of the party."""
    inv = pow(prod_factor(K.q, k), -1, K.q)
    return [K.exp_scalar(uc, (-x_j[c % kw]) * inv % K.q) for c, uc in enumerate(u)]


def combine_decryption_factors(K, factors, correct, k: int, threshold: int):
    """prod_t f_{j_t}^(lambda_t) in every component: the threshold integers are scalars, nothing depends on the key width."""
    idx = [l for l in range(1, k + 1) if correct[l]][:threshold]
    ints = lagrange_integers(K.q, correct, k, threshold)
    out = []
    for c in range(len(factors[idx[0]])):
        acc = None
        for l, lam in zip(idx, ints):
            term = K.exp_scalar(factors[l][c], lam % K.q)
            acc = term if acc is None else K.mul_arrays(acc, term)
        out.append(acc)
    return out


def plaintexts(K, v, combined):
    return [K.mul_arrays(vc, fc) for vc, fc in zip(v, combined)]


class KeyedDistrElGamalSessionBasic:
    """One instance per party j; prover of j and verifier of every l.  rand: a tape (ring_array(kappa): r_0 first)."""

    def __init__(self, K, g, kw: int, j: int, k: int, threshold: int, rand=None):
        self.K, self.q, self.g, self.kw, self.j, self.k, self.threshold, self.rand = K, K.q, g, kw, j, k, threshold, rand
        self.inverseFactor = pow(prod_factor(K.q, k), -1, K.q)
        self.yp, self.Bp, self.B, self.k_x = {}, {}, {}, {}
        self.bad_reply = set()

    def setInstance(self, u, y, f):
        """u: W arrays; y[l]: the kappa public keys of party l; f[l]: the W factor arrays of party l."""
        assert len(u) % self.kw == 0
        self.u, self.y, self.f, self.width = u, y, f, len(u)

    def setBatchVector(self, e):
        self.e = list(e)

    def _expprod(self, arrays):
        return [self.K.exp_prod(a, self.e) for a in arrays]

    def batchInput(self):
        self.A = self._expprod(self.u)

    def commit(self, x):
        K, kw = self.K, self.kw
        self.x = tuple(xi % self.q for xi in x)
        self.r = tuple(self.rand.ring_array(kw))                                          # randomElement of Z_q^kappa
        self.yp[self.j] = tuple(K.exp(self.g, ri) for ri in self.r)                       # y'_j = g^(r_j)
        self.Bp[self.j] = tuple(K.exp(Ac, self.r[c % kw]) for c, Ac in enumerate(self.A))  # B'_c = A_c^(r_{c mod kappa})
        return self.yp[self.j], self.Bp[self.j]

    def reply(self, v: int):
        q = self.q
        self.k_x[self.j] = tuple(((-xi) * self.inverseFactor % q * (v % q) + ri) % q for xi, ri in zip(self.x, self.r))
        return self.k_x[self.j]

    def setCommitment(self, l: int, yp, Bp):
        self.yp[l], self.Bp[l] = tuple(yp), tuple(Bp)

    def setReply(self, l: int, k_x):
        if any(not 0 <= kv < self.q for kv in k_x):            # one row that is no field element: the zero of Z_q^kappa, verdict false
            self.k_x[l] = (0,) * self.kw
            self.bad_reply.add(l)
        else:
            self.k_x[l] = tuple(k_x)
            self.bad_reply.discard(l)

    def batch(self, l: int):
        self.B[l] = self._expprod(self.f[l])

    def _check(self, y, yexp, yp, B, Bp, v, k_x) -> bool:
        K, kw = self.K, self.kw
        ok = True
        for i in range(kw):
            ok = ok and K.mul(K.exp(K.inv(y[i]), yexp), yp[i]) == K.exp(self.g, k_x[i])
        for c, (Bc, Bpc, Ac) in enumerate(zip(B, Bp, self.A)):
            ok = ok and K.mul(K.exp(Bc, v), Bpc) == K.exp(Ac, k_x[c % kw])
        return ok

    def verify(self, l: int, v: int) -> bool:
        if l in self.bad_reply:
            return False
        return self._check(self.y[l], self.inverseFactor * (v % self.q) % self.q, self.yp[l], self.B[l], self.Bp[l], v % self.q, self.k_x[l])

    def combine(self, correct, combinedy, combinedf):
        K, kw = self.K, self.kw
        idx = [l for l in range(1, self.k + 1) if correct[l]][:self.threshold]
        ints = lagrange_integers(self.q, correct, self.k, self.threshold)
        self.combinedyp, self.combinedBp, self.combinedk_x = [None] * kw, [None] * self.width, [0] * kw
        for l, lam in zip(idx, ints):
            ex = lam % self.q
            for i in range(kw):
                t = K.exp(self.yp[l][i], ex)
                self.combinedyp[i] = t if self.combinedyp[i] is None else K.mul(self.combinedyp[i], t)
                self.combinedk_x[i] = (self.combinedk_x[i] + self.k_x[l][i] * ex) % self.q
            for c in range(self.width):
                t = K.exp(self.Bp[l][c], ex)
                self.combinedBp[c] = t if self.combinedBp[c] is None else K.mul(self.combinedBp[c], t)
        self.combinedy, self.combinedf = tuple(combinedy), combinedf

    def batchCombined(self):
        self.combinedB = self._expprod(self.combinedf)

    def verifyCombined(self, v: int) -> bool:
        return self._check(self.combinedy, v % self.q, self.combinedyp, self.combinedB, self.combinedBp, v % self.q, self.combinedk_x)


def shamir_keys(K, g, tape, kw: int, k: int, threshold: int):
    """kappa independent Shamir sharings over Z_q: (xs, ys, y) with xs[l] / ys[l] the kappa secret / public shares of party l
    (entry 0 unused) and y the kappa joint public keys."""
    q = K.q
    coeffs = [tape.ring_array(threshold) for _ in range(kw)]
    share = lambda i, j: sum(cf * pow(j, d, q) for d, cf in enumerate(coeffs[i])) % q
    xs = [None] + [tuple(share(i, j) for i in range(kw)) for j in range(1, k + 1)]
    ys = [None] + [tuple(K.exp(g, xi) for xi in xj) for xj in xs[1:]]
    return xs, ys, tuple(K.exp(g, coeffs[i][0]) for i in range(kw))


def encrypt(K, g, y, tape, kw: int, omega: int, n: int):
    """n plaintexts of (G^kappa)^omega and their ciphertexts under the key y of width kappa: (msgs, u, v), W arrays each."""
    W = kw * omega
    msgs = [K.exp_fixed(g, tape.ring_array(n)) for _ in range(W)]
    rs = [tape.ring_array(n) for _ in range(W)]
    u = [K.exp_fixed(g, r) for r in rs]
    v = [K.mul_arrays(m, K.exp_fixed(y[c % kw], r)) for c, (m, r) in enumerate(zip(msgs, rs))]
    return msgs, u, v


def run_session(K, g, kw, u, y, xs, f, e, chal, k: int, threshold: int, tape_of):
    """Every party commits and replies (tape_of(j): party j's random tape); returns the transcript the verifier of party 1 sees:
    {"commit": {j: (y', B')}, "reply": {j: k_x}, "verifier": the session object with everything set}."""
    ver = KeyedDistrElGamalSessionBasic(K, g, kw, 1, k, threshold)
    ver.setInstance(u, y, f)
    ver.setBatchVector(e)
    ver.batchInput()
    out = {"commit": {}, "reply": {}, "verifier": ver}
    for j in range(1, k + 1):
        pr = KeyedDistrElGamalSessionBasic(K, g, kw, j, k, threshold, rand=tape_of(j))
        pr.setInstance(u, y, f)
        pr.setBatchVector(e)
        pr.batchInput()
        out["commit"][j] = pr.commit(xs[j])
        out["reply"][j] = pr.reply(chal)
        ver.setCommitment(j, *out["commit"][j])
        ver.setReply(j, out["reply"][j])
        ver.batch(j)
    return out
