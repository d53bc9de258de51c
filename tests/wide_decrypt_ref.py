"""Test infrastructure: verifiable threshold decryption of width-omega ciphertext lists in Python integers / affine points.

A restatement of the reference's elgamal/DistrElGamalSessionBasic.java with the plaintext group G^omega: u, A = u.expProd(e),
B' = A^r and B_l = f_l.expProd(e) are elements of G^omega (a list of omega elements of G, component 0 first); g, the public key
shares y_l, the secret, the randomizer r, the reply k_x and the challenge stay in G / Z_q (:524-540, :595-598, :642-727).  The
factors are firstComponents.exp(-x_j / c) over all omega components (elgamal/DistrElGamalSession.java:365-389).

Written against the group adapter K of oracle/pyref_proofs.py (ModPAdapter over oracle/pyref.py, ECAdapter over
oracle/pyref_ec.py), so the same statements cover modular groups and curves.  A width-omega array is a list of omega lists."""
from oracle import pyref_proofs as P


def prod_factor(q: int, k: int) -> int:
    """c = (prod over primes p <= k of the largest power of p not exceeding k)^2 mod q   (:318-344)."""
    res = 1
    for prime in range(2, k + 1):
        if any(prime % d == 0 for d in range(2, prime)):
            continue
        a = prime
        while a * prime <= k:
            a *= prime
        res *= a
    return res * res % q


def lagrange_integers(q: int, correct, k: int, threshold: int):
    """The modified Lagrange coefficients c * prod_{l != i} l / (l - i) over the first `threshold` correct parties, each as the
    integer of smallest absolute value in its class mod q (:358-452)."""
    idx = [l for l in range(1, k + 1) if correct[l]][:threshold]
    if len(idx) < threshold:
        raise ValueError("attempting to combine too few decryption factors")
    c = prod_factor(q, k)
    out = []
    for i in idx:
        res = c
        for l in idx:
            if l != i:
                res = res * l % q * pow(l - i, -1, q) % q
        out.append(res - q if q - res < res else res)
    return out


def decryption_factors(K, u, x_j: int, k: int):
    """f_j = u^(-x_j / c) in every component (DistrElGamalSession.java:365-389)."""
    ex = (-x_j) * pow(prod_factor(K.q, k), -1, K.q) % K.q
    return [K.exp_scalar(uc, ex) for uc in u]


def combine_decryption_factors(K, factors, correct, k: int, threshold: int):
    """prod_t f_{j_t}^(lambda_t) in every component (:465-503); factors[l] = the omega arrays of party l (entry 0 unused)."""
    idx = [l for l in range(1, k + 1) if correct[l]][:threshold]
    ints = lagrange_integers(K.q, correct, k, threshold)
    width = len(factors[idx[0]])
    out = []
    for c in range(width):
        acc = None
        for l, lam in zip(idx, ints):
            term = K.exp_scalar(factors[l][c], lam % K.q)
            acc = term if acc is None else K.mul_arrays(acc, term)
        out.append(acc)
    return out


def plaintexts(K, v, combined):
    """second components times the combined factors (DistrElGamalSession.java:536-538)."""
    return [K.mul_arrays(vc, fc) for vc, fc in zip(v, combined)]


class WideDistrElGamalSessionBasic:
    """One instance per party j; prover of j and verifier of every l.  g: generator of G; rand: a tape (ring_element())."""

    def __init__(self, K, g, j: int, k: int, threshold: int, rand=None):
        self.K, self.q, self.g, self.j, self.k, self.threshold, self.rand = K, K.q, g, j, k, threshold, rand
        self.inverseFactor = pow(prod_factor(K.q, k), -1, K.q)
        self.yp, self.Bp, self.B, self.k_x = {}, {}, {}, {}
        self.bad_reply = set()

    def setInstance(self, u, y, f):
        self.u, self.y, self.f, self.width = u, y, f, len(u)

    def setBatchVector(self, e):
        self.e = list(e)

    def _expprod(self, arrays):
        return [self.K.exp_prod(a, self.e) for a in arrays]

    def batchInput(self):
        self.A = self._expprod(self.u)                                         # :524-526

    def commit(self, x: int):
        K = self.K
        self.x = x % self.q
        self.r = self.rand.ring_element()
        self.yp[self.j] = K.exp(self.g, self.r)                                # y' = g^r        :536
        self.Bp[self.j] = tuple(K.exp(Ac, self.r) for Ac in self.A)            # B' = A^r in G^omega  :537
        return self.yp[self.j], self.Bp[self.j]

    def reply(self, v: int) -> int:
        self.k_x[self.j] = ((-self.x) * self.inverseFactor % self.q * (v % self.q) + self.r) % self.q      # :595-598
        return self.k_x[self.j]

    def setCommitment(self, l: int, yp, Bp):
        self.yp[l], self.Bp[l] = yp, tuple(Bp)

    def setReply(self, l: int, k_x: int):
        if not 0 <= k_x < self.q:                                              # pRing.toElement fails  :606-613
            self.k_x[l] = 0
            self.bad_reply.add(l)
        else:
            self.k_x[l] = k_x
            self.bad_reply.discard(l)

    def batch(self, l: int):
        self.B[l] = self._expprod(self.f[l])                                   # :707-709

    def _check(self, y, yexp, yp, B, Bp, v, k_x) -> bool:
        K = self.K
        ok = K.mul(K.exp(K.inv(y), yexp), yp) == K.exp(self.g, k_x)
        for Bc, Bpc, Ac in zip(B, Bp, self.A):
            ok = ok and K.mul(K.exp(Bc, v), Bpc) == K.exp(Ac, k_x)
        return ok

    def verify(self, l: int, v: int) -> bool:                                  # :718-727
        if l in self.bad_reply:
            return False
        return self._check(self.y[l], self.inverseFactor * (v % self.q) % self.q, self.yp[l], self.B[l], self.Bp[l], v % self.q, self.k_x[l])

    def combine(self, correct, combinedy, combinedf):                          # :642-678
        K = self.K
        idx = [l for l in range(1, self.k + 1) if correct[l]][:self.threshold]
        ints = lagrange_integers(self.q, correct, self.k, self.threshold)
        self.combinedyp, self.combinedBp, self.combinedk_x = None, [None] * self.width, 0
        for l, lam in zip(idx, ints):
            ex = lam % self.q
            t = K.exp(self.yp[l], ex)
            self.combinedyp = t if self.combinedyp is None else K.mul(self.combinedyp, t)
            for c in range(self.width):
                t = K.exp(self.Bp[l][c], ex)
                self.combinedBp[c] = t if self.combinedBp[c] is None else K.mul(self.combinedBp[c], t)
            self.combinedk_x = (self.combinedk_x + self.k_x[l] * ex) % self.q
        self.combinedy, self.combinedf = combinedy, combinedf

    def batchCombined(self):
        self.combinedB = self._expprod(self.combinedf)                         # :683-685

    def verifyCombined(self, v: int) -> bool:                                  # :693-700
        return self._check(self.combinedy, v % self.q, self.combinedyp, self.combinedB, self.combinedBp, v % self.q, self.combinedk_x)


def adapter_modp(p: int, q: int):
    return P.ModPAdapter(p, q)


def adapter_curve(curve):
    return P.ECAdapter(curve)


def run_session(K, g, u, y, xs, f, e, chal, k: int, threshold: int, tape_of):
    """Every party commits and replies (tape_of(j): party j's random tape); returns the transcript the verifier of party 1 sees:
    {"commit": {j: (y', B')}, "reply": {j: k_x}, "verifier": the session object with everything set}."""
    ver = WideDistrElGamalSessionBasic(K, g, 1, k, threshold)
    ver.setInstance(u, y, f)
    ver.setBatchVector(e)
    ver.batchInput()
    out = {"commit": {}, "reply": {}, "verifier": ver}
    for j in range(1, k + 1):
        pr = WideDistrElGamalSessionBasic(K, g, j, k, threshold, rand=tape_of(j))
        pr.setInstance(u, y, f)
        pr.setBatchVector(e)
        pr.batchInput()
        out["commit"][j] = pr.commit(xs[j])
        out["reply"][j] = pr.reply(chal)
        ver.setCommitment(j, *out["commit"][j])
        ver.setReply(j, out["reply"][j])
        ver.batch(j)
    return out
