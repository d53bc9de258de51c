"""Catalogue for the equality of curve points (csrc/ec_kernels.h: k_ec_equal, behind vmn_garray_equals -- a verifier's whole
verdict on check (B) of the shuffle proofs over a curve): the pairs of group elements on which a wrong comparison differs
from a right one, the representations in which one group element reaches the kernel, and the chains of pointwise operations
that leave the rows it really sees.  Shared by tests/test_gpu_ec_equality.py (the kernel's verdict on every pair in every
pair of representations) and tests/test_ec_equality_catalogue.py (the catalogue holds what it claims; no GPU).

The two sides of a comparison are Jacobian rows (X, Y, Z, flag) out of different chains of kernels: their Z are unrelated,
their coordinates are lazy (a small multiple of p above the residue) and either may carry the infinity flag.  Equal means
X1 Z2^2 = X2 Z1^2 and Y1 Z2^3 = Y2 Z1^3 mod p, or both flags.

A DRESS is a way to obtain a device row of a target T through the public array API:
    plain     import T                                             Z = 1, canonical coordinates
    negated   import -T, inv()                                     Z = 1, Y = 256p - (p - y): the lazy value of k_ec_neg
    sum       import A = T - D and D (a base point), A.mul(D)      the general addition: Z = 2 (x_D - x_A), lazy X and Y
    doubled   import H = ((n + 1) / 2) T, H.mul(H)                 the equal-points branch of the addition: Z = 2 y_H
    scaled    import U = T / k, U.exp(ring array of the k)         a row of k_ec_mulvar
and the identity in its own form in each: imported, imported and negated, A + (-A), the identity doubled, a point raised to
0.  A side of a comparison is a gather (permute(idx), idx of any length and with repeats) from a POOL: the array of every
target in one dress.  The gather moves the uint4 chunks of a row as they are (light_kernels.h: k_gather), so the dress
survives it.

Reference cost: every array is built from a few dozen points per curve (16 seeded multiples of G as the background, the
edge points, the identity and their partners), so the affine Python reference is evaluated once per point, not per row.

The model at the end -- same() over integer rows, its mutants, rows() of a target in a dress -- is what the catalogue test
uses to prove that every pair is needed: the mutants break the model, never a kernel."""
import functools
from collections import namedtuple

import ec_wire_edges as we
from oracle import pyref
from oracle.pyref_prg import sqrt_mod

CURVES = we.CURVES
NAMES = we.NAMES
DRESSES = ("plain", "negated", "sum", "doubled", "scaled")
COMBOS = [(dl, dr) for dl in DRESSES for dr in DRESSES]
NBASE = 16
N = 257                                                   # elements of a compared array: one more than a workgroup
POSITIONS = (0, 63, 64, 255, 256)                         # first, last of a wave, first of the next, last of a block, the next block
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
IDENTITY = "O"

Pair = namedtuple("Pair", "left right equal")             # labels of the pool, the expected verdict
# how a target is made in each dress: the points to import (and the exponent of `scaled`)
Recipe = namedtuple("Recipe", "neg A D H U k")


def _seed(name, *parts):
    return b"ec-equality/" + name.encode() + b"/" + b"/".join(str(p).encode() for p in parts)


def same_y_partner(c, P):
    """A point with the y of P and another x, or None: the other roots of x^3 + a x + b - y^2, which has the root x0, are
    those of x^2 + x0 x + (x0^2 + a): (-x0 +- sqrt(-3 x0^2 - 4a)) / 2."""
    x0, y = P
    r = sqrt_mod((-3 * x0 * x0 - 4 * c.a) % c.p, c.p)
    if r is None:
        return None
    x1 = (-x0 + r) * pow(2, -1, c.p) % c.p
    return None if x1 == x0 else (x1, y)


_cases = {}


def cases(name):
    """Everything about a curve, computed once: dict(c, base, targets, pool, recipes, pairs, equal, unequal, partners)."""
    if name in _cases:
        return _cases[name]
    f = we.facts(name)
    c = f["c"]
    ks = [1 + k % (c.n - 1) for k in pyref.stream_ints(_seed(name, "base"), NBASE, c.n)]
    base = [c.mul(k, c.g) for k in ks]
    assert len(set(base)) == NBASE
    # -- the targets: what an equal pair is made of
    targets = [("base#%d" % i, P) for i, P in enumerate(base)] + [("G", c.g), ("min-x", f["min_x"]), ("max-x", f["max_x"])]
    if f["zero_x"] and f["zero_x"] != f["min_x"]:             # (0, sqrt b) is the point of smallest x wherever it exists
        targets.append(("x=0", f["zero_x"]))
    targets.append((IDENTITY, None))
    pool = dict(targets)
    finite = [label for label, P in targets if P is not None]
    pairs = [Pair(label, label, True) for label, _ in targets]
    # -- (T, -T): the same x
    for label in finite:
        pool["-" + label] = c.neg(pool[label])
        pairs.append(Pair(label, "-" + label, False))
    # -- (T, T'): the same y, another x -- the first two base points that have such a partner
    partners = []
    for i, P in enumerate(base):
        Q = same_y_partner(c, P)
        if Q is not None and len(partners) < 2:
            partners.append("base#%d" % i)
            pool["base#%d'" % i] = Q
            pairs.append(Pair("base#%d" % i, "base#%d'" % i, False))
    assert partners, name
    # -- the identity on either side: against the edge points, G, and base#0, whose coordinates the model puts under the flag
    for label in ["base#0", "G", "min-x", "max-x"] + (["x=0"] if "x=0" in pool else []):
        pairs.append(Pair(label, IDENTITY, False))
        pairs.append(Pair(IDENTITY, label, False))
    # -- (T, T + G): plainly another point
    for label in ("base#0", "base#1", "G", "min-x"):
        pool[label + "+G"] = c.add(pool[label], c.g)
        pairs.append(Pair(label, label + "+G", False))
    assert len(set(pool.values())) == len(pool), name         # no two labels name one point
    # -- how to dress every point of the pool
    recipes = {}
    half = (c.n + 1) // 2
    for j, (label, T) in enumerate(pool.items()):
        if T is None:
            recipes[label] = Recipe(None, base[0], c.neg(base[0]), None, base[1], 0)
        elif label.startswith("-"):                           # the dress of -T is the negated dress of T
            r = recipes[label[1:]]
            recipes[label] = Recipe(c.neg(r.neg), c.neg(r.A), c.neg(r.D), c.neg(r.H), c.neg(r.U), r.k)
        else:
            k = 2 + pyref.stream_ints(_seed(name, "k", label), 1, c.n - 3)[0]
            for d in range(NBASE):                            # D with T - D neither the identity nor +-D: the general addition
                D = base[(j + d) % NBASE]
                A = c.add(T, c.neg(D))
                if A is not None and A[0] != D[0]:
                    break
            else:
                raise AssertionError("no D for " + label)
            # (scalar_mul: the catalogue test proves H + H = T and k U = T with the oracle's own arithmetic)
            recipes[label] = Recipe(c.neg(T), A, D, scalar_mul(c, half, T), scalar_mul(c, pow(k, -1, c.n), T), k)
    out = dict(c=c, name=name, base=base, targets=targets, pool=pool, labels=list(pool), recipes=recipes, pairs=pairs,
               equal=[p for p in pairs if p.equal], unequal=[p for p in pairs if not p.equal], partners=partners)
    _cases[name] = out
    return out


# ---- where the pairs sit in the compared arrays -------------------------------------------------------------------------
def background(n=N):
    """The labels of an array of n background elements: base[i % 16]."""
    return ["base#%d" % (i % NBASE) for i in range(n)]


def equal_layout(name, combo):
    """The labels of the 257 elements of the equal-pairs call of the dress combination number `combo`: the background, which
    holds every base point at 16 positions or more, and the other targets at the positions of POSITIONS (which of them turns
    with the combination) and in the middle of the waves between."""
    labels = background()
    others = [label for label, _ in cases(name)["targets"] if not label.startswith("base#")]
    assert len(others) <= len(POSITIONS)
    for j, label in enumerate(others):
        labels[POSITIONS[(j + combo) % len(POSITIONS)]] = label
        labels[97 + 32 * j] = label
    return labels


def unequal_calls(name):
    """[(pair, left dress, right dress, position)]: one call per unequal pair and dress combination, the position of the pair
    turning through POSITIONS from combination to combination and its start from pair to pair."""
    out = []
    for i, pair in enumerate(cases(name)["unequal"]):
        for j, (dl, dr) in enumerate(COMBOS):
            out.append((pair, dl, dr, POSITIONS[(i + j) % len(POSITIONS)]))
    return out


def sides(pair, at, n=N):
    """(left labels, right labels): the background on both sides, the pair at position `at`."""
    left, right = background(n), background(n)
    left[at], right[at] = pair.left, pair.right
    return left, right


# ---- chains --------------------------------------------------------------------------------------------------------------
CHAIN_LEN, CHAIN_N, CHAINS, CHAIN_MULS = 12, 70, 4, 3
OPS = ("mul-other", "mul-self", "inv", "exp-small", "exp-array", "exp2", "permute", "shift-push")
# what an operation costs the reference in full-size scalar multiplications per element
OP_COST = {"exp-array": 1, "exp2": 2}


def chain_inputs(name):
    """The 70 points a chain starts from: the base points, G, -G, the identity and the edge-x points with both signs of y,
    repeated so that G, -G and the identity meet each other and themselves under the seeded gathers."""
    k = cases(name)
    c, pool = k["c"], k["pool"]
    special = [c.g, c.neg(c.g), None] + [pool[e] for e in ("min-x", "-min-x", "max-x", "-max-x", "x=0", "-x=0") if e in pool]
    pts = list(k["base"]) + special
    return [pts[i % len(pts)] for i in range(CHAIN_N)]


def _exponents(name, tag, c):
    es = pyref.stream_ints(_seed(name, "chain-e", tag), CHAIN_N, c.n)
    for i, e in enumerate((0, 1, c.n - 1, 2, c.n - 2)):
        es[(7 * i + 3) % CHAIN_N] = e
    return es


def chain_program(name, j):
    """The 12 steps of chain j of a curve: [(op, argument)], seeded; the argument is what the step needs beyond the running
    array -- the index of the earlier state it is multiplied with (0: the inputs), a small or a full exponent, a list of
    exponents, a gather list, a pushed point.  At most CHAIN_MULS full-size scalar multiplications per element; the first
    steps of the four chains of a curve go through OPS in turn, so every operation runs on every curve."""
    k = cases(name)
    c = k["c"]
    draws = pyref.stream_ints(_seed(name, "chain", j), 4 * CHAIN_LEN, 1 << 32)
    steps, cost = [], 0
    forced = [OPS[(2 * j) % len(OPS)], OPS[(2 * j + 1) % len(OPS)]]
    for s in range(CHAIN_LEN):
        op = forced[s] if s < len(forced) else OPS[draws[4 * s] % len(OPS)]
        if cost + OP_COST.get(op, 0) > CHAIN_MULS:            # the reference's budget is spent: a light step instead
            op = ("mul-other", "mul-self", "inv", "exp-small", "permute", "shift-push")[draws[4 * s + 1] % 6]
        cost += OP_COST.get(op, 0)
        tag = "%d/%d" % (j, s)
        if op == "mul-other":
            arg = draws[4 * s + 2] % (s + 1)
        elif op == "exp-small":
            arg = 2 + draws[4 * s + 2] % 14
        elif op == "exp-array":
            arg = _exponents(name, tag, c)
        elif op == "exp2":                                    # self^e other^f: (e, index of the earlier state, f)
            arg = (pyref.stream_ints(_seed(name, "chain-e2", tag), 1, c.n)[0], draws[4 * s + 2] % (s + 1), _exponents(name, tag + "/f", c))
        elif op == "permute":                                 # a gather: most entries moved, a few repeated
            arg = [v % CHAIN_N for v in pyref.stream_ints(_seed(name, "chain-perm", tag), CHAIN_N, 1 << 32)]
        elif op == "shift-push":
            arg = k["pool"][("G", "-G", IDENTITY, "max-x")[draws[4 * s + 2] % 4]]
        else:
            arg = None
        steps.append((op, arg))
    return steps


def scalar_mul(c, k, P):
    """k P in Python integers, as oracle/pyref_ec.Curve.mul gives it (tests/test_ec_equality_catalogue.py holds the two
    against each other): the same double-and-add over the bits of k mod n, with the running sum in Jacobian coordinates and
    P affine, so that one inversion at the end replaces one per step -- the chains need 200 full-size products per curve."""
    k %= c.n
    if P is None or k == 0:
        return None
    p, a = c.p, c.a
    x2, y2 = P
    acc = None                                                # (X, Y, Z), Z != 0, or None: the identity
    for bit in bin(k)[2:]:
        if acc is not None:                                   # double (no point of order 2: every curve here has cofactor 1)
            X, Y, Z = acc
            YY = Y * Y % p
            S = 4 * X * YY % p
            M = (3 * X * X + a * pow(Z, 4, p)) % p
            X3 = (M * M - 2 * S) % p
            acc = (X3, (M * (S - X3) - 8 * YY * YY) % p, 2 * Y * Z % p)
        if bit == "1":
            if acc is None:
                acc = (x2, y2, 1)
                continue
            X, Y, Z = acc
            ZZ = Z * Z % p
            H = (x2 * ZZ - X) % p
            r = (y2 * ZZ * Z - Y) % p
            if H == 0:                                        # acc = +-P: only where k has run through a multiple of n +- 1
                acc = jac_of(c, c.add(affine_of(c, acc), P))
                continue
            HH = H * H % p
            V = X * HH % p
            X3 = (r * r - HH * H - 2 * V) % p
            acc = (X3, (r * (V - X3) - Y * HH * H) % p, Z * H % p)
    return affine_of(c, acc)


def affine_of(c, J):
    if J is None:
        return None
    zi = pow(J[2], -1, c.p)
    return J[0] * zi * zi % c.p, J[1] * zi ** 3 % c.p


def jac_of(c, P):
    return None if P is None else (P[0], P[1], 1)


def chain_step_reference(c, states, op, arg):
    """The next state of a chain in affine Python points; `states` are the inputs and every state so far."""
    cur = states[-1]
    if op == "mul-other":
        return c.mul_arrays(cur, states[arg])
    if op == "mul-self":
        return [c.add(P, P) for P in cur]
    if op == "inv":
        return [c.neg(P) for P in cur]
    if op == "exp-small":
        return [c.mul(arg, P) for P in cur]
    if op == "exp-array":
        return [scalar_mul(c, e, P) for P, e in zip(cur, arg)]
    if op == "exp2":
        e, other, fs = arg
        return [c.add(scalar_mul(c, e, P), scalar_mul(c, f, Q)) for P, Q, f in zip(cur, states[other], fs)]
    if op == "permute":
        return [cur[i] for i in arg]
    if op == "shift-push":
        return [arg] + cur[:-1]
    raise KeyError(op)


def chain_reference(name, j):
    """Every state of chain j, the inputs first."""
    c = cases(name)["c"]
    states = [chain_inputs(name)]
    for op, arg in chain_program(name, j):
        states.append(chain_step_reference(c, states, op, arg))
    return states


# ---- the model ----------------------------------------------------------------------------------------------------------
X_ONLY, Y_ONLY, INF_EITHER, INF_IGNORED, ROWS, FIRST_WORKGROUP_ONLY = ("x-only", "y-only", "inf-either", "inf-ignored", "rows",
                                                                     "first-workgroup-only")
ROW_MUTANTS = (X_ONLY, Y_ONLY, INF_EITHER, INF_IGNORED, ROWS)
MUTANTS = ROW_MUTANTS + (FIRST_WORKGROUP_ONLY,)
WORKGROUP = 256


@functools.lru_cache(maxsize=None)
def same(p, P, Q, mutant=None):
    """Are the integer Jacobian rows P and Q = (X, Y, Z, flag) one group element?  Coordinates of any size (lazy values).
    `mutant` breaks the predicate in one of five ways."""
    if mutant == ROWS:                                        # a comparison of representations
        return P == Q
    if mutant != INF_IGNORED and (P[3] or Q[3]):
        return bool(P[3] or Q[3]) if mutant == INF_EITHER else bool(P[3] and Q[3])
    X1, Y1, Z1, _ = P
    X2, Y2, Z2, _ = Q
    x_eq = (X1 * Z2 * Z2 - X2 * Z1 * Z1) % p == 0
    y_eq = (Y1 * Z2 ** 3 - Y2 * Z1 ** 3) % p == 0
    if mutant == X_ONLY:
        return x_eq
    if mutant == Y_ONLY:
        return y_eq
    return x_eq and y_eq


def arrays_same(p, left, right, mutant=None):
    """The verdict of one call on two lists of rows.  FIRST_WORKGROUP_ONLY never looks at a position from 256 on."""
    if len(left) != len(right):
        return False
    upto = min(len(left), WORKGROUP) if mutant == FIRST_WORKGROUP_ONLY else len(left)
    return all(same(p, P, Q, mutant if mutant in ROW_MUTANTS else None) for P, Q in zip(left[:upto], right[:upto]))


_rows = {}


def row(name, label, dress):
    """The model's row of a point of the pool in a dress: (x Z^2, y Z^3, Z) for a seeded Z (1 where the dress leaves Z = 1),
    multiples of p added within the bounds the header of ec_kernels.h states (coordinates below 81p, a negated Y 256p - Y,
    Z below 546p).  The identity is the row of a base point under a raised flag -- base#0 in the plain dress, base#1 in the
    negated one and so on: the coordinates under a flag are nonzero and say nothing, not even that two identities agree.
    (That is the contract, and harsher than today's rows: every identity the array kernels write has Z = 0 mod p under its
    flag -- pt_set_inf, or a doubling of it -- so a comparison that ignored the flag would meet 0 = 0 there.)"""
    key = (name, label, dress)
    if key in _rows:
        return _rows[key]
    k = cases(name)
    p = k["c"].p
    T = k["pool"][label]
    if T is None:
        X, Y, Z, _ = row(name, "base#%d" % DRESSES.index(dress), dress)
        out = (X, Y, Z, 1)
    elif dress == "plain":
        out = (T[0], T[1], 1, 0)
    elif dress == "negated":
        out = (T[0], 256 * p - (p - T[1]), 1, 0)
    else:
        z, kx, ky, kz = pyref.stream_ints(_seed(name, "row", label, dress), 4, p - 1)
        z += 1
        out = (T[0] * z * z % p + kx % 80 * p, T[1] * z ** 3 % p + ky % 80 * p, z + kz % 545 * p, 0)
    assert out[0] % p and out[1] % p and out[2] % p or T[0] == 0
    _rows[key] = out
    return out


def rows(name, labels, dress):
    return [row(name, label, dress) for label in labels]
