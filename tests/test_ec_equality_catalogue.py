"""The pairs of tests/ec_equality_cases.py are not vacuous: every target and every partner is the point it is called, the
ingredients of every dress reproduce the target under the oracle's affine arithmetic, the reference predicate gives the
expected verdict on every pair in every pair of dresses, and six mutants of the predicate (never of a kernel) -- X only, Y
only, either identity is enough, the identity flag ignored, rows instead of group elements, nothing beyond the first
workgroup -- are each caught on every curve.  No GPU: the kernel meets these pairs in tests/test_gpu_ec_equality.py."""
import pytest

import ec_equality_cases as ec
import ec_wire_edges as we

B_IS_A_SQUARE = {"P-192", "P-256", "P-384", "P-521", "prime239v1"}


@pytest.fixture(scope="module", params=ec.NAMES)
def k(request):
    return ec.cases(request.param)


def test_targets_and_partners_are_what_they_are_called(k):
    c, pool = k["c"], k["pool"]
    f = we.facts(k["name"])
    labels = [label for label, _ in k["targets"]]
    assert labels[:ec.NBASE] == ["base#%d" % i for i in range(ec.NBASE)] and labels[-1] == ec.IDENTITY
    assert labels[ec.NBASE:-1] == ["G", "min-x", "max-x"]     # (0, sqrt b), where b is a square, is the point of smallest x
    assert (pool["min-x"][0] == 0) == (k["name"] in B_IS_A_SQUARE) and f["zero_x"] in (None, pool["min-x"])
    assert all(c.on_curve(P) for P in pool.values()) and len(set(pool.values())) == len(pool)
    assert [label for label, P in pool.items() if P is None] == [ec.IDENTITY]
    assert pool["G"] == c.g and pool["min-x"] == f["min_x"] and pool["max-x"] == f["max_x"]
    # the pairs: every target with itself; every finite target with its negative; the partners; the identity; T + G
    assert [(p.left, p.right) for p in k["equal"]] == [(label, label) for label in labels]
    unequal = {(p.left, p.right) for p in k["unequal"]}
    assert len(unequal) == len(k["unequal"]) and all(pool[a] != pool[b] for a, b in unequal)
    for label in labels[:-1]:
        T, M = pool[label], pool["-" + label]
        assert (label, "-" + label) in unequal and M[0] == T[0] and M[1] == c.p - T[1] != T[1]
    assert 1 <= len(k["partners"]) <= 2
    for label in k["partners"]:
        T, Q = pool[label], pool[label + "'"]
        assert (label, label + "'") in unequal and Q[1] == T[1] and Q[0] != T[0] and c.on_curve(Q)
        assert ec.same_y_partner(c, Q)[0] in (T[0], (-T[0] - Q[0]) % c.p)       # the three roots of the cubic sum to 0
    assert {(a, b) for a, b in unequal if ec.IDENTITY in (a, b)} >= {("G", ec.IDENTITY), (ec.IDENTITY, "G"), ("base#0", ec.IDENTITY),
                                                                     (ec.IDENTITY, "base#0"), ("min-x", ec.IDENTITY), (ec.IDENTITY, "max-x")}
    for a, b in unequal:
        if b.endswith("+G"):
            assert a + "+G" == b and pool[b] == c.add(pool[a], c.g)
    assert sum(b.endswith("+G") for _, b in unequal) == 4
    assert set(pool) == {x for p in k["pairs"] for x in (p.left, p.right)}


def test_about_half_of_all_points_have_a_partner_of_the_same_y():
    """-3 x0^2 - 4a is a square for about half of the x0 -- and where a = 0 (secp224k1, secp256k1) for all of them, -3 being
    a square of both primes: the partners are omega x0, omega^2 x0 for the cube roots of unity."""
    for name in ec.NAMES:
        k = ec.cases(name)
        c = k["c"]
        have = [ec.same_y_partner(c, P) is not None for P in k["base"]]
        assert (sum(have) == ec.NBASE) if c.a == 0 else (2 <= sum(have) <= ec.NBASE - 2), (name, sum(have))
        assert (c.a == 0) == (name in ("secp224k1", "secp256k1"))


def test_dresses_reproduce_their_target(k):
    c = k["c"]
    for label, T in k["pool"].items():
        r = k["recipes"][label]
        assert all(c.on_curve(P) for P in (r.neg, r.A, r.D, r.H, r.U)), label
        assert c.neg(r.neg) == T and c.add(r.A, r.D) == T and c.add(r.H, r.H) == T, label
        if label.startswith("-"):                             # k (-U) = -(k U): the recipe of T, negated
            q = k["recipes"][label[1:]]
            assert r.U == c.neg(q.U) and r.k == q.k and T == c.neg(k["pool"][label[1:]]), label
        else:
            assert c.mul(r.k, r.U) == T, label
        if T is None:                                         # the identity's own forms: A + (-A), a doubled identity, a zeroth power
            assert r.neg is None and r.H is None and r.k == 0 and r.U is not None and r.A is not None and r.D == c.neg(r.A), label
        else:                                                 # the general addition, the equal-points branch, a real power
            assert r.A is not None and r.A[0] != r.D[0] and r.D in k["base"] + [c.neg(B) for B in k["base"]], label
            assert r.H is not None and r.H[1] != 0 and 2 <= r.k < c.n and r.U is not None, label


def test_model_rows_are_their_target_in_another_representation(k):
    c, p = k["c"], k["c"].p
    for label, T in k["pool"].items():
        seen = set()
        for dress in ec.DRESSES:
            X, Y, Z, flag = ec.row(k["name"], label, dress)
            assert flag == (T is None) and Z % p and X < 81 * p and Y < 256 * p and Z < 546 * p, (label, dress)
            if T is None:
                assert X % p and Y % p                      # nonzero coordinates under the flag
                continue
            zi = pow(Z, -1, p)
            assert (X * zi * zi % p, Y * zi ** 3 % p) == T, (label, dress)
            assert (Z == 1) == (dress in ("plain", "negated")), (label, dress)
            seen.add((X, Y, Z))
        assert T is None or len(seen) == len(ec.DRESSES)       # five representations of one point
    assert ec.row(k["name"], "G", "negated")[1] > 255 * p


def test_same_gives_the_expected_verdict_on_every_pair_in_every_dress_combination(k):
    name, p = k["name"], k["c"].p
    for pair in k["pairs"]:
        for dl, dr in ec.COMBOS:
            assert ec.same(p, ec.row(name, pair.left, dl), ec.row(name, pair.right, dr)) == pair.equal, (pair, dl, dr)


def caught(k, mutant):
    name, p = k["name"], k["c"].p
    return [(pair, dl, dr) for pair in k["pairs"] for dl, dr in ec.COMBOS
            if ec.same(p, ec.row(name, pair.left, dl), ec.row(name, pair.right, dr), mutant) != pair.equal]


def test_every_mutant_of_the_predicate_is_caught(k):
    pool = k["pool"]
    got = {m: caught(k, m) for m in ec.ROW_MUTANTS}
    assert all(got.values()), [m for m in got if not got[m]]
    # and by the rows that are there for it
    negatives = {(p, dl, dr) for p in k["unequal"] if p.right == "-" + p.left for dl, dr in ec.COMBOS}
    assert set(got[ec.X_ONLY]) == negatives                                   # P = -P, and nothing else
    assert {p for p, _, _ in got[ec.Y_ONLY]} == {p for p in k["unequal"] if p.right == p.left + "'"}
    assert {p for p, _, _ in got[ec.INF_EITHER]} == {p for p in k["unequal"] if ec.IDENTITY in (p.left, p.right)}
    ignored = {p for p, _, _ in got[ec.INF_IGNORED]}
    assert ec.Pair(ec.IDENTITY, ec.IDENTITY, True) in ignored                 # two identities over different coordinates
    assert {ec.Pair("base#0", ec.IDENTITY, False), ec.Pair(ec.IDENTITY, "base#0", False)} <= ignored     # a point under the flag
    assert all(ec.IDENTITY in (p.left, p.right) for p in ignored)
    # a comparison of rows is right on every unequal pair, and on an equal pair only where both sides wear one dress
    assert set(got[ec.ROWS]) == {(p, dl, dr) for p in k["equal"] for dl, dr in ec.COMBOS if dl != dr}
    assert pool[ec.IDENTITY] is None


def test_gpu_layouts_hold_every_pair_and_catch_the_workgroup_mutant(k):
    name, p = k["name"], k["c"].p
    targets = [label for label, _ in k["targets"]]
    for combo in range(len(ec.COMBOS)):
        labels = ec.equal_layout(name, combo)
        assert len(labels) == ec.N and set(labels) == set(targets)
        dl, dr = ec.COMBOS[combo]
        assert ec.arrays_same(p, ec.rows(name, labels, dl), ec.rows(name, labels, dr))
    # every target that is no base point sits at every position of POSITIONS in some combination
    for label in targets[ec.NBASE:]:
        assert {at for combo in range(len(ec.COMBOS)) for at in ec.POSITIONS if ec.equal_layout(name, combo)[at] == label} == set(ec.POSITIONS)
    calls = ec.unequal_calls(name)
    assert len(calls) == len(k["unequal"]) * len(ec.COMBOS) and {at for _, _, _, at in calls} == set(ec.POSITIONS)
    beyond = 0
    for pair, dl, dr, at in calls:
        left, right = ec.sides(pair, at)
        assert [i for i in range(ec.N) if left[i] != right[i]] == [at] and (left[at], right[at]) == (pair.left, pair.right)
        L, R = ec.rows(name, left, dl), ec.rows(name, right, dr)
        assert not ec.arrays_same(p, L, R)
        assert ec.arrays_same(p, L, R, ec.FIRST_WORKGROUP_ONLY) == (at >= ec.WORKGROUP)
        beyond += at >= ec.WORKGROUP
    assert beyond >= len(calls) // len(ec.POSITIONS)          # the rows that catch it: a fifth of the calls
    # every pair meets every position, and so does every dress combination
    for pair in k["unequal"]:
        assert {at for q, _, _, at in calls if q == pair} == set(ec.POSITIONS)
    for combo in ec.COMBOS:
        assert {at for _, dl, dr, at in calls if (dl, dr) == combo} == set(ec.POSITIONS)
    # the sizes of the position test: first and last element, around a wave and a block
    for n in ec.SIZES:
        for at in {0, n - 1}:
            left, right = ec.sides(ec.Pair("G", "-G", False), at, n)
            L, R = ec.rows(name, left, "sum"), ec.rows(name, right, "scaled")
            assert not ec.arrays_same(p, L, R) and ec.arrays_same(p, L, L)
            assert ec.arrays_same(p, L, R, ec.FIRST_WORKGROUP_ONLY) == (at >= ec.WORKGROUP)
            assert ec.arrays_same(p, L, R, ec.X_ONLY)
    assert not ec.arrays_same(p, ec.rows(name, ec.background(64), "plain"), ec.rows(name, ec.background(65), "plain"))
    assert ec.arrays_same(p, [], [])


def test_the_chains_scalar_multiplication_is_the_oracles(k):
    c = k["c"]
    es = [0, 1, 2, 3, c.n - 1, c.n, c.n + 1, (c.n + 1) // 2] + ec.pyref.stream_ints(b"ec-equality/scalar-mul", 2, c.n)
    for P in (k["pool"]["-G"], k["pool"]["max-x"], None):
        for e in es:
            assert ec.scalar_mul(c, e, P) == c.mul(e, P), (e, P)


def test_chain_programs():
    """Twelve steps, at most three full-size scalar multiplications per element, every operation on every curve, and inputs
    that hold what the issue names; the reference of one chain on the smallest curve ends in points of the curve."""
    for name in ec.NAMES:
        k = ec.cases(name)
        c = k["c"]
        inputs = ec.chain_inputs(name)
        assert len(inputs) == ec.CHAIN_N and set(k["base"]) | {c.g, c.neg(c.g), None, k["pool"]["min-x"], k["pool"]["max-x"]} <= set(inputs)
        seen = set()
        for j in range(ec.CHAINS):
            prog = ec.chain_program(name, j)
            assert len(prog) == ec.CHAIN_LEN and prog == ec.chain_program(name, j)
            assert sum(ec.OP_COST.get(op, 0) for op, _ in prog) <= ec.CHAIN_MULS
            for s, (op, arg) in enumerate(prog):
                if op == "mul-other":
                    assert 0 <= arg <= s
                elif op == "exp-small":
                    assert 2 <= arg < 16
                elif op in ("exp-array", "exp2"):
                    es = arg if op == "exp-array" else arg[2]
                    assert len(es) == ec.CHAIN_N and {0, 1, c.n - 1} <= set(es) and all(0 <= e < c.n for e in es)
                    assert op == "exp-array" or (0 <= arg[1] <= s and 0 <= arg[0] < c.n)
                elif op == "permute":
                    assert len(arg) == ec.CHAIN_N and all(0 <= i < ec.CHAIN_N for i in arg) and len(set(arg)) < ec.CHAIN_N
                elif op == "shift-push":
                    assert c.on_curve(arg)
            seen |= {op for op, _ in prog}
        assert seen == set(ec.OPS), name
    states = ec.chain_reference("P-192", 2)
    c = ec.cases("P-192")["c"]
    assert len(states) == ec.CHAIN_LEN + 1 and all(len(s) == ec.CHAIN_N and all(c.on_curve(P) for P in s) for s in states)
    assert len(set(states[-1])) > ec.CHAIN_N // 2
