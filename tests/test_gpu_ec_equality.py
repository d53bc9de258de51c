"""GPU suite: the equality of curve points (csrc/ec_kernels.h: k_ec_equal behind vmn_garray_equals -- over a curve, a
verifier's whole verdict on check (B) of the shuffle proofs) on every representation of a point, on one curve per kernel
instantiation: the pairs of tests/ec_equality_cases.py -- a point and itself, its negative (the same x), a point of the same
y, the identity on either side, plainly another point -- with each side in each of five dresses (imported, negated, a general
sum, a doubling, a scalar multiple: unrelated Z, lazy coordinates, the identity in five forms), the differing pair alone in
an array of 257 and at the lanes that begin and end a wave and a workgroup; and chains of twelve pointwise operations
without an export between them, whose last rows are exported, compared with the import of the reference, and compared with
that import after one negation.  Exact integers throughout: the expected points come from the oracle's affine arithmetic."""
import pytest

import ec_equality_cases as ec

pytestmark = pytest.mark.gpu


class Pools:
    """One curve: the group, and every point of the catalogue's pool in every dress -- five arrays, built once."""

    def __init__(self, vmn, gpu_ctx, name):
        self.name, self.k = name, ec.cases(name)
        self.c = self.k["c"]
        self.G = G = vmn.ECqPGroup(gpu_ctx, name)
        labels = self.k["labels"]
        self.index = {label: i for i, label in enumerate(labels)}
        rs = [self.k["recipes"][label] for label in labels]
        H = G.toElementArray([r.H for r in rs])
        self.pool = {
            "plain": G.toElementArray([self.k["pool"][label] for label in labels]),
            "negated": G.toElementArray([r.neg for r in rs]).inv(),
            "sum": G.toElementArray([r.A for r in rs]).mul(G.toElementArray([r.D for r in rs])),
            "doubled": H.mul(H),
            "scaled": G.toElementArray([r.U for r in rs]).exp(G.ringArray([r.k for r in rs])),
        }

    def side(self, dress, labels):
        """The array of the points `labels` in a dress: a gather from the pool, which moves rows as they are."""
        return self.pool[dress].permute([self.index[label] for label in labels])

    def points(self, labels):
        return [self.k["pool"][label] for label in labels]

    def close(self):
        self.pool.clear()
        self.G.close()


@pytest.fixture(scope="module", params=ec.NAMES)
def pools(request, vmn, gpu_ctx):
    p = Pools(vmn, gpu_ctx, request.param)
    yield p
    p.close()


def test_every_dress_exports_its_targets(pools):
    want = pools.points(pools.k["labels"])
    for dress in ec.DRESSES:
        assert pools.pool[dress].toInts() == want, dress
    # ... and a gather with repeats, longer than the pool, exports what it gathered
    labels = ec.equal_layout(pools.name, 0)
    assert pools.side("sum", labels).toInts() == pools.points(labels)


def test_equal_pairs_in_every_pair_of_dresses(pools):
    """One call per dress combination on 257 elements that hold every equal pair, the identity included: True, both ways
    round, and both sides export the targets -- the verdict is about the values a reader of the arrays would get."""
    for combo, (dl, dr) in enumerate(ec.COMBOS):
        labels = ec.equal_layout(pools.name, combo)
        want = pools.points(labels)
        L, R = pools.side(dl, labels), pools.side(dr, labels)
        assert L.equals(R) and R.equals(L), (dl, dr)
        assert L.toInts() == want and R.toInts() == want, (dl, dr)


def test_one_unequal_pair_among_257(pools):
    """One call per unequal pair and dress combination: the pair alone at position 0, 63, 64, 255 or 256, everything else
    equal -- so a False is that row's.  Every call must say False."""
    calls = ec.unequal_calls(pools.name)
    assert len(calls) == 25 * len(pools.k["unequal"]) >= 25 * 30
    wrong = []
    for pair, dl, dr, at in calls:
        left, right = ec.sides(pair, at)
        if pools.side(dl, left).equals(pools.side(dr, right)):
            wrong.append((pair.left, pair.right, dl, dr, at))
    assert not wrong, (len(wrong), wrong[:12])


@pytest.mark.parametrize("n", ec.SIZES)
def test_a_negated_point_first_and_last_in_arrays_around_a_wave_and_a_block(pools, n):
    """(T, -T) -- the pair that only the Y half of the comparison tells apart -- as the first and as the last of n elements,
    and at each of the positions 0, 63, 64, 255, 256 that n holds; the same arrays without it are equal."""
    pair = ec.Pair("base#3", "-base#3", False)
    for i, at in enumerate(sorted({0, n - 1} | {q for q in ec.POSITIONS if q < n})):
        dl, dr = ec.COMBOS[(7 * i + n) % len(ec.COMBOS)]
        left, right = ec.sides(pair, at, n)
        L, R = pools.side(dl, left), pools.side(dr, right)
        assert not L.equals(R) and not R.equals(L), (n, at, dl, dr)
        assert L.equals(pools.side(dr, left)) and pools.side(dl, right).equals(R), (n, at, dl, dr)


def test_sizes_that_differ_and_empty_arrays(pools):
    G = pools.G
    for n, m in ((64, 65), (256, 257), (1, 2), (0, 1)):
        A, B = pools.side("sum", ec.background(n)), pools.side("scaled", ec.background(m))
        assert not A.equals(B) and not B.equals(A), (n, m)
    assert G.toElementArray([]).equals(G.toElementArray([]))
    assert pools.side("doubled", []).equals(G.toElementArray([]))


def test_a_verdict_does_not_outlive_its_call(pools):
    """Every comparison of a context, of curve points and of ring elements alike, leaves its verdict in one flag word:
    unequal, equal, unequal in turn, with comparisons of ring arrays of either verdict between them."""
    G, c = pools.G, pools.c
    left, right = ec.sides(ec.Pair("G", "-G", False), 256)
    L, R, L2 = pools.side("sum", left), pools.side("negated", right), pools.side("doubled", left)
    es = list(range(1, 70))
    E, E2, F = G.ringArray(es), G.ringArray(es), G.ringArray(es[:-1] + [c.n - 1])
    for _ in range(2):
        assert not L.equals(R)
        assert E.equals(E2)
        assert L.equals(L2)
        assert not E.equals(F)
        assert L2.equals(L)
        assert not R.equals(L2)
        assert not E.equals(F)
        assert not L.equals(R)


@pytest.mark.parametrize("j", range(ec.CHAINS))
def test_chains_of_pointwise_operations_without_an_export(pools, j):
    """Twelve seeded operations on 70 points, each on the rows the one before left: the header of ec_kernels.h argues in
    comments that every formula accepts what every other leaves (coordinates below 81p, a negated Y below 256p, Z below
    546p).  At the end the rows export to the reference, equal its import, and differ from it once one element is negated."""
    G, c = pools.G, pools.c
    states = ec.chain_reference(pools.name, j)
    dev = [G.toElementArray(states[0])]
    for op, arg in ec.chain_program(pools.name, j):
        cur = dev[-1]
        if op == "mul-other":
            nxt = cur.mul(dev[arg])
        elif op == "mul-self":
            nxt = cur.mul(cur)
        elif op == "inv":
            nxt = cur.inv()
        elif op == "exp-small":
            nxt = cur.exp(arg)
        elif op == "exp-array":
            nxt = cur.exp(G.ringArray(arg))
        elif op == "exp2":
            nxt = cur.exp2(arg[0], dev[arg[1]], G.ringArray(arg[2]))
        elif op == "permute":
            nxt = cur.permute(arg)
        else:
            assert op == "shift-push"
            nxt = cur.shiftPush(arg)
        dev.append(nxt)
    want, got = states[-1], dev[-1]
    assert got.toInts() == want
    W = G.toElementArray(want)
    assert got.equals(W) and W.equals(got)
    at = next(i for i in range(5 * j, ec.CHAIN_N) if want[i] is not None)
    bad = list(want)
    bad[at] = c.neg(want[at])
    B = G.toElementArray(bad)
    assert not got.equals(B) and not B.equals(got), at
    assert dev[0].toInts() == states[0]                       # (no operation wrote into its operand)
