"""GPU suite: the light modular layer (csrc/modp_kernels.h: mod_add, mod_neg, sub_full, canonicalize, normalize,
limbs_from_be and the range check of k_import_be; k_words_maxbits of csrc/light_kernels.h) at its carry and borrow edges,
in every built geometry and under five ring moduli each -- against Python integers (%, pow, int.bit_length), by exact
equality.

The operands come from tests/ring_edges.py.  Arrays are held in Montgomery form, so every pair of the catalogue is fed
twice: as it stands, and as the pair whose DEVICE form is (a, b) -- ring_edges.montgomery_preimages() -- so that the
all-ones and all-zero shares are what the add and the negation really find in their registers."""
import math

import pytest

import ring_edges as re_
from test_gpu_geometry import force, restore
from oracle import pyref

pytestmark = pytest.mark.gpu

CASES = [(geo.id, name) for geo in re_.GEOMETRIES for name in re_.moduli(geo)]
CURVES = ["P-256", "P-384", "P-521", "secp256k1"]


class Case:
    """One geometry and ring modulus: the group (p = 2^bits - 1: the geometry follows the bit length of p, Montgomery
    arithmetic needs an odd modulus only), the catalogue's operands and their arrays on the device."""

    def __init__(self, vmn, gpu_ctx, geo, name):
        self.vmn, self.ctx, self.geo, self.name = vmn, gpu_ctx, geo, name
        self.p = (1 << geo.bits) - 1
        self.q = re_.modulus(geo, name)
        self.G = vmn.ModPGroup(gpu_ctx, self.p, self.q, 3, nbytes=geo.bits // 8)
        plain = re_.catalogue(self.q, geo.bits)
        # the preimages first, the pairs themselves after them: the array ends in (q - 1, q - 1)
        pairs = re_.montgomery_preimages(plain, self.q, geo.rows) + plain
        self.n_pre = len(plain)
        self.a = [a for a, _ in pairs]
        self.b = [b for _, b in pairs]
        self.A = self.G.ringArray(self.a)
        self.B = self.G.ringArray(self.b)
        self.rnd = pyref.stream_ints(b"ring-edges/v/%s/%s" % (geo.id.encode(), name.encode()), 4, self.q)

    def pre(self, x, modulus=None):
        """The value whose device form is x (x / R)."""
        m = modulus or self.q
        return x * pow(1 << (re_.LIMB * self.geo.rows), -1, m) % m

    def ring(self, values):
        return self.G.ringArray(values)

    def same(self, arr, want):
        """The array holds exactly `want`: by its export, and row for row on the device (a non-canonical row -- q for 0 --
        exports like the canonical one; the comparison of the rows tells them apart)."""
        assert arr.toInts() == want
        assert arr.equals(self.ring(want))

    def close(self):
        self.A.free()
        self.B.free()
        self.G.close()


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def case(request, vmn, gpu_ctx):
    """Module-scoped and parametrised: every test of a (geometry, modulus) runs on one group, created once and closed after
    them; where the geometry is a choice by size, the thresholds that force it hold for those tests and the defaults are
    back afterwards."""
    geo = re_.GEOMETRY[request.param[0]]
    if geo.force:
        force(gpu_ctx, geo.force)
    c = None
    try:
        c = Case(vmn, gpu_ctx, geo, request.param[1])
        yield c
    finally:
        if c is not None:
            c.close()
        if geo.force:
            restore(gpu_ctx)


# ---- element-wise -----------------------------------------------------------------------------------------------------
def test_add_and_neg(case):
    q, a, b = case.q, case.a, case.b
    case.same(case.A.add(case.B), [(x + y) % q for x, y in zip(a, b)])
    case.same(case.B.add(case.A), [(x + y) % q for x, y in zip(a, b)])
    nA, nB = case.A.neg(), case.B.neg()
    case.same(nA, [-x % q for x in a])
    case.same(nB, [-y % q for y in b])
    case.same(case.A.add(nA), [0] * len(a))
    case.same(nB.add(case.B), [0] * len(b))
    assert case.ring([0, 1, q - 1]).neg().toInts() == [0, q - 1, 1]
    case.same(case.A.add(case.A), [2 * x % q for x in a])


def test_mul(case):
    q, a, b = case.q, case.a, case.b
    case.same(case.A.mul(case.B), [x * y % q for x, y in zip(a, b)])


def test_mul_add_by_small_scalars(case):
    q, a, b = case.q, case.a, case.b
    for v in (0, 1, 2):
        case.same(case.A.mulAdd(v, case.B), [(x * v + y) % q for x, y in zip(a, b)])
        case.same(case.A.mulAdd(v, None), [x * v % q for x in a])


def test_mul_add_by_large_scalars(case):
    """v = q - 1, a random value, and the v whose device form is 1: the product is then the other operand's row as it is,
    and the sum that follows is the catalogue's own pair."""
    q, a, b, k = case.q, case.a, case.b, case.n_pre
    large = case.geo.bits >= 8192                           # (the largest sizes: each scalar on one half of the array)
    one = case.pre(1)
    n1 = k if large else len(a)
    case.same(case.ring(a[:n1]).mulAdd(one, case.ring(b[:n1])), [(x * one + y) % q for x, y in zip(a[:n1], b[:n1])])
    lo = k if large else 0
    case.same(case.ring(a[lo:]).mulAdd(q - 1, case.ring(b[lo:])), [(x * (q - 1) + y) % q for x, y in zip(a[lo:], b[lo:])])
    A, B, a, b = case.ring(a[k:]), case.ring(b[k:]), a[k:], b[k:]
    v = case.rnd[0]
    case.same(A.mulAdd(v, B), [(x * v + y) % q for x, y in zip(a, b)])
    case.same(A.mulAdd(v, None), [x * v % q for x in a])
    case.same(A.mulAdd(q - 1, None), [x * (q - 1) % q for x in a])


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_array_lengths_around_a_workgroup(case, n):
    """The last workgroup is full, one short, one over: a dead lane recomputes element n - 1, an edge value."""
    q = case.q
    k = case.n_pre                                          # (the preimages of the edge pairs come first)
    a = (case.a[:k] * (n // k + 1))[:n]
    b = (case.b[:k] * (n // k + 1))[:n]
    A, B = case.ring(a), case.ring(b)
    case.same(A.add(B), [(x + y) % q for x, y in zip(a, b)])
    case.same(A.neg(), [-x % q for x in a])
    case.same(A.mulAdd(q - 1, B), [(x * (q - 1) + y) % q for x, y in zip(a, b)])
    case.same(A.mulAdd(2, None), [2 * x % q for x in a])
    assert A.sum() == sum(a) % q and A.innerProduct(B) == sum(x * y for x, y in zip(a, b)) % q
    assert A.maxBits() == max(x.bit_length() for x in a)
    assert A.get(n - 1) == a[-1]


# ---- reductions and scans ---------------------------------------------------------------------------------------------
def test_sum_inner_product_and_prod(case):
    q, a, b = case.q, case.a, case.b
    assert case.A.sum() == sum(a) % q
    assert case.A.innerProduct(case.B) == sum(x * y for x, y in zip(a, b)) % q
    assert case.A.prod() == 0 and 0 in a
    nz = [x for x in a if x]
    assert case.ring(nz).prod() == pyref.prod(nz, q)
    pre = case.pre
    for x in (1, 2, (q - 1) // 2, q - 2, case.rnd[1]):
        for f in (lambda v: v, pre):                        # the running total passes exactly through q and through 0
            assert case.ring([f(x), f(q - x), f(1)]).sum() == f(1)
            assert case.ring([f(x), f(q - x)]).sum() == 0
            assert case.ring([f(1), f(x), f(q - x - 1)]).sum() == 0
            assert case.ring([f(x), 1, f(1)]).innerProduct(case.ring([1, f(q - x), 1])) == f(1)
            assert case.ring([f(x), 0, f(q - 1)]).prod() == 0
    for m in (1, 2, 3, 16, 17, 64, 65, 257, 258):
        assert case.ring([q - 1] * m).prod() == (1 if m % 2 == 0 else q - 1), m
        assert case.ring([q - 1] * m).sum() == -m % q, m


def test_rec_lin_and_prods(case):
    q = case.q
    lo = case.n_pre if case.geo.bits >= 8192 else 0         # (the largest sizes: the pairs as they stand, a few hundred)
    b = case.b[lo:]
    B = case.ring(b)
    for zeros in (True, False):
        e = list(case.a[lo:])
        for i in range(3, len(e), 7):                       # a zero restarts the recurrence, q - 1 flips the sign
            e[i] = (0 if zeros else 2, 1, q - 1)[(i // 7) % 3]
        if not zeros:
            e = [v or 1 for v in e]
        assert {0, 1, q - 1} <= set(e) or not zeros
        E = case.ring(e)
        x, d = B.recLin(E)
        want, run = [], 0
        for i, (bi, ei) in enumerate(zip(b, e)):
            run = bi if i == 0 else (run * ei + bi) % q
            want.append(run)
        case.same(x, want)
        assert d == want[-1]
        want, run = [], 1
        for ei in e:
            run = run * ei % q
            want.append(run)
        case.same(E.prods(), want)


# ---- access, comparison, the wire -------------------------------------------------------------------------------------
def test_get_equals_and_round_trips(case):
    G, q, a, geo = case.G, case.q, case.a, case.geo
    n = len(a)
    for i in (0, 1, case.n_pre - 1, n // 2, n - 1):
        assert case.A.get(i) == a[i]
    assert case.A.equals(case.ring(a)) and not case.A.equals(case.B)
    top = q.bit_length() - 1                                # the top limb, in the top lane's share where q has the full width
    share = max(re_.LIMB * re_.limbs_per_lane(geo) * (geo.LPE - 1), 0)
    for idx, bit in ((0, 0), (n - 1, top), (n // 2, top), (n // 2, min(share, top))):
        base, other = list(a), list(a)
        base[idx] = (1 << bit) if bit else 3                # below q: q is odd and has bit `top`
        other[idx] = base[idx] ^ (1 << bit)                 # one bit of limb 0 / of the top limb / of the top lane's share
        assert 0 <= other[idx] < base[idx] < q
        assert not case.ring(base).equals(case.ring(other)), (idx, bit)
        assert case.ring(other).equals(case.ring(other))
    assert not case.A.equals(case.ring(a[:-1]))
    assert case.A.toBytes() == b"".join(x.to_bytes(G.exp_bytes, "big") for x in a)
    back = G.ringArrayFromByteTree(case.A.toByteTree())
    assert back.toInts() == a and back.equals(case.A)
    # every word boundary set: the words 0x80000001 (emit_words / limbs_from_be)
    pattern = sum(0x80000001 << (32 * k) for k in range(re_.words(geo)))
    vals = [pattern % q, (pattern >> 1) % q, pattern & ((1 << (q.bit_length() - 1)) - 1)]
    assert G.ringArrayFromByteTree(case.ring(vals).toByteTree()).toInts() == vals


def maxbits_positions(qbits):
    ks = set()
    for w in range(0, 257, 32):
        ks.update((w - 1, w, w + 1))
    ks.update(range(28, qbits, max(28, 28 * (qbits // (28 * 24)))))
    ks.update(range(320, qbits, max(32, 32 * (qbits // (32 * 24)))))
    ks.update((qbits - 33, qbits - 32, qbits - 31, qbits - 2, qbits - 1))
    return sorted(k for k in ks if 0 <= k < qbits)


def test_max_bits(case):
    q = case.q
    qbits = q.bit_length()
    for k in maxbits_positions(qbits):
        m, r = k % 5, k % 3
        assert (1 << k) - 1 < q
        assert case.ring([0] * m + [(1 << k) - 1] + [0] * r).maxBits() == k, k
        if (1 << k) < q:
            assert case.ring([0] * m + [1 << k] + [1] * r).maxBits() == k + 1, k
    assert case.ring([0] * 7).maxBits() == 0
    assert case.ring([]).maxBits() == 0
    assert case.ring([q - 1]).maxBits() == (q - 1).bit_length()
    assert case.A.maxBits() == max(x.bit_length() for x in case.a)
    big = 1 << (qbits - 2)
    for n in (257, 1025):                                   # the maximum first, last (alone in the last workgroup), in the middle
        for pos in (0, n - 1, n // 2):
            vals = [3] * n
            vals[pos] = big
            assert case.ring(vals).maxBits() == qbits - 1, (n, pos)


# ---- the group side: products that canonicalise to exactly 1, or from exactly N ---------------------------------------
def test_group_products_that_end_in_one(case):
    G, p, geo = case.G, case.p, case.geo
    cand = re_.values(p, geo.bits)[:80] + pyref.stream_ints(b"ring-edges/x/%s" % geo.id.encode(), 12, p)
    cand = [a for a in cand if a and math.gcd(a, p) == 1]
    keep = 24 if geo.bits >= 8192 else 92
    xs = cand[:keep]
    xs += [case.pre(a, p) for a in xs[:keep // 2]]          # device form = the edge value itself
    assert all(math.gcd(a, p) == 1 for a in xs) and len(xs) > 20 and p - 1 in xs
    inv = [pow(a, -1, p) for a in xs]
    X = G.toElementArray(xs)
    Y = X.inv()
    assert Y.toInts() == inv
    ones = G.toElementArray([1] * len(xs))
    for prod in (X.mul(Y), Y.mul(X), X.mul(G.toElementArray(inv))):
        assert prod.toInts() == [1] * len(xs) and prod.equals(ones)
    sq = G.toElementArray([p - 1]).mul(G.toElementArray([p - 1]))
    assert sq.toInts() == [1] and sq.equals(G.toElementArray([1]))
    for a, ai in list(zip(xs, inv))[::5]:
        assert G.toElementArray([a, ai, p - 1, p - 1]).prod() == 1
        assert G.toElementArray([p - 1, a, p - 1, ai, p - 1]).prod() == p - 1


# ---- the range check of the import -------------------------------------------------------------------------------------
def out_of_range_values(N, geo, nbytes):
    """N, N + 1, the largest NW words, and N with one bit added in each lane's share: what fits the wire width."""
    L = re_.limbs_per_lane(geo)
    bad = [N, N + 1, (1 << (32 * re_.words(geo))) - 1] + [N + (1 << (re_.LIMB * L * h)) for h in range(geo.LPE)]
    return sorted({v for v in bad if N <= v < 1 << (8 * nbytes)})


def check_range(make, N, geo, nbytes):
    """make(values, checked=False) -> array: every out-of-range value is reported and replaced by 1, alone and together,
    and nothing next to it is touched; in-range values pass unchanged."""
    L = re_.limbs_per_lane(geo)
    good = [5, N - 1, 7, N - 2, (N - 1) ^ (1 << (N.bit_length() - 1)), N >> 1]
    good += [N - (1 << (re_.LIMB * L * h)) for h in range(geo.LPE) if N > 1 << (re_.LIMB * L * h)]
    good = [v for v in good if v]
    assert all(0 < v < N for v in good)
    arr = make(good, checked=False)
    assert arr.all_in_range is True and arr.toInts() == good
    bad = out_of_range_values(N, geo, nbytes)
    assert N in bad
    for v in bad:
        vals = [5, N - 1, v, 7, N - 2]
        arr = make(vals, checked=False)
        assert arr.all_in_range is False, hex(v - N)
        assert arr.toInts() == [5, N - 1, 1, 7, N - 2], hex(v - N)
        with pytest.raises(ValueError):
            make(vals)
    mixed = []
    for v in bad:
        mixed += [N - 1, v]
    arr = make(mixed + [N - 1], checked=False)
    assert arr.all_in_range is False and arr.toInts() == [N - 1, 1] * len(bad) + [N - 1]
    for n in (256, 257):                                    # the offender last, in a full workgroup and alone in the next
        vals = [N - 1] * (n - 1) + [N]
        arr = make(vals, checked=False)
        assert arr.all_in_range is False and arr.toInts() == [N - 1] * (n - 1) + [1]


def test_import_range_check(case):
    nbytes = case.geo.bits // 8
    check_range(case.G.ringArray, case.q, case.geo, nbytes)
    check_range(case.G.toElementArray, case.p, case.geo, nbytes)


@pytest.mark.parametrize("extra", [1, 3])
def test_import_with_leading_bytes(case, extra):
    """A wire width of 4 NW + 1 / + 3 bytes: a value below N under a non-zero leading byte is out of range (the `extra`
    loop of k_import_be), the same value under zero bytes is not."""
    geo, p, q = case.geo, case.p, case.q
    nw4 = 4 * re_.words(geo)
    nb = nw4 + extra
    G = case.vmn.ModPGroup(case.ctx, p, q, 3, nbytes=nb)
    try:
        assert G.nbytes == nb and G.exp_bytes == nb
        for make, N in ((G.ringArray, q), (G.toElementArray, p)):
            check_range(make, N, geo, nb)
            lows = [N - 1, 1, N >> 1]
            for low in lows:
                for pos in range(extra):
                    for byte in (1, 0x80):
                        lead = bytearray(extra)
                        lead[pos] = byte
                        row = bytes(lead) + low.to_bytes(nw4, "big")
                        ok_row = bytes(extra) + low.to_bytes(nw4, "big")
                        blk = (N - 2).to_bytes(nb, "big") + row + ok_row + (5).to_bytes(nb, "big")
                        arr = make(blk, checked=False)
                        assert arr.all_in_range is False, (hex(low), pos, byte)
                        assert arr.toInts() == [N - 2, 1, low, 5]
            arr = make(b"".join(bytes(extra) + low.to_bytes(nw4, "big") for low in lows), checked=False)
            assert arr.all_in_range is True and arr.toInts() == lows
            assert arr.toBytes() == b"".join(low.to_bytes(nb, "big") for low in lows)
    finally:
        G.close()


def test_wire_width_with_a_partial_word(case):
    """A wire width that is no multiple of 4 (4 NW - 3 bytes; the moduli 24 bits shorter, the same geometry): the edge
    values round-trip through the partial top word of load_be_word / store_be_word, and the range check holds."""
    geo = case.geo
    bits = geo.bits - 24
    nb = 4 * re_.words(geo) - 3
    p = (1 << bits) - 1
    q = (case.q >> 24) | 1 if case.q.bit_length() > bits else case.q
    G = case.vmn.ModPGroup(case.ctx, p, q, 3, nbytes=nb)
    try:
        assert G.nbytes == nb and G.exp_bytes == nb
        for make, N, tree in ((G.ringArray, q, G.ringArrayFromByteTree), (G.toElementArray, p, G.toElementArrayFromByteTree)):
            vals = [v for v in re_.values(N, bits) if v]
            arr = make(vals, checked=False)
            assert arr.all_in_range is True and arr.toInts() == vals
            assert arr.toBytes() == b"".join(v.to_bytes(nb, "big") for v in vals)
            assert tree(arr.toByteTree()).toInts() == vals
            check_range(make, N, geo, nb)
        A = G.ringArray(re_.values(q, bits))
        assert A.neg().toInts() == [-v % q for v in re_.values(q, bits)]
    finally:
        G.close()


# ---- the same kernels as the scalar field of a curve -------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_curve_scalar_fields(curve, vmn, gpu_ctx):
    G = vmn.ECqPGroup(gpu_ctx, curve)
    try:
        q = G.q
        bits = q.bit_length()
        rows = next(g.rows for g in re_.GEOMETRIES if bits <= g.bits)
        plain = re_.catalogue(q, bits)
        pairs = re_.montgomery_preimages(plain, q, rows) + plain
        a, b = [x for x, _ in pairs], [y for _, y in pairs]
        A, B = G.ringArray(a), G.ringArray(b)

        def same(arr, want):
            assert arr.toInts() == want and arr.equals(G.ringArray(want))
        same(A.add(B), [(x + y) % q for x, y in zip(a, b)])
        same(A.neg(), [-x % q for x in a])
        same(A.add(A.neg()), [0] * len(a))
        v = pyref.stream_ints(b"ring-edges/curve-v", 1, q)[0]
        for s in (0, 1, 2, q - 1, v):
            same(A.mulAdd(s, B), [(x * s + y) % q for x, y in zip(a, b)])
            same(A.mulAdd(s, None), [x * s % q for x in a])
        assert A.sum() == sum(a) % q
        assert A.innerProduct(B) == sum(x * y for x, y in zip(a, b)) % q
        assert A.maxBits() == max(x.bit_length() for x in a) and G.ringArray([0, 0]).maxBits() == 0
        for k in (0, 1, 31, 32, 33, 64, 224, 255, bits - 1):
            assert G.ringArray([0, (1 << k) - 1, 0]).maxBits() == k
            assert G.ringArray([1 << k]).maxBits() == k + 1
        for bad in (q, q + 1, (1 << (8 * G.exp_bytes)) - 1):
            arr = G.ringArray([q - 1, bad, 2], checked=False)
            assert arr.all_in_range is False and arr.toInts() == [q - 1, 1, 2]
        assert G.ringArray([q - 1, 0, 2], checked=False).all_in_range is True
    finally:
        G.close()
