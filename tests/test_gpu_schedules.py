"""GPU suite: every schedule the library picks from the array size, forced through its knob at a size the exact references
can afford -- the window width of the multi-exponentiation (VMN_WINDOW_BITS, signed and unsigned windows: VMN_SIGNED_WINDOWS),
the fan-in and depth of its bucket trees (VMN_TREE_FANIN), the chunk and depth of the scans (VMN_SCAN_CHUNK), the levels of
the batched inversion (VMN_EC_NORMALISE_CHUNK), the fixed-base window and its split into pieces (VMN_FIXED_WINDOW,
VMN_FIXED_WINDOW_REUSE, VMN_FIXED_SPLIT_FILL), and the kernels no other module runs (VMN_EC_HORNER_DEVICE,
VMN_EC_EXPORT_DEVICE, membership by x^q = 1, VMN_PAIR_MIXED=0).  The other GPU modules meet the values a 10^5 - 10^6 array uses
(13-bit windows, five tree levels, three levels of inversions, 16-bit tables) through algebraic identities only.

A forced value that the library ignored would let a case pass without having run what it names, so every case also asserts
a WITNESS of the schedule: launch counts per kernel family (Context.timing_report()) and the bytes of the cached tables
(tableBytes()), computed here from the arithmetic the host code documents (the functions below restate it).

References: the GMP oracle for modular groups, the affine Python curve for curves -- over 16 base points with aggregated
coefficients, so that its cost does not grow with the array.

GPU suite wall time (pytest -m gpu on one MI355X, once each): 447 s at the parent commit (318 tests), 415 s with this module
(428 tests; measured on another machine, which is where the difference comes from -- the module alone takes 20 s)."""
import collections
import contextlib
import os
import random

import pytest

from named_curves import ref_curve
from oracle import pyref
from oracle.pyref_ec import CURVES, Curve

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------------
# the schedules, as csrc/vmnhip.hip documents them
# ------------------------------------------------------------------------------------------------------------------------
def ceil_div(a, b):
    return -(-a // b)


def ring_words(qbits):
    """32-bit words of an exponent row (size_for_bits): what a signed recoding covers."""
    return next(nw for bits, nw in ((256, 8), (384, 12), (512, 16), (1024, 32), (2048, 64), (3072, 96), (4096, 128)) if qbits <= bits)


def window_digits(e, c, nwin, signed):
    """The digits of e in nwin windows of c bits; signed: recoded to (-2^(c-1), 2^(c-1)] (light_kernels.h signed_digit)."""
    mask, half = (1 << c) - 1, 1 << (c - 1)
    if not signed:
        return [(e >> (w * c)) & mask for w in range(nwin)]
    out, carry = [], 0
    for w in range(nwin):
        d = ((e >> (w * c)) & mask) + carry
        carry = 1 if d > half else 0
        out.append(d - (1 << c) if d > half else d)
    assert carry == 0
    return out


def scan_launches(n, seglen, chunk, per_level=2):
    """(launches, levels) of scan_affine over n values in segments of seglen: a level that does not fit one chunk runs totals
    (two of them for recLin: per_level = 3) + apply around the scan of its chunk totals.  chunk: VMN_SCAN_CHUNK, or the
    library's own choice as a function of the level's size; with several segments the largest divisor of a segment not above
    it."""
    launches = levels = 0
    while True:
        levels += 1
        ch = chunk(n) if callable(chunk) else chunk
        if seglen != n:
            while ch > 1 and seglen % ch:
                ch -= 1
        if seglen <= ch:
            return launches + 1, levels
        nchunks = ceil_div(n, ch)
        seglen = nchunks if seglen == n else seglen // ch
        n = nchunks
        launches += per_level


def default_ec_scan_chunk(n, num_cus):
    """scan_chunk without the knob, curve scans: 16, halved down to 4 while the top level has fewer lanes than the chip."""
    ch = 16
    while ch > 4 and n // ch < num_cus * 4 * 64 * 4:
        ch >>= 1
    return ch


def normalise_levels(k, n, K, top=2048):
    """The level vector of ec_normalize: values per level until at most `top` are left for the Fermat chain."""
    sizes = [k * n, k * ceil_div(n, K)]
    while sizes[-1] > top:
        sizes.append(ceil_div(sizes[-1], K))
    return sizes


def normalise_launches(k, n, K):
    """up (per group of 8 arrays) + one per upper level, the top, one down per upper level, down (per group of 8 arrays)"""
    L = len(normalise_levels(k, n, K))
    return 2 * ceil_div(k, 8) + 2 * (L - 2) + 1


def k3_schedule(es, c, signed, ebits, F, chunk, k=1, normalised=None, horner_device=False):
    """Launches per family of one multi-exponentiation of k arrays under the exponents es with c-bit windows (expprod_words):
    ebits = the bits the windows cover (signed: all the exponent row can hold, one more for the last carry)."""
    nwin = (ebits + c) // c if signed else ceil_div(ebits, c)
    cb = c - 1 if signed else c
    nb = 1 << cb
    counts = collections.Counter()
    for e in es:
        for w, d in enumerate(window_digits(e, c, nwin, signed)):
            if d:                                           # (zero digits: not inserted / their bucket dropped)
                counts[w, abs(d)] += 1
    largest = max(counts.values())
    levels, mx = 1, ceil_div(largest, F)                  # the largest bucket says how many tree levels there are
    while mx > 1:
        mx = ceil_div(mx, F)
        levels += 1
    scans, depth = scan_launches(k * nwin * nb, nb, chunk)
    want = {"expprod_sort": 4 + (0 if signed else 1) + 3 * levels,      # hist, scan (2), scatter [, drop zero]; 3 per level's shape
            "expprod": levels,                                          # one launch per level for the k <= 8 arrays together
            "expprod_agg": k + (0 if signed else 1) + (1 if horner_device else 0),
            "scan": scans,
            "normalize": normalise_launches(k, len(es), normalised) if normalised else 0}
    return dict(nwin=nwin, nb=nb, levels=levels, largest=largest, scan_depth=depth, launches=want)


@contextlib.contextmanager
def launches(ctx):
    """{family: launches} of what runs inside the block."""
    out = {}
    ctx.timing_reset()
    ctx.timing_enable(True)
    try:
        yield out
    finally:
        ctx.timing_enable(False)
        out.update({fam: v[0] for fam, v in ctx.timing_report().items()})
        ctx.timing_reset()


def witness(got, want, what):
    """The schedule that ran is the schedule that was forced: the families named in `want`, launch for launch."""
    seen = {fam: got.get(fam, 0) for fam in want}
    assert seen == want, ("the forced schedule did not run", what, seen, want)


# ------------------------------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------------------------------
def edge_exponents(c, bits):
    """The recoding's edges at width c, below 2^(bits - 1): every digit exactly 2^(c-1) (a carry arrives or not), one above and
    one below, all ones (a carry through every window), one digit off."""
    lim = (1 << (bits - 1)) - 1
    half = sum((1 << (c - 1)) << (c * k) for k in range(bits // c + 1))
    ones = (1 << (c * (bits // c))) - 1
    return [e & lim for e in (half, half + 1, half - 1, half << 1, ones, ones - (1 << (c - 1)), half ^ (1 << (c * 3 + c - 1)))]


def k3_exponents(order, bits, n, seed):
    """The edges of EVERY width 2 ... 17 (a superset of the edges of the width a case forces: one reference serves all widths),
    the top bits of the order, 0, 1, order - 1, and random ones."""
    rnd = random.Random(seed)
    es = [0, 1, 2, order - 1, order - 2, (1 << (bits - 1)) - 1, (1 << (bits - 1)) % order]
    for c in range(2, 18):
        es += edge_exponents(c, bits)
    return es + [rnd.randrange(order) for _ in range(n - len(es))]


def curve(name):
    return Curve(name) if name in CURVES else ref_curve(name)


def base_points(c, seed, count=16):
    rnd = random.Random(seed)
    return [c.mul(rnd.randrange(1, c.n), c.g) for _ in range(count)]


def aggregated(c, base, owner, es, shift=0):
    """sum_i es[i] * (sign_i base[j_i]) for owner[i] = (j_i, sign_i) or None (the identity), with one scalar multiplication per
    base point."""
    coeff = [0] * len(base)
    for o, e in zip(owner, es):
        if o is not None:
            j = (o[0] + shift) % len(base)
            coeff[j] = (coeff[j] + o[1] * e) % c.n
    return c.exp_prod(base, coeff)


_curve_cases = {}


def curve_case(name, n=320):
    """(curve, points, exponents, reference) of the per-width cases over a curve: the points cycle through 16 base points (equal
    points meet in every bucket)."""
    if name not in _curve_cases:
        c = curve(name)
        base = base_points(c, 4243)
        es = k3_exponents(c.n, c.n.bit_length(), n, 77)
        owner = [(i % 16, 1) for i in range(n)]
        _curve_cases[name] = (c, base, owner, es, aggregated(c, base, owner, es))
    return _curve_cases[name]


def modp_inputs(tag, n, p):
    return [pow(1 + v % (p - 1), 2, p) for v in pyref.stream_ints(tag + b"/x", n, p)]


DEFAULT_WIDE = int(os.environ.get("VMN_WIDE_MAX", 40960))
DEFAULT_WIDE8 = int(os.environ.get("VMN_WIDE8_MAX", 6144))


@pytest.fixture(params=["base geometry", "the geometry of the size"])
def geometry(request, gpu_ctx):
    """Modular groups: every launch in the base geometry, or in the one geom() picks for the size (wide, at these sizes)."""
    if request.param == "base geometry":
        gpu_ctx.set_small_array_threshold(0)
        gpu_ctx.set_tiny_array_threshold(0)
    yield request.param
    gpu_ctx.set_small_array_threshold(DEFAULT_WIDE)
    gpu_ctx.set_tiny_array_threshold(DEFAULT_WIDE8)


@pytest.fixture(scope="module")
def modp(vmn, gpu_ctx):
    cache = {}

    def get(bits):
        if bits not in cache:
            p, q, g = pyref.modp_group(bits)
            cache[bits] = (vmn.ModPGroup(gpu_ctx, p, q, g), p, q, g)
        return cache[bits]
    return get


@pytest.fixture(scope="module")
def ecgroup(vmn, gpu_ctx):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = vmn.ECqPGroup(gpu_ctx, name)
        return cache[name]
    return get


def set_first_level(monkeypatch, rows):
    monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "0" if rows == "normalised" else "1000000000")


# ------------------------------------------------------------------------------------------------------------------------
# 1. the multi-exponentiation at every window width
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [2048, 3072, 4096])
def test_multi_exponentiation_at_every_window_width_modular(bits, geometry, modp, gpu_ctx, oracle_for, monkeypatch):
    """VMN_WINDOW_BITS = 2 ... 16 over 2048 / 3072 / 4096-bit moduli (one, two and four lanes per element in the base geometry)
    with 256-bit exponents against GMP; 2^c buckets per window, so the suffix scan over the buckets and the reduction run at
    the segment length a 10^6 array gives them.  Witness: the launches of the sort, the tree, the aggregation and the scan
    (chunk 2 in the base geometry -- its depth is then c, a different count for every width -- and 4 / 8 / 16 in the other)."""
    G, p, q, g = modp(bits)
    orc = oracle_for(p, q)
    n, ebits = 320, 256
    xs = modp_inputs(b"sched-k3-%d" % bits, n, p)
    xs[5], xs[6], xs[7] = 1, p - 1, xs[8]
    es = k3_exponents(1 << ebits, ebits + 1, n, 78)
    want = orc.exp_prod(xs, es, ebits=ebits, pippenger_c=5)
    assert want == orc.exp_prod(xs, es, ebits=ebits)                  # (GMP's own Pippenger and its plain product agree)
    X = G.toElementArray(xs, checked=False)
    for c in range(2, 17):
        chunk = 2 if geometry == "base geometry" else (4, 8, 16)[c % 3]
        monkeypatch.setenv("VMN_WINDOW_BITS", str(c))
        monkeypatch.setenv("VMN_SCAN_CHUNK", str(chunk))
        sched = k3_schedule(es, c, False, ebits, 8, chunk)
        with launches(gpu_ctx) as got:
            assert X.expProd(es, ebits) == want, c
        witness(got, sched["launches"], ("VMN_WINDOW_BITS", c))
        assert geometry != "base geometry" or sched["scan_depth"] == c


CURVE_WIDTHS = {"P-256": range(2, 18), "P-384": range(2, 18), "brainpoolp256r1": range(2, 18), "secp256k1": range(2, 18),
                "P-521": (2, 9, 13, 17)}


@pytest.mark.parametrize("rows", ["normalised", "as they are"])
@pytest.mark.parametrize("name", list(CURVE_WIDTHS))
def test_multi_exponentiation_at_every_window_width_curves(name, rows, ecgroup, gpu_ctx, monkeypatch):
    """VMN_WINDOW_BITS = 2 ... 17 with signed windows over P-256 (wide digits), P-384, brainpoolp256r1 (general a), secp256k1
    (a = 0) and, at four widths, P-521: the exponents sit on the recoding's edges at the width that runs.  Both first levels.
    Witness as above; the scan runs with chunk 2 over normalised rows (depth c - 1: a different count for every width) and
    with the library's own chunk over the rows as they are."""
    G = ecgroup(name)
    c, base, owner, es, want = curve_case(name)
    X, E = G.toElementArray([base[o[0]] for o in owner]), G.ringArray(es)
    storage = 32 * ring_words(c.n.bit_length())
    set_first_level(monkeypatch, rows)
    for w in CURVE_WIDTHS[name]:
        monkeypatch.setenv("VMN_WINDOW_BITS", str(w))
        if rows == "normalised":
            chunk = 2
            monkeypatch.setenv("VMN_SCAN_CHUNK", "2")
        else:
            chunk = lambda n: default_ec_scan_chunk(n, gpu_ctx.num_cus)
        sched = k3_schedule(es, w, True, storage, 16, chunk, normalised=8 if rows == "normalised" else None)
        with launches(gpu_ctx) as got:
            assert X.expProd(E) == want, w
        witness(got, sched["launches"], ("VMN_WINDOW_BITS", w))
        assert rows != "normalised" or sched["scan_depth"] == max(1, w - 1)


@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1"])
def test_unsigned_windows_over_curves(name, ecgroup, gpu_ctx, monkeypatch):
    """VMN_SIGNED_WINDOWS=0: curves sort by plain digits, 2^c buckets per window, the zero bucket dropped and the segment heads
    blanked as over modular groups -- widths 2 ... 16, alternating first levels.  Witness: one more launch in the sort and in
    the aggregation than the signed form, windows over the order's bits only; 17 bits are the signed picker's alone."""
    G = ecgroup(name)
    c, base, owner, es, want = curve_case(name)
    X, E = G.toElementArray([base[o[0]] for o in owner]), G.ringArray(es)
    monkeypatch.setenv("VMN_SIGNED_WINDOWS", "0")
    monkeypatch.setenv("VMN_SCAN_CHUNK", "4")
    for w in range(2, 17):
        rows = "normalised" if w % 2 else "as they are"
        set_first_level(monkeypatch, rows)
        monkeypatch.setenv("VMN_WINDOW_BITS", str(w))
        sched = k3_schedule(es, w, False, c.n.bit_length(), 16, 4, normalised=8 if rows == "normalised" else None)
        with launches(gpu_ctx) as got:
            assert X.expProd(E) == want, w
        witness(got, sched["launches"], ("VMN_SIGNED_WINDOWS=0, VMN_WINDOW_BITS", w))
    # the same call with signed windows again: the knob is read per call
    monkeypatch.delenv("VMN_SIGNED_WINDOWS")
    set_first_level(monkeypatch, "normalised")
    sched = k3_schedule(es, 16, True, 32 * ring_words(c.n.bit_length()), 16, 4, normalised=8)
    with launches(gpu_ctx) as got:
        assert X.expProd(E) == want
    witness(got, sched["launches"], "signed windows again")


@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1", "modp2048"])
def test_several_arrays_under_one_exponent_array_at_the_widest_window(name, vmn, ecgroup, modp, gpu_ctx, oracle_for, monkeypatch):
    """expProdMulti with k = 3 arrays at the widest window (17 bits signed, 16 unsigned): one sort, the levels and the grouped
    aggregation for the three arrays together (the scan runs over 3 x nwin segments)."""
    monkeypatch.setenv("VMN_SCAN_CHUNK", "16")
    if name == "modp2048":
        G, p, q, g = modp(2048)
        orc = oracle_for(p, q)
        n = 320
        es = k3_exponents(q, q.bit_length(), n, 79)
        arrays = [modp_inputs(b"sched-multi-%d" % a, n, p) for a in range(3)]
        want = [orc.exp_prod(xs, es) for xs in arrays]
        sched = k3_schedule(es, 16, False, q.bit_length(), 8, 16, k=3)
        monkeypatch.setenv("VMN_WINDOW_BITS", "16")
    else:
        G = ecgroup(name)
        c, base, owner, es, _ = curve_case(name)
        arrays = [[base[(o[0] + a) % 16] for o in owner] for a in range(3)]
        want = [aggregated(c, base, owner, es, shift=a) for a in range(3)]
        sched = k3_schedule(es, 17, True, 32 * ring_words(c.n.bit_length()), 16, 16, k=3, normalised=8)
        monkeypatch.setenv("VMN_WINDOW_BITS", "17")
        monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "0")
    X, E = [G.toElementArray(xs) for xs in arrays], G.ringArray(es)
    with launches(gpu_ctx) as got:
        assert vmn.expProdMulti(X, E) == want
    witness(got, sched["launches"], "k = 3 at the widest window")


# ------------------------------------------------------------------------------------------------------------------------
# 2. deep bucket trees
# ------------------------------------------------------------------------------------------------------------------------
def tree_exponents(pattern, n, order, seed):
    """All equal (one bucket per window holds everything: what a batch vector of equal entries does), two values, 90 % equal."""
    rnd = random.Random(seed)
    a, b = (rnd.randrange(order >> 1, order) | int("01" * 128, 2)) % order, rnd.randrange(order)
    if pattern == "all equal":
        return [a] * n
    if pattern == "two values":
        return [a if rnd.random() < 0.6 else b for _ in range(n)]
    return [a if i % 10 else rnd.randrange(order) for i in range(n)]


TREE_WINDOW = 6


@pytest.mark.parametrize("pattern", ["all equal", "two values", "90 % equal"])
@pytest.mark.parametrize("fanin", ["4", None])
@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1"])
def test_deep_bucket_trees_over_curves(name, fanin, pattern, ecgroup, gpu_ctx, monkeypatch):
    """3000 points in ONE bucket per window: six tree levels at VMN_TREE_FANIN=4 (three at the default 16), where the other
    modules reach two or three -- over equal points, opposite pairs and identities in one bucket, as affine rows and as
    Jacobian rows (2 P, one mul on the device), both first levels.  Witness: one "expprod" launch per level."""
    G, c = ecgroup(name), curve(name)
    n = 3000
    base = base_points(c, 910)
    rnd = random.Random(911)
    owner = [None if i % 97 == 5 else (rnd.randrange(16), rnd.choice((1, -1))) for i in range(n)]
    owner[10], owner[11], owner[12], owner[13] = (3, 1), (3, -1), (3, 1), (3, 1)
    es = tree_exponents(pattern, n, c.n, 912)
    want = aggregated(c, base, owner, es)
    X = G.toElementArray([None if o is None else (base[o[0]] if o[1] > 0 else c.neg(base[o[0]])) for o in owner])
    E = G.ringArray(es)
    F = int(fanin) if fanin else 16
    if fanin:
        monkeypatch.setenv("VMN_TREE_FANIN", fanin)
    monkeypatch.setenv("VMN_WINDOW_BITS", str(TREE_WINDOW))
    monkeypatch.setenv("VMN_SCAN_CHUNK", "4")
    storage = 32 * ring_words(c.n.bit_length())
    for rows, arr, ref in (("normalised", X, want), ("as they are", X, want), ("normalised", X.mul(X), c.add(want, want)),
                           ("as they are", X.mul(X), c.add(want, want))):
        set_first_level(monkeypatch, rows)
        sched = k3_schedule(es, TREE_WINDOW, True, storage, F, 4, normalised=8 if rows == "normalised" else None)
        if pattern == "all equal":
            assert sched["largest"] == n and sched["levels"] == (6 if fanin else 3)
        with launches(gpu_ctx) as got:
            assert arr.expProd(E) == ref, rows
        witness(got, sched["launches"], ("VMN_TREE_FANIN", fanin, rows))


@pytest.mark.parametrize("pattern", ["all equal", "two values", "90 % equal"])
@pytest.mark.parametrize("fanin", ["4", None])
@pytest.mark.parametrize("bits", [2048, 3072])
def test_deep_bucket_trees_modular(bits, fanin, pattern, modp, gpu_ctx, oracle_for, monkeypatch):
    """The same over 2048 / 3072-bit moduli (default fan-in 8: four levels; 4: six), 256-bit exponents against GMP; equal
    elements, ones and p - 1 among the elements."""
    G, p, q, g = modp(bits)
    orc = oracle_for(p, q)
    n, ebits = 3000, 256
    xs = modp_inputs(b"sched-tree-%d" % bits, n, p)
    for i in range(0, n, 50):
        xs[i], xs[i + 1], xs[i + 2], xs[i + 3] = 1, p - 1, xs[i + 4], xs[i + 4]
    es = tree_exponents(pattern, n, 1 << ebits, 913)
    want = orc.exp_prod(xs, es, ebits=ebits)
    F = int(fanin) if fanin else 8
    if fanin:
        monkeypatch.setenv("VMN_TREE_FANIN", fanin)
    monkeypatch.setenv("VMN_WINDOW_BITS", str(TREE_WINDOW))
    monkeypatch.setenv("VMN_SCAN_CHUNK", "4")
    sched = k3_schedule(es, TREE_WINDOW, False, ebits, F, 4)
    if pattern == "all equal":
        assert sched["largest"] == n and sched["levels"] == (6 if fanin else 4)
    with launches(gpu_ctx) as got:
        assert G.toElementArray(xs, checked=False).expProd(es, ebits) == want
    witness(got, sched["launches"], ("VMN_TREE_FANIN", fanin))


# ------------------------------------------------------------------------------------------------------------------------
# 3. scans
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [2, 3, 5, 16, 64])
@pytest.mark.parametrize("bits", [2048, 3072, 4096])
def test_scans_at_every_chunk_length_and_depth(bits, chunk, modp, gpu_ctx, oracle_for, monkeypatch):
    """recLin and prods with VMN_SCAN_CHUNK = 2, 3, 5, 16, 64 at one element, one chunk, one chunk and one element, chunk^2 + 1
    and 5000 elements (twelve levels at chunk 2) against GMP.  Witness: the launches of the levels."""
    G, p, q, g = modp(bits)
    orc = oracle_for(p, q)
    monkeypatch.setenv("VMN_SCAN_CHUNK", str(chunk))
    bs_all = pyref.stream_ints(b"sched-scan/b%d" % bits, 5000, q)
    es_all = pyref.stream_ints(b"sched-scan/e%d" % bits, 5000, q)
    for n in (1, chunk, chunk + 1, chunk * chunk + 1, 5000):
        bs, es = bs_all[:n], list(es_all[:n])
        if n > 3:
            es[1], es[n // 2], bs[2] = 1, q - 1, 0
        B, E = G.ringArray(bs), G.ringArray(es)
        with launches(gpu_ctx) as got:
            x, d = B.recLin(E)
        want = orc.rec_lin(bs, es)
        assert x.toInts() == want and d == want[-1], n
        count, depth = scan_launches(n, n, chunk, 3)
        witness(got, {"scan": count}, ("VMN_SCAN_CHUNK", chunk, n))
        with launches(gpu_ctx) as got:
            pr = E.prods()
        assert pr.toInts() == orc.prods(es), n
        witness(got, {"scan": scan_launches(n, n, chunk, 2)[0]}, ("VMN_SCAN_CHUNK", chunk, n))
        if n == 5000 and chunk <= 16:
            assert depth >= 3


@pytest.mark.parametrize("chunk", [2, 3, 5, 16])
@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1", "modp3072"])
def test_segmented_suffix_scan_recurses_through_several_levels(name, chunk, ecgroup, modp, gpu_ctx, oracle_for, monkeypatch):
    """The scans of curve points live inside the aggregation of a multi-exponentiation: 13-bit windows give segments of 2^12
    buckets (2^13 over the modular group), so the segmented suffix scan recurses 12 / 12 / 6 / 3 levels at chunk 2 / 3 / 5 / 16.
    A chunk that does not divide the segment is replaced by the largest divisor below it.
    (Found by this case: the chunk was halved until it divided the segment, so VMN_SCAN_CHUNK=3 over a power of two ended at
    chunks of ONE element, and the recursion over the chunk totals never got shorter.)"""
    monkeypatch.setenv("VMN_WINDOW_BITS", "13")
    monkeypatch.setenv("VMN_SCAN_CHUNK", str(chunk))
    if name == "modp3072":
        G, p, q, g = modp(3072)
        n, ebits = 320, 256
        xs = modp_inputs(b"sched-seg", n, p)
        es = k3_exponents(1 << ebits, ebits + 1, n, 80)
        sched = k3_schedule(es, 13, False, ebits, 8, chunk)
        want = oracle_for(p, q).exp_prod(xs, es, ebits=ebits)
        with launches(gpu_ctx) as got:
            assert G.toElementArray(xs).expProd(es, ebits) == want
    else:
        G = ecgroup(name)
        c, base, owner, es, want = curve_case(name)
        sched = k3_schedule(es, 13, True, 32 * ring_words(c.n.bit_length()), 16, chunk)
        monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "1000000000")
        with launches(gpu_ctx) as got:
            assert G.toElementArray([base[o[0]] for o in owner]).expProd(G.ringArray(es)) == want
    assert sched["scan_depth"] >= 3
    witness(got, sched["launches"], ("VMN_SCAN_CHUNK", chunk))


# ------------------------------------------------------------------------------------------------------------------------
# 4. the batched inversion
# ------------------------------------------------------------------------------------------------------------------------
_sums = {}


def running_sums(name, count=20009):
    """(curve, base, S) with S[i] = d[0] + ... + d[i], d[i] = base[i % 16]: additions only."""
    if name not in _sums:
        c = curve(name)
        base = base_points(c, 920)
        S, acc = [], None
        for i in range(count):
            acc = c.add(acc, base[i % 16])
            S.append(acc)
        _sums[name] = (c, base, S)
    return _sums[name]


INVERSION_CASES = [(8, 1001, 2), (8, 16391, 3), (2, 5001, 3), (2, 9001, 4), (3, 701, 2), (3, 20008, 4)]


@pytest.mark.parametrize("K,n,levels", INVERSION_CASES)
@pytest.mark.parametrize("name", ["P-256", "P-384", "brainpoolp256r1"])
def test_batched_inversion_at_every_depth(name, K, n, levels, ecgroup, gpu_ctx, monkeypatch):
    """ec_normalize with VMN_EC_NORMALISE_CHUNK = 2, 3, 8 and two, three and four levels of chunk products (ragged last chunks
    at every level), over rows with Z != 1: S[i] + d[i + 1], one mul on the device, = S[i + 1] of the running sums.  Identities
    among them: single ones, a run of eight, whole chunks of them (a lane's chunk is strided: the rows c, c + nl, ...; the last
    two chunks, one of them short, and chunk 3), the last row.  Both users of the routine:
    the normalised export against the sums themselves, and the multi-exponentiation over the normalised rows against the
    reference with aggregated coefficients.  Witness: the launches of the "normalize" family."""
    G = ecgroup(name)
    c, base, S = running_sums(name)
    nl = ceil_div(n, K)                                               # lane c of the lowest level holds the rows c, c + nl, c + 2 nl ...
    dead = set(range(40, 48)) | {0, 7, 333, n - 1} | set(range(3, n, nl)) | set(range(nl - 1, n, nl)) | set(range(nl - 2, n, nl))
    X = G.toElementArray([None if i in dead else S[i] for i in range(n)])
    D = G.toElementArray([None if i in dead else base[(i + 1) % 16] for i in range(n)])
    J = X.mul(D)
    want = [None if i in dead else S[i + 1] for i in range(n)]
    sizes = normalise_levels(1, n, K)
    assert len(sizes) == levels and all(s % K for s in sizes[:-1])            # ragged at every level
    monkeypatch.setenv("VMN_EC_NORMALISE_CHUNK", str(K))
    monkeypatch.setenv("VMN_EC_EXPORT_NORMALISE_MIN", "1")
    with launches(gpu_ctx) as got:
        out = J.toInts()
    assert out == want
    witness(got, {"normalize": normalise_launches(1, n, K), "export": 1}, ("VMN_EC_NORMALISE_CHUNK", K, n))
    # the multi-exponentiation: sum_i e[i] S[i + 1] = sum_j (sum of the e[i] with i + 1 >= j) d[j]
    rnd = random.Random(921)
    es = [rnd.randrange(c.n) for _ in range(n)]
    coeff, suffix = [0] * 16, 0
    for j in range(n, -1, -1):
        if j >= 1 and j - 1 not in dead:
            suffix += es[j - 1]
        coeff[j % 16] = (coeff[j % 16] + suffix) % c.n
    monkeypatch.delenv("VMN_EC_EXPORT_NORMALISE_MIN")                # (the window results leave by the ordinary export)
    monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "0")
    with launches(gpu_ctx) as got:
        assert J.expProd(G.ringArray(es)) == c.exp_prod(base, coeff)
    witness(got, {"normalize": normalise_launches(1, n, K)}, ("VMN_EC_NORMALISE_CHUNK in expProd", K, n))


# ------------------------------------------------------------------------------------------------------------------------
# 5. fixed base
# ------------------------------------------------------------------------------------------------------------------------
FIXED_WINDOWS = [2, 3, 5, 8, 11, 13, 16]


def fixed_exponents(order, n, seed):
    """0, 1, order - 1, exponents with zero windows and with all-ones windows at every width, random ones."""
    rnd = random.Random(seed)
    bits = order.bit_length()
    es = [0, 1, order - 1, order - 2, 1 << (bits - 2), (1 << (bits - 1)) - 1]
    for w in FIXED_WINDOWS:
        ones = (1 << w) - 1
        es.append(sum(ones << (2 * w * k) for k in range(bits // (2 * w))) % order)              # all ones / zero, alternating
        es.append(sum((ones << (2 * w * k + w)) for k in range(bits // (2 * w))) % order)
        es.append(((ones << (w * (bits // w - 1))) | 1) % order)                                  # zero windows between the ends
    return es + [rnd.randrange(order) for _ in range(n - len(es))]


@contextlib.contextmanager
def tables_released(G, *bases):
    """The tables of these bases leave the group's cache, whatever happens inside (the groups are shared by the module)."""
    try:
        yield
    finally:
        for b in bases:
            G.releaseFixed(b)


def fixed_case(G, ctx, base, E, w, nwin, row_bytes=None):
    """One fixed-base exponentiation on a table built now: (result, row bytes); witness = the table's size and the launches
    of its build (the seed and one launch per level 1 ... w - 1)."""
    G.releaseFixed(base)
    assert G.tableBytes() == 0
    with launches(ctx) as got:
        out = G.exp(base, E)
    witness(got, {"fixed_table": w}, ("VMN_FIXED_WINDOW", w))
    entries = nwin << w
    assert G.tableBytes() % entries == 0, ("VMN_FIXED_WINDOW", w, G.tableBytes(), entries)
    row = G.tableBytes() // entries
    assert row_bytes is None or row == row_bytes, ("VMN_FIXED_WINDOW", w, G.tableBytes(), entries, row_bytes)
    return out, row


@pytest.mark.parametrize("bits", [2048, 3072])
def test_fixed_base_tables_at_every_window_modular(bits, modp, gpu_ctx, oracle_for, monkeypatch):
    """VMN_FIXED_WINDOW = 2 ... 16 over 2048 / 3072-bit groups (2047 / 3071-bit exponents: no window divides them), exponents
    with zero and all-ones windows, 0 and q - 1, against GMP.  Witness: tableBytes() = nwin 2^w rows of the group's row size
    (304 / 448 bytes: 76 / 2 x 56 words of 28-bit limbs) and w launches of the table's build."""
    G, p, q, g = modp(bits)
    orc = oracle_for(p, q)
    base = pow(g, 0x1234567, p)
    es = fixed_exponents(q, 200, 930)
    want = orc.exp_fixed(base, es)
    E = G.ringArray(es)
    with tables_released(G, base):
        for w in FIXED_WINDOWS:
            monkeypatch.setenv("VMN_FIXED_WINDOW", str(w))
            assert q.bit_length() % w
            out, _ = fixed_case(G, gpu_ctx, base, E, w, ceil_div(q.bit_length(), w), {2048: 304, 3072: 448}[bits])
            assert out.toInts() == want, w


@pytest.mark.parametrize("name", ["P-256", "secp256k1"])
def test_fixed_base_tables_at_every_window_curves(name, ecgroup, gpu_ctx, monkeypatch):
    """The same over P-256 and secp256k1 (k_ec_fixed_level, the table normalised by the batched inversion: three levels of it
    from w = 11 on) against the affine reference; rows of 3 x 12 words."""
    G, c = ecgroup(name), curve(name)
    base = c.mul(0x7654321, c.g)
    es = fixed_exponents(c.n, 200, 931)
    want = c.exp_fixed(base, es)
    E = G.ringArray(es)
    with tables_released(G, base):
        for w in FIXED_WINDOWS:
            monkeypatch.setenv("VMN_FIXED_WINDOW", str(w))
            out, _ = fixed_case(G, gpu_ctx, base, E, w, ceil_div(c.n.bit_length(), w), 144)
            assert out.toInts() == want, w


def split_parts(n, nwin, fill):
    """Pieces an element's chain of nwin products is cut into (vmn_group_exp_fixed)."""
    parts = 1
    while parts < 16 and 2 * parts * n <= fill and nwin // (2 * parts) >= 4:
        parts *= 2
    return parts


DEFAULT_SPLIT_FILL = 786432


@pytest.mark.parametrize("fill", ["0", None, str(1 << 40)])
def test_fixed_base_chain_cut_into_pieces(fill, vmn, gpu_ctx, oracle_for, short_group, monkeypatch):
    """VMN_FIXED_SPLIT_FILL = 0 / default / huge, crossed with windows whose nwin / (2 parts) lands on both sides of 4 (256-bit
    exponents: 128 ... 16 windows, cut into 16, 8, 4 pieces or not at all), and an array large enough for the default to stop
    before the huge value does.  Witness: on the cached table the only "modmul" launches are the log2(parts) levels of the
    tree that multiplies the pieces together."""
    p, q, g = short_group
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    orc = oracle_for(p, q)
    base = pow(g, 0xabcdef, p)
    limit = DEFAULT_SPLIT_FILL if fill is None else int(fill)
    if fill is not None:
        monkeypatch.setenv("VMN_FIXED_SPLIT_FILL", fill)
    seen = set()
    for n, windows in ((200, FIXED_WINDOWS), (50000, [2])):
        es = fixed_exponents(q, n, 932)
        want = orc.exp_fixed(base, es)
        E = G.ringArray(es)
        for w in windows:
            monkeypatch.setenv("VMN_FIXED_WINDOW", str(w))
            nwin = ceil_div(q.bit_length(), w)
            out, _ = fixed_case(G, gpu_ctx, base, E, w, nwin)
            assert out.toInts() == want, (n, w)
            parts = split_parts(n, nwin, limit)
            seen.add((n, parts))
            with launches(gpu_ctx) as got:
                again = G.exp(base, E)
            assert again.toInts() == want, (n, w)
            witness(got, {"fixed_table": 0, "fixed": 1, "modmul": parts.bit_length() - 1}, ("VMN_FIXED_SPLIT_FILL", fill, n, w))
    G.releaseFixed(base)
    assert seen == ({(200, 1), (50000, 1)} if fill == "0" else
                    {(200, 16), (200, 8), (200, 4), (50000, 8 if fill is None else 16)})


def test_fixed_window_of_a_long_lived_base(modp, gpu_ctx, oracle_for, monkeypatch):
    """VMN_FIXED_WINDOW_REUSE acts on the tables of long-lived bases only (precomputeFixed): the generator's table is built
    with it and serves the later calls; a base seen for the first time keeps the window of one call."""
    G, p, q, g = modp(2048)
    orc = oracle_for(p, q)
    es = fixed_exponents(q, 200, 933)
    E = G.ringArray(es)
    nwin = lambda w: ceil_div(q.bit_length(), w)
    monkeypatch.setenv("VMN_FIXED_WINDOW_REUSE", "13")
    other = pow(g, 77, p)
    with tables_released(G, g, other):
        G.releaseFixed(g)
        assert G.tableBytes() == 0
        with launches(gpu_ctx) as got:
            G.precomputeFixed(g, 200, 16)
        witness(got, {"fixed_table": 13}, "VMN_FIXED_WINDOW_REUSE")
        assert G.tableBytes() == (nwin(13) << 13) * 304
        with launches(gpu_ctx) as got:
            assert G.exp(g, E).toInts() == orc.exp_fixed(g, es)
        witness(got, {"fixed_table": 0}, "the long-lived table serves")
        with launches(gpu_ctx) as got:
            assert G.exp(other, E).toInts() == orc.exp_fixed(other, es)
        w1 = got["fixed_table"]                                     # the window of one call: the cost model's, not the knob's
        assert 2 <= w1 < 13 and G.tableBytes() == ((nwin(13) << 13) + (nwin(w1) << w1)) * 304


# ------------------------------------------------------------------------------------------------------------------------
# 6. kernels and paths no other module runs
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1"])
def test_horner_over_the_windows_on_the_device(name, vmn, ecgroup, gpu_ctx, monkeypatch):
    """VMN_EC_HORNER_DEVICE=1 (k_ec_horner, one lane per array): expProd, expProdMulti and PendingExpProd.finish() equal the
    host chain's results and the reference.  Witness: one more launch in the aggregation's family."""
    G = ecgroup(name)
    c, base, owner, es, want = curve_case(name)
    arrays = [[base[(o[0] + a) % 16] for o in owner] for a in range(2)]
    wants = [want, aggregated(c, base, owner, es, shift=1)]
    X, E = [G.toElementArray(xs) for xs in arrays], G.ringArray(es)
    monkeypatch.setenv("VMN_WINDOW_BITS", "7")
    monkeypatch.setenv("VMN_SCAN_CHUNK", "4")
    monkeypatch.setenv("VMN_EC_NORMALISE_MIN", "1000000000")
    storage = 32 * ring_words(c.n.bit_length())
    for device in (False, True, False):                     # (back again: the knob is read per call)
        if device:
            monkeypatch.setenv("VMN_EC_HORNER_DEVICE", "1")
        else:
            monkeypatch.delenv("VMN_EC_HORNER_DEVICE", raising=False)
        with launches(gpu_ctx) as got:
            assert X[0].expProd(E) == want
        witness(got, k3_schedule(es, 7, True, storage, 16, 4, horner_device=device)["launches"], ("VMN_EC_HORNER_DEVICE", device))
        two = k3_schedule(es, 7, True, storage, 16, 4, k=2, horner_device=device)["launches"]
        with launches(gpu_ctx) as got:
            assert vmn.expProdMulti(X, E) == wants
        witness(got, two, ("VMN_EC_HORNER_DEVICE, two arrays", device))
        with launches(gpu_ctx) as got:
            pending = vmn.PendingExpProd(X, E)
            busy = X[0].mul(X[1])
            assert pending.finish() == wants
        witness(got, two, ("VMN_EC_HORNER_DEVICE, pending", device))
        assert busy.get(0) == c.add(arrays[0][0], arrays[1][0])


@pytest.mark.parametrize("name", ["P-256", "brainpoolp256r1", "secp256k1", "P-521"])
def test_export_of_a_few_points_on_the_device(name, ecgroup, gpu_ctx, monkeypatch):
    """Up to four points leave through the host (ec_export_few_host) unless VMN_EC_EXPORT_DEVICE is set: the export kernel
    gives the same points -- the identity and Jacobian rows (Z != 1) among them.  Witness: the "export" launch."""
    G, c = ecgroup(name), curve(name)
    base = base_points(c, 940, 4)
    for n in (1, 2, 3, 4):
        xs = base[:n]
        if n >= 2:
            xs[1] = None
        X = G.toElementArray(xs)
        J = X.mul(G.toElementArray([base[3]] * n))                  # Jacobian rows; base[3] + base[3] in the last row of n = 4
        want = [c.add(P, base[3]) for P in xs]
        for arr, ref in ((X, xs), (J, want)):
            monkeypatch.delenv("VMN_EC_EXPORT_DEVICE", raising=False)
            with launches(gpu_ctx) as got:
                host = arr.toBytes()
            witness(got, {"export": 0}, "host export")
            monkeypatch.setenv("VMN_EC_EXPORT_DEVICE", "1")
            with launches(gpu_ctx) as got:
                dev = arr.toBytes()
            witness(got, {"export": 1}, "VMN_EC_EXPORT_DEVICE")
            assert dev == host and G.dec_els(dev) == ref, n
            assert arr.get(n - 1) == ref[n - 1] and arr.prod() == c.prod(ref)


def is_probable_prime(n, rnd):
    if n < 2:
        return False
    for sp in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):
        if n % sp == 0:
            return n == sp
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for _ in range(32):
        x = pow(rnd.randrange(2, n - 1), d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


SMALL_PRIMES = [s for s in range(3, 2000, 2) if all(s % t for t in range(3, int(s ** 0.5) + 1, 2))]


@pytest.fixture(scope="module")
def short_group():
    """p = k q + 1 with a 1024-bit p and a 256-bit q (k > 2: the reference's ModPGroup allows such groups), g of order q:
    a seeded search."""
    rnd = random.Random(20240607)
    while True:
        q = rnd.getrandbits(256) | (3 << 254) | 1
        if all(q % s for s in SMALL_PRIMES) and is_probable_prime(q, rnd):
            break
    while True:
        k = (rnd.getrandbits(768) | (3 << 766)) & ~1
        p = k * q + 1
        if all(p % s for s in SMALL_PRIMES) and is_probable_prime(p, rnd):
            break
    assert p.bit_length() == 1024 and q.bit_length() == 256
    h = 2
    while pow(h, k, p) == 1:
        h += 1
    g = pow(h, k, p)
    assert pow(g, q, p) == 1 and g != 1
    return p, q, g


def test_membership_by_power_in_a_group_with_a_short_subgroup(vmn, gpu_ctx, oracle_for, short_group):
    """p = k q + 1 with k > 2: the Jacobi symbol does not decide, membership is x^q = 1 for every element (shared-exponent
    modpow + compare).  Members, one non-member and p - 1 (of order 2) inside arrays of 3000.  Witness: no launch of the
    Jacobi kernels, one of the power."""
    p, q, g = short_group
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    orc = oracle_for(p, q)
    n = 3000
    es = pyref.stream_ints(b"sched-member/e", n, q)
    xs = orc.exp_fixed(g, es)
    xs[0], xs[1] = 1, g
    X = G.toElementArray(xs)
    with launches(gpu_ctx) as got:
        assert X.isMember()
    witness(got, {"member": 0}, "membership by power")
    assert got.get("modpow", 0) >= 1
    rnd = random.Random(950)
    for pos, bad in ((0, p - 1), (n - 1, p - 1), (1234, rnd.randrange(2, p - 1)), (2999, pow(3, q, p)), (17, pow(g, 5, p) * (p - 1) % p)):
        assert pow(bad, q, p) != 1
        ys = list(xs)
        ys[pos] = bad
        assert not G.toElementArray(ys, checked=False).isMember(), pos
    assert G.toElementArray([xs[5]]).isMember() and not G.toElementArray([p - 1], checked=False).isMember()


def test_array_operations_with_exponents_much_shorter_than_the_modulus(vmn, gpu_ctx, oracle_for, short_group):
    """The same group (exponent rows of 1024 bits holding 256-bit residues) through the array operations, against GMP."""
    p, q, g = short_group
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    orc = oracle_for(p, q)
    n = 700
    es = pyref.stream_ints(b"sched-short/e", n, q)
    fs = pyref.stream_ints(b"sched-short/f", n, q)
    es[0], es[1], es[2] = 0, 1, q - 1
    xs = orc.exp_fixed(g, fs)
    X, E, F = G.toElementArray(xs), G.ringArray(es), G.ringArray(fs)
    assert X.exp(E).toInts() == orc.exp_array(xs, es)
    assert G.exp(g, E).toInts() == orc.exp_fixed(g, es)
    assert X.expProd(E) == orc.exp_prod(xs, es)
    assert X.exp(q - 1).toInts() == orc.exp_scalar(xs, q - 1)
    assert X.mul(X.inv()).toInts() == [1] * n
    assert E.mul(F).toInts() == [a * b % q for a, b in zip(es, fs)]
    assert E.add(F).toInts() == [(a + b) % q for a, b in zip(es, fs)]
    assert E.innerProduct(F) == sum(a * b for a, b in zip(es, fs)) % q
    x, d = E.recLin(F)
    want = orc.rec_lin(es, fs)
    assert x.toInts() == want and d == want[-1]
    assert F.prods().toInts() == orc.prods(fs)


def test_membership_by_power_agrees_with_the_jacobi_symbol(modp, gpu_ctx, monkeypatch):
    """VMN_MEMBER_BY_POWER=1 on a safe prime: x^q = 1 gives the Jacobi kernels' verdicts.  Witness: which family ran."""
    G, p, q, g = modp(2048)
    n = 3000
    xs = modp_inputs(b"sched-member-safe", n, p)
    bad = list(xs)
    bad[n - 2] = p - xs[n - 2]                                     # -x of a square: a non-residue (p = 3 mod 4)
    for arr, verdict in ((xs, True), (bad, False), ([p - 1] + xs[1:], False)):
        X = G.toElementArray(arr, checked=False)
        monkeypatch.delenv("VMN_MEMBER_BY_POWER", raising=False)
        with launches(gpu_ctx) as got:
            assert X.isMember() is verdict
        witness(got, {"member": 1, "modpow": 0}, "the Jacobi symbol")
        monkeypatch.setenv("VMN_MEMBER_BY_POWER", "1")
        with launches(gpu_ctx) as got:
            assert X.isMember() is verdict
        witness(got, {"member": 0}, "VMN_MEMBER_BY_POWER")
        assert got.get("modpow", 0) >= 1


@pytest.mark.parametrize("mixed", [None, "0", "1"])
def test_two_powers_in_one_launch_with_and_without_the_mixed_form(mixed, modp, gpu_ctx, oracle_for, monkeypatch):
    """The mixed case of test_gpu_parity.test_two_powers_in_one_launch (7001 and 6500 elements of a 2048-bit group: the longer
    job eight lanes per element, the shorter four) with VMN_PAIR_MIXED unset, 0 and 1: k_modpow_jobs_mixed or k_modpow_jobs,
    the same powers.  Witness: the "pair_mixed" mark the mixed launch leaves in the timing report."""
    G, p, q, g = modp(2048)
    orc = oracle_for(p, q)
    big = 7001
    xs = modp_inputs(b"sched-pair-mixed", big, p)
    fs = pyref.stream_ints(b"sched-pair-mixed/f", big, q)
    ys = xs[::-1]
    e256 = pyref.stream_ints(b"sched-pair/e", 1, 1 << 256)[0]
    if mixed is None:
        monkeypatch.delenv("VMN_PAIR_MIXED", raising=False)
    else:
        monkeypatch.setenv("VMN_PAIR_MIXED", mixed)
    for nx, ny, e, fbits in ((6500, big, e256, 613), (big, 6300, q - 1, 100)):
        f = [v % (1 << fbits) for v in fs[:ny]]
        with launches(gpu_ctx) as got:
            gx, gy = G.toElementArray(xs[:nx]).expPair(e, G.toElementArray(ys[:ny]), G.ringArray(f), fbits)
        witness(got, {"modpow": 1, "pair_mixed": 0 if mixed == "0" else 1}, ("VMN_PAIR_MIXED", mixed))
        assert gx.toInts() == orc.exp_scalar(xs[:nx], e), (nx, ny)
        assert gy.toInts() == orc.exp_array(ys[:ny], f), (nx, ny)
