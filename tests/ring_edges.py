"""Operand catalogue for the light modular layer (csrc/modp_kernels.h: mod_add, mod_neg, sub_full, canonicalize, the range
check of k_import_be): the values at which a carry or a borrow runs through a whole lane's share, and the sums that are
exactly q - 1, q, q + 1 and 2q - 2.  Shared by tests/test_gpu_ring_edges.py (the kernels against Python integers) and
tests/test_ring_edge_catalogue.py (the catalogue really holds such operands; no GPU).

An element is S limbs of 28 bits, cut into LPE shares of L = S / LPE limbs, one share per lane.

Arrays live on the device in Montgomery form: the limbs mod_add, mod_neg and their sub_full see are those of x R mod q
(R = 2^(28 ROWS)), not those of x.  Only the import's range check and the export's last canonicalize work on the limbs of
x itself.  So the GPU tests feed every pair of the catalogue twice: as it stands (import / export / the exact
comparisons), and as its Montgomery preimage (a / R, b / R) mod q -- montgomery_preimages() -- whose device form is
exactly (a, b): that is the array in which the catalogue's ripples reach the add and the negation.  The expected values
are Python integers mod q either way."""
from collections import namedtuple

from oracle import pyref

LIMB = 28
LIMB_MASK = (1 << LIMB) - 1

# One row per built modular geometry (csrc/modp_instances.h): Cfg<S, LPE>, the reduction rows of a product (R = 2^(28 rows)),
# and the thresholds that enter it where the choice depends on the array's size (FORCE of tests/test_gpu_geometry.py).
Geometry = namedtuple("Geometry", "id bits S LPE rows force")
GEOMETRIES = [
    Geometry("256", 256, 10, 1, 10, None),
    Geometry("384", 384, 14, 1, 14, None),
    Geometry("512", 512, 19, 1, 19, None),
    Geometry("1024", 1024, 37, 1, 37, None),
    Geometry("2048-base", 2048, 74, 1, 74, "base"),
    Geometry("2048-wide", 2048, 76, 4, 74, "wide"),
    Geometry("2048-wide8", 2048, 80, 8, 74, "wide8"),
    Geometry("3072-base", 3072, 110, 2, 110, "base"),
    Geometry("3072-wide", 3072, 112, 4, 110, "wide"),
    Geometry("4096", 4096, 148, 4, 148, None),
    Geometry("8192", 8192, 296, 8, 296, None),
    Geometry("16384", 16384, 592, 16, 592, None),
]
GEOMETRY = {g.id: g for g in GEOMETRIES}
MODULI = ("ones", "hi", "step", "rnd", "small256")


def limbs_per_lane(geo):
    return geo.S // geo.LPE


def words(geo):
    """NW: packed 32-bit words of an element on the wire side."""
    return geo.bits // 32


def seeded_odd(seed, bits):
    """A seeded odd integer of exactly `bits` bits (generic_modulus() of tests/test_gpu_modpow29.py, at any size)."""
    return pyref.stream_ints(seed, 1, 1 << bits)[0] | (1 << (bits - 1)) | 1


def modulus(geo, name):
    """The ring modulus `name` of a geometry, or None where it does not exist there (small256 below 1024 bits)."""
    bits = geo.bits
    if name == "ones":                                  # every limb all ones
        return (1 << bits) - 1
    if name == "hi":                                    # one, zero limbs, the top bit: x - q borrows through every limb
        return (1 << (bits - 1)) + 1
    if name == "step":                                  # all-ones shares above a share that is 1, 0, 0 ...
        L = limbs_per_lane(geo) if geo.LPE > 1 else geo.S // 2
        return (1 << bits) - (1 << (LIMB * L)) + 1
    if name == "rnd":
        return seeded_odd(b"ring-edges/q/%d" % bits, bits)
    if name == "small256":                              # every limb above the ninth is zero in q and in the operands
        return seeded_odd(b"ring-edges/q256/%d" % bits, 256) if bits >= 1024 else None
    raise KeyError(name)


def moduli(geo):
    return {name: modulus(geo, name) for name in MODULI if modulus(geo, name) is not None}


def boundaries(bits):
    """The bit positions k the edge values are built around: every limb boundary (which holds every share boundary of every
    geometry) and every word boundary below `bits`; at 8192 and 16384 bits the lane boundaries, the limbs next to them and
    every 64th word boundary."""
    if bits >= 8192:
        lane = LIMB * 37
        ks = set()
        for k in range(lane, bits, lane):
            ks.update((k - LIMB, k, k + LIMB))
        ks.update(range(32 * 64, bits, 32 * 64))
    else:
        ks = set(range(LIMB, bits, LIMB)) | set(range(32, bits, 32))
    return sorted(k for k in ks if 0 < k < bits)


def values(q, bits):
    """V: the edge values below q, in a fixed order, each once."""
    vs = [0, 1, 2, q - 1, q - 2, (q - 1) // 2, (q + 1) // 2]
    for k in boundaries(bits):
        vs += [(1 << k) - 1, 1 << k, (1 << k) + 1, q - (1 << k), q - (1 << k) + 1]
        # q's limbs below k, plus one: q - a borrows in limb 0 and on through every limb below k (the negation's ripple)
        vs.append((q & ((1 << k) - 1)) + 1)
    seen, out = set(), []
    for v in vs:
        if 0 <= v < q and v not in seen:
            seen.add(v)
            out.append(v)
    return out


def catalogue(q, bits):
    """The operand pairs (a, b), both below q, deterministic: the sums q, q - 1, q + 1 for every edge value, zeros on either
    side, the carries born in limb 0, twenty-four seeded random pairs, and (q - 1, q - 1) last (a dead lane recomputes the
    last element: an edge value sits there)."""
    V = values(q, bits)
    pairs = []
    for a in V:
        if a:
            pairs.append((a, q - a))
        pairs.append((a, q - a - 1))
        pairs.append((a, q - a + 1))
        pairs.append((a, 0))
        pairs.append((0, a))
    for k in boundaries(bits):
        pairs.append(((1 << k) - 1, 1))
    rnd = pyref.stream_ints(b"ring-edges/pairs/%d/%x" % (bits, q & 0xffffffff), 48, q)
    pairs += list(zip(rnd[:24], rnd[24:]))
    seen, out = set(), []
    for a, b in pairs:
        if 0 <= a < q and 0 <= b < q and (a, b) not in seen and (a, b) != (q - 1, q - 1):
            seen.add((a, b))
            out.append((a, b))
    out.append((q - 1, q - 1))
    return out


def montgomery_preimages(pairs, q, rows):
    """(a / R, b / R) mod q, R = 2^(28 rows): the pairs whose device (Montgomery) form is exactly (a, b)."""
    rinv = pow(1 << (LIMB * rows), -1, q)
    return [(a * rinv % q, b * rinv % q) for a, b in pairs]


# ---- the limb model of the CPU test ---------------------------------------------------------------------------------
def limbs(x, S):
    out = [(x >> (LIMB * j)) & LIMB_MASK for j in range(S)]
    assert x >> (LIMB * S) == 0
    return out


def carry_chain(a, b, S):
    """(sums, carries): s[j] = a[j] + b[j] limb-wise and c[j] = the carry INTO limb j of the settled sum (c[S] = out)."""
    al, bl = limbs(a, S), limbs(b, S)
    s = [x + y for x, y in zip(al, bl)]
    c = [0]
    for j in range(S):
        c.append((s[j] + c[j]) >> LIMB)
    return s, c


def borrow_chain(x, n, S):
    """(raw, borrows): raw[j] = x[j] - n[j] limb-wise and w[j] = the borrow (0 / 1) INTO limb j of x - n (w[S] = out)."""
    xl, nl = limbs(x, S), limbs(n, S)
    raw = [u - v for u, v in zip(xl, nl)]
    w = [0]
    for j in range(S):
        w.append(1 if raw[j] - w[j] < 0 else 0)
    return raw, w


def carry_into(a, b, pos):
    """The carry into bit `pos` of a + b."""
    m = (1 << pos) - 1
    return ((a & m) + (b & m)) >> pos


def borrow_into(x, n, pos):
    """The borrow (0 / 1) into bit `pos` of x - n."""
    m = (1 << pos) - 1
    return 1 if (x & m) < (n & m) else 0


def carry_ripples_through_share(a, b, geo, h):
    """(a): the sum carries into share h, and every limb of share h - 1 is 0xfffffff + the carry that reaches it -- the
    carry is born in limb 0 of the element (h = 1) or arrives from the share below (h > 1), and whether it leaves share
    h - 1 depends on nothing else."""
    L = limbs_per_lane(geo)
    lo, hi = (h - 1) * L, h * L
    if not carry_into(a, b, LIMB * hi) or (h > 1 and not carry_into(a, b, LIMB * lo)):
        return False
    s, c = carry_chain(a, b, geo.S)
    return all(s[j] + c[j] == 1 << LIMB for j in range(lo, hi))


def borrow_ripples_through_share(x, q, geo, h):
    """(b): x - q borrows into share h, and the limb-wise difference of share h - 1 is all zero but for the limb the borrow
    is born in (limb 0 of the element, h = 1): the borrow that leaves share h - 1 is the one that entered it."""
    L = limbs_per_lane(geo)
    lo, hi = (h - 1) * L, h * L
    if not borrow_into(x, q, LIMB * hi) or (h > 1 and not borrow_into(x, q, LIMB * lo)):
        return False
    raw, _ = borrow_chain(x, q, geo.S)
    return all(raw[j] == 0 for j in range(lo + (1 if h == 1 else 0), hi))


def negation_borrows_across_every_boundary(a, q, geo):
    """(d): q - a borrows into every share above the lowest."""
    L = limbs_per_lane(geo)
    return all(borrow_into(q, a, LIMB * h * L) for h in range(1, geo.LPE))
