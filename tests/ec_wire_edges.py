"""Wire-format catalogue for the curve import and export (csrc/ec_kernels.h: k_ec_import, k_ec_export; csrc/vmnhip.hip:
ec_export_few_host, import_one): the encodings at which untrusted bytes become device rows, and the reference verdict on
each of them.  Shared by tests/test_gpu_ec_wire_edges.py (the kernels against decode()) and
tests/test_ec_wire_edge_catalogue.py (the catalogue holds what it claims; decode() is libcrypto's verdict; no GPU).

A point crosses the boundary as x || y, `nbytes` big-endian bytes each.  The import rule of include/vmnhip.h, in plain
integers, is decode(): all 0xff is the identity; a coordinate >= p or a pair off the curve is replaced by the identity and
raises the flag.  A coordinate x + p that passed the range check would reduce to a valid point -- one group element, two
encodings -- so the aliases x + p and y + p are the rows that matter: they are the only inputs on which a missing or
off-by-one range check differs from a correct one.

Every constant comes from the product's own table (ecscalar.py through named_curves.ref_curve); the points are computed
here, with Python integers."""
from collections import namedtuple

from named_curves import library_table, ref_curve
from oracle import pyref
from oracle.pyref_prg import sqrt_mod

# One curve per kernel instantiation of csrc/ec_instances.h (kind, field limbs), and those whose widths are awkward: P-192
# (24 of the 28 bytes of its packed words), prime239v1 (30 of 32), P-521 (66 of 68), brainpoolp512r1 (64 of 68).
CURVES = [
    ("P-224", "NIST", 9), ("P-192", "NIST", 9), ("P-256", "NIST", 10), ("P-384", "NIST", 15), ("P-521", "NIST", 21),
    ("secp224k1", "GENERAL", 9), ("brainpoolp256r1", "GENERAL", 10), ("secp256k1", "GENERAL", 10), ("prime239v1", "GENERAL", 10),
    ("brainpoolp320r1", "GENERAL", 13), ("brainpoolp384r1", "GENERAL", 15), ("brainpoolp512r1", "GENERAL", 21),
]
NAMES = [name for name, _, _ in CURVES]
WIDTHS = ("natural", "java", "buffer", "beyond")

# the classes of a row; only VALID rows decode to ok = True
VALID, ALIAS, LEAD, RANGE, OFF, NEARINF = "valid", "alias", "lead", "range", "off", "nearinf"
Row = namedtuple("Row", "label cls x y")                 # x, y: `nbytes` bytes each

# mutants of decode() (never of a kernel): what tests/test_ec_wire_edge_catalogue.py proves the catalogue catches
NO_RANGE_X, NO_RANGE_Y, GT_FOR_GE, LOW_WORDS_ONLY, NIST_A = "no-range-x", "no-range-y", "gt-for-ge", "low-words-only", "nist-a"
MUTANTS = (NO_RANGE_X, NO_RANGE_Y, GT_FOR_GE, LOW_WORDS_ONLY, NIST_A)

ALIAS_Y_SEARCH = 400                                      # k G, k <= 400: the points whose y + p may fit the width


def decode(curve, nbytes, xbytes, ybytes, mutant=None, nw=None):
    """(point | None, ok): the import rule of include/vmnhip.h.  `mutant` breaks it in one of five ways (`nw`: the packed
    words of the curve's kernel, for LOW_WORDS_ONLY)."""
    assert len(xbytes) == nbytes and len(ybytes) == nbytes
    if xbytes + ybytes == b"\xff" * (2 * nbytes):
        return None, True
    p, a, b = curve.p, curve.a, curve.b
    x, y = int.from_bytes(xbytes, "big"), int.from_bytes(ybytes, "big")
    if mutant == LOW_WORDS_ONLY:                          # the bytes above the packed words are never looked at
        x, y = x & ((1 << (32 * nw)) - 1), y & ((1 << (32 * nw)) - 1)
    if mutant == NIST_A:
        a = p - 3
    x_bad = x > p if mutant == GT_FOR_GE else x >= p
    y_bad = y > p if mutant == GT_FOR_GE else y >= p
    if (x_bad and mutant != NO_RANGE_X) or (y_bad and mutant != NO_RANGE_Y):
        return None, False
    if (y * y - (x * x * x + a * x + b)) % p != 0:
        return None, False
    return (x % p, y % p), True


# ---- the points -------------------------------------------------------------------------------------------------------
def lift(x, p, a, b):
    """The smaller y with y^2 = x^3 + a x + b mod p, or None."""
    y = sqrt_mod((x * x * x + a * x + b) % p, p)
    return None if y is None else min(y, p - y)


def _search(p, a, b, xs):
    for x in xs:
        y = lift(x, p, a, b)
        if y is not None and y != 0:
            return x, y
    raise AssertionError("no point found")


_facts = {}


def facts(name):
    """Everything about a curve that does not depend on the width, computed once: the oracle's curve, the geometry of its
    kernel, the edge points and the points of the neighbouring curves."""
    if name in _facts:
        return _facts[name]
    c = ref_curve(name)
    table, _ = library_table()
    p, a, b = c.p, c.a, c.b
    f = dict(c=c, name=name, NW=table[name]["NW"], S=table[name]["S"], kind="NIST" if table[name]["a"] is None else "GENERAL")
    ks = [1 + k % (c.n - 1) for k in pyref.stream_ints(b"ec-wire-edges/k/" + name.encode(), 3, c.n)]
    f["multiples"] = [c.mul(k, c.g) for k in ks]
    f["min_x"] = _search(p, a, b, range(0, 1 << 16))
    f["max_x"] = _search(p, a, b, range(p - 1, p - (1 << 16), -1))
    y0 = lift(0, p, a, b)
    f["zero_x"] = None if y0 is None else (0, y0)
    # points of the curves next door: a replaced (by -3, the NIST kernels' a; by 0 where a = -3 already: the NIST curves and
    # prime239v1, which runs in the general kernels all the same), b replaced by b + 1
    a2 = p - 3 if a != p - 3 else 0
    f["wrong_a"] = next(P for P in (_search(p, a2, b, range(s, 1 << 16)) for s in range(1, 64)) if not c.on_curve(P))
    f["wrong_b"] = next(P for P in (_search(p, a, (b + 1) % p, range(s, 1 << 16)) for s in range(1, 64)) if not c.on_curve(P))
    kg, acc = [], None
    for _ in range(ALIAS_Y_SEARCH):
        acc = c.add(acc, c.g)
        kg.append(acc)
    f["kG"] = kg
    _facts[name] = f
    return f


def widths(name):
    """{natural, java, buffer, beyond}: the coordinate widths of a curve.  natural: the bytes of p; java: the length of
    BigInteger.toByteArray() of p (vmn_group_set_wire_bytes(g, 0, 0)); buffer = 4 NW + 4 and beyond = 4 NW + 5: the widest
    coordinate the framed import once moved into a per-thread buffer, and the narrowest it could not."""
    f = facts(name)
    bits = f["c"].p.bit_length()
    return dict(natural=(bits + 7) // 8, java=bits // 8 + 1, buffer=4 * f["NW"] + 4, beyond=4 * f["NW"] + 5)


def enc(v, nbytes):
    return int(v).to_bytes(nbytes, "big")


_rows = {}


def catalogue(name, nbytes):
    """(rows, absent): the rows of a curve at a coordinate width, and {label: reason} for every row that cannot exist there."""
    if (name, nbytes) in _rows:
        return _rows[(name, nbytes)]
    f = facts(name)
    c, p = f["c"], f["c"].p
    top = 1 << (8 * nbytes)
    ones = top - 1
    rows, absent = [], {}

    def put(label, cls, x, y):
        rows.append(Row(label, cls, enc(x, nbytes), enc(y, nbytes)))

    gx, gy = c.g
    # -- valid
    put("G", VALID, gx, gy)
    put("-G", VALID, gx, p - gy)
    for i, P in enumerate(f["multiples"]):
        put("kG#%d" % i, VALID, *P)
    for tag, P in (("min-x", f["min_x"]), ("max-x", f["max_x"])):
        put(tag + "+", VALID, P[0], P[1])
        put(tag + "-", VALID, P[0], p - P[1])
    if f["zero_x"]:
        put("x=0+", VALID, 0, f["zero_x"][1])
        put("x=0-", VALID, 0, p - f["zero_x"][1])
    else:
        absent["x=0+"] = absent["x=0-"] = "b is not a square mod p: no point has x = 0"
    rows.append(Row("identity", VALID, b"\xff" * nbytes, b"\xff" * nbytes))
    # -- out of range, but a valid point after reduction
    mx, my = f["min_x"]
    if mx + p < top:
        put("alias-x+", ALIAS, mx + p, my)
        put("alias-x-", ALIAS, mx + p, p - my)
    else:
        absent["alias-x+"] = absent["alias-x-"] = "x + p does not fit %d bytes" % nbytes
    hit = next(((P[0], y) for P in f["kG"] for y in (P[1], p - P[1]) if y + p < top), None)
    if hit:
        put("alias-y", ALIAS, hit[0], hit[1] + p)
        if mx + p < top and hit[0] + p < top:
            put("alias-xy", ALIAS, hit[0] + p, hit[1] + p)
    else:
        absent["alias-y"] = ("y + p fits %d bytes only for y < 2^%d - p: none of +-k G, k <= %d"
                             % (nbytes, 8 * nbytes, ALIAS_Y_SEARCH))
    # -- a valid point under a non-zero byte above the packed words
    if nbytes > 4 * f["NW"]:
        qx, qy = f["multiples"][0]
        hi = 8 * (nbytes - 1)
        put("lead-01-x", LEAD, qx | (0x01 << hi), qy)
        put("lead-80-x", LEAD, qx | (0x80 << hi), qy)
        put("lead-01-y", LEAD, qx, qy | (0x01 << hi))
        put("lead-80-y", LEAD, qx, qy | (0x80 << hi))
    else:
        for label in ("lead-01-x", "lead-80-x", "lead-01-y", "lead-80-y"):
            absent[label] = "%d bytes lie within the %d bytes of the packed words" % (nbytes, 4 * f["NW"])
    # -- plainly out of range
    put("(p,y)", RANGE, p, gy)
    put("(x,p)", RANGE, gx, p)
    put("(p-1,p-1)", RANGE, p - 1, p - 1)
    put("ones-x", RANGE, ones, gy)
    put("ones-y", RANGE, gx, ones)
    # -- off the curve
    for label, P in (("y+1", (gx, gy + 1)), ("y-1", (gx, gy - 1)), ("x+1", (gx + 1, gy)), ("x-1", (gx - 1, gy)), ("swapped", (gy, gx))):
        if c.on_curve(P):
            absent[label] = "that neighbour of G lies on the curve"
        else:
            put(label, OFF, *P)
    put("wrong-a", OFF, *f["wrong_a"])
    put("wrong-b", OFF, *f["wrong_b"])
    put("(0,0)", OFF, 0, 0)
    # -- near the encoding of the identity
    put("ff-ylsb", NEARINF, ones, ones - 1)
    put("ff-xmsb", NEARINF, ones >> 1, ones)
    put("ff-x", NEARINF, ones, my)
    _rows[(name, nbytes)] = (rows, absent)
    return rows, absent


LABELS = ("G", "-G", "kG#0", "kG#1", "kG#2", "min-x+", "min-x-", "max-x+", "max-x-", "x=0+", "x=0-", "identity",
          "alias-x+", "alias-x-", "alias-y", "lead-01-x", "lead-80-x", "lead-01-y", "lead-80-y",
          "(p,y)", "(x,p)", "(p-1,p-1)", "ones-x", "ones-y", "y+1", "y-1", "x+1", "x-1", "swapped", "wrong-a", "wrong-b", "(0,0)",
          "ff-ylsb", "ff-xmsb", "ff-x")


def decoded(name, nbytes, rows=None):
    """[(point | None, ok)] of the rows (default: the whole catalogue)."""
    c = facts(name)["c"]
    return [decode(c, nbytes, r.x, r.y) for r in (catalogue(name, nbytes)[0] if rows is None else rows)]


def flat(rows):
    return b"".join(r.x + r.y for r in rows)


def random_valid_rows(name, nbytes, count, seed=b"ec-wire-edges/random"):
    """`count` seeded points of the curve (a seeded x that has a y, the sign of y seeded too), as rows."""
    f = facts(name)
    c = f["c"]
    out, block = [], 0
    while len(out) < count:
        xs = pyref.stream_ints(seed + b"/%s/%d" % (name.encode(), block), 2 * count, c.p)
        block += 1
        for x in xs:
            y = lift(x, c.p, c.a, c.b)
            if y is not None and len(out) < count:
                y = y if x & 1 else c.p - y
                out.append(Row("random#%d" % len(out), VALID, enc(x, nbytes), enc(y, nbytes)))
    return out


# ---- the framed form ---------------------------------------------------------------------------------------------------
def _u32(v):
    return int(v).to_bytes(4, "big")


def framed_point(x, y):
    """node(leaf(x), leaf(y)) = 00 00000002 | 01 len x | 01 len y"""
    return b"\x00" + _u32(2) + b"\x01" + _u32(len(x)) + x + b"\x01" + _u32(len(y)) + y


def framed(rows):
    """The byte tree of a row list: 00 | n | n x node(leaf(x), leaf(y))."""
    return b"\x00" + _u32(len(rows)) + b"".join(framed_point(r.x, r.y) for r in rows)


def header_mutants(rows, nbytes):
    """[(label, byte tree)]: one element of the otherwise valid tree of `rows` with a broken header -- wrong node tag, wrong
    child count, wrong leaf tag on x and on y, a leaf length off by one (the total length kept) on x and on y -- at the
    first, a middle and the last position."""
    good = framed(rows)
    stride = 15 + 2 * nbytes
    edits = (("node-tag", 0, b"\x01"), ("child-count", 1, _u32(3)), ("x-leaf-tag", 5, b"\x00"), ("y-leaf-tag", 10 + nbytes, b"\x02"),
             ("x-leaf-len+1", 6, _u32(nbytes + 1)), ("y-leaf-len-1", 11 + nbytes, _u32(nbytes - 1)))
    out = []
    for pos in sorted({0, len(rows) // 2, len(rows) - 1}):
        for label, off, patch in edits:
            at = 5 + pos * stride + off
            bad = good[:at] + patch + good[at + len(patch):]
            assert len(bad) == len(good) and bad != good
            out.append(("%s@%d" % (label, pos), bad))
    return out
