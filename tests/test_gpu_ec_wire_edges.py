"""GPU suite: the curve import and export (csrc/ec_kernels.h: k_ec_import, k_ec_export; csrc/vmnhip.hip: ec_export_few_host,
import_one) at their wire-format edges, on one curve per kernel instantiation and at the natural and the Java coordinate
width each -- against tests/ec_wire_edges.decode(), the import rule of include/vmnhip.h in Python integers, by exact
equality.  The rows that matter are the aliases x + p and y + p: out of range, and a valid point if the range check let
them through."""
import ctypes as C

import pytest

import ec_wire_edges as we

pytestmark = pytest.mark.gpu

CASES = [(name, w) for name in we.NAMES for w in ("natural", "java")]
POSITION_CURVES = ["P-256", "brainpoolp320r1", "P-521"]
BEYOND_CURVES = ["P-256", "brainpoolp512r1"]
VMN_ERR_FORMAT = -4


def ints(row):
    """A row as the wrappers' element: a pair of integers of any size below 2^(8 nbytes), None for the all-0xff row."""
    if row.x + row.y == b"\xff" * (2 * len(row.x)):
        return None
    return int.from_bytes(row.x, "big"), int.from_bytes(row.y, "big")


class Case:
    """One curve at one coordinate width: the group, the catalogue and decode()'s verdict on every row."""

    def __init__(self, vmn, gpu_ctx, name, nbytes=None, java=False):
        self.vmn, self.ctx, self.name = vmn, gpu_ctx, name
        self.f = we.facts(name)
        self.c = self.f["c"]
        self.G = vmn.ECqPGroup(gpu_ctx, name, java_widths=java)
        if nbytes is not None:
            vmn._check(vmn.lib().vmn_group_set_wire_bytes(self.G._h, C.c_size_t(nbytes), C.c_size_t(0)))
            self.G._read_widths()
        self.nb = self.G.nbytes
        self.rows, _ = we.catalogue(name, self.nb)
        self.want = we.decoded(name, self.nb)
        self.points = [P for P, _ in self.want]
        self.valid = [r for r in self.rows if r.cls == we.VALID]
        self.valid_points = [P for r, P in zip(self.rows, self.points) if r.cls == we.VALID]
        self.bad = [r for r in self.rows if r.cls != we.VALID]
        assert self.bad and all(not ok for r, (_, ok) in zip(self.rows, self.want) if r.cls != we.VALID)
        self.edges = [(r, P) for r, P in zip(self.rows, self.points) if r.label.startswith(("min-x", "max-x", "x=0"))]

    def live(self):
        return self.ctx.memory_stats()["live_bytes"]

    def from_bytetree(self, bt):
        """vmn_garray_from_bytetree as it is: (array | None, format_ok, all_in_range) -- the wrapper raises on either flag."""
        h, fmt, rng = C.c_void_p(), C.c_int(0), C.c_int(1)
        self.vmn._check(self.vmn.lib().vmn_garray_from_bytetree(self.G._h, bt, C.c_size_t(len(bt)), C.c_size_t(0), C.byref(h),
                                                                C.byref(fmt), C.byref(rng)))
        return (self.vmn.PGroupElementArray(self.G, h) if h else None), bool(fmt.value), bool(rng.value)

    def enc(self, points):
        """The canonical encoding of affine points at the group's width (leading zero bytes above the bytes of p)."""
        return b"".join(b"\xff" * (2 * self.nb) if P is None else P[0].to_bytes(self.nb, "big") + P[1].to_bytes(self.nb, "big")
                        for P in points)

    def as_rows(self, points):
        return [we.Row("", we.VALID, e[:self.nb], e[self.nb:]) for e in (self.enc([P]) for P in points)]

    def close(self):
        self.G.close()


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def case(request, vmn, gpu_ctx):
    name, width = request.param
    c = Case(vmn, gpu_ctx, name, java=width == "java")
    assert c.nb == we.widths(name)[width]
    yield c
    c.close()


# ---- flat import -------------------------------------------------------------------------------------------------------
def test_flat_import_of_the_whole_catalogue(case):
    G = case.G
    arr = G.toElementArray(we.flat(case.rows), checked=False)
    assert arr.size() == len(case.rows)
    got = arr.toInts()
    wrong = [r.label for r, g, w in zip(case.rows, got, case.points) if g != w]
    assert not wrong, wrong
    assert arr.all_in_range is False
    with pytest.raises(ValueError):
        G.toElementArray(we.flat(case.rows))
    for r in case.bad:                                      # each bad row alone
        one = G.toElementArray(r.x + r.y, checked=False)
        assert one.all_in_range is False and one.toInts() == [None], r.label
        with pytest.raises(ValueError):
            G.toElementArray(r.x + r.y)
    ok = G.toElementArray(we.flat(case.valid))
    assert ok.all_in_range is True and ok.toInts() == case.valid_points
    for r, P in zip(case.valid, case.valid_points):         # and each valid row alone
        one = G.toElementArray(r.x + r.y, checked=False)
        assert one.all_in_range is True and one.toInts() == [P], r.label


# ---- one bad entry among a block's lanes -----------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=POSITION_CURVES)
def position_case(request, vmn, gpu_ctx):
    c = Case(vmn, gpu_ctx, request.param)
    yield c
    c.close()


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_one_alias_row_at_the_lanes_that_end_a_wave_and_a_block(position_case, n):
    """The verdict is one atomicOr from any lane: a single alias row first, last in a wave, first in the next, and last of an
    array around a wave and a block -- flag raised, that entry the identity, every other entry untouched."""
    case = position_case
    G = case.G
    base = case.f["kG"][:n]                                 # k G, k = 1 .. n (computed once per curve)
    good = case.enc(base)
    alias = next(r for r in case.rows if r.label == "alias-x+")
    w = 2 * case.nb
    for at in sorted({0, 63, 64, n - 1}):
        if at >= n:
            continue
        arr = G.toElementArray(good[:at * w] + alias.x + alias.y + good[(at + 1) * w:], checked=False)
        assert arr.all_in_range is False, at
        got = arr.toInts()
        assert got[at] is None and got[:at] == base[:at] and got[at + 1:] == base[at + 1:], at
    arr = G.toElementArray(good, checked=False)
    assert arr.all_in_range is True and arr.toInts() == base


# ---- framed import and export -------------------------------------------------------------------------------------------
def test_framed_import_is_the_flat_import(case):
    G = case.G
    arr, fmt, rng = case.from_bytetree(we.framed(case.rows))
    assert fmt and not rng and arr is not None
    got = arr.toInts()
    wrong = [r.label for r, g, w in zip(case.rows, got, case.points) if g != w]
    assert not wrong, wrong
    with pytest.raises(ValueError, match="ArithmFormatException"):
        G.toElementArrayFromByteTree(we.framed(case.rows))
    for r in case.bad:
        one, fmt, rng = case.from_bytetree(we.framed([r]))
        assert fmt and not rng and one.toInts() == [None], r.label
    ok = G.toElementArrayFromByteTree(we.framed(case.valid))
    assert ok.toInts() == case.valid_points
    assert G.toElementArrayFromByteTree(we.framed(case.valid), len(case.valid)).size() == len(case.valid)


def test_framed_export_is_byte_identical(case):
    """toByteTree() of the valid rows is framed() of their canonical encodings (zero leading bytes at the Java width), from
    rows with Z = 1 and from rows with Z != 1."""
    G = case.G
    X = G.toElementArray(we.flat(case.valid))
    assert we.flat(case.valid) == case.enc(case.valid_points)                # the valid rows are canonical as they stand
    bt = X.toByteTree()
    assert bt == we.framed(case.valid) and X.byteTreeSize() == len(bt)
    four = [case.c.mul(4, P) for P in case.valid_points]
    J = X.exp(3).mul(X)                                                       # Z != 1
    assert J.toByteTree() == we.framed(case.as_rows(four))
    assert G.toElementArrayFromByteTree(bt).toByteTree() == bt


def test_header_mutants_are_format_errors(case):
    G = case.G
    good = we.framed(case.valid)
    G.toElementArrayFromByteTree(good).free()               # (warm: scratch and pool blocks of this size exist)
    live0 = case.live()
    for label, bt in we.header_mutants(case.valid, case.nb):
        with pytest.raises(ValueError, match="EIOException"):
            G.toElementArrayFromByteTree(bt)
        arr, fmt, _ = case.from_bytetree(bt)
        assert arr is None and not fmt, label
        assert case.live() == live0, label
    # the outer header: wrong tag, a count that disagrees with the length, a length that disagrees with the count
    for bt in (b"\x01" + good[1:], good[:4] + bytes([good[4] + 1]) + good[5:], good[:-1], good + b"\x00"):
        with pytest.raises(ValueError, match="EIOException"):
            G.toElementArrayFromByteTree(bt)
        assert case.live() == live0
    assert G.toElementArrayFromByteTree(good).toInts() == case.valid_points


# ---- the four export paths --------------------------------------------------------------------------------------------------
def test_export_paths_agree(case, monkeypatch):
    """The device kernel (five points or more), the host path (four or fewer), the device kernel forced on four or fewer, and
    the export that normalises the rows first -- and get(i) -- all give the oracle's affine point at the group's width, from
    rows with Z = 1 and with Z != 1."""
    G, c = case.G, case.c
    X = G.toElementArray(we.flat(case.valid))
    J = X.exp(3).mul(X)
    for arr, want in ((X, case.valid_points), (J, [c.mul(4, P) for P in case.valid_points])):
        n = len(want)
        assert n >= 5
        full = case.enc(want)
        w = 2 * case.nb
        chunks = [(lo, min(lo + 4, n)) for lo in range(0, n, 4)] + [(n - 1, n), (0, 3)]
        parts = [(lo, hi, arr.copyOfRange(lo, hi)) for lo, hi in chunks]
        assert arr.toBytes() == full                                           # device kernel
        for lo, hi, part in parts:
            assert part.toBytes() == full[lo * w:hi * w], (lo, hi)             # host path
        assert [arr.get(i) for i in range(n)] == want
        monkeypatch.setenv("VMN_EC_EXPORT_DEVICE", "1")
        for lo, hi, part in parts:
            assert part.toBytes() == full[lo * w:hi * w], (lo, hi)             # device kernel on four or fewer
        assert [arr.get(i) for i in range(n)] == want
        monkeypatch.delenv("VMN_EC_EXPORT_DEVICE")
        monkeypatch.setenv("VMN_EC_EXPORT_NORMALISE_MIN", "1")
        assert arr.toBytes() == full                                           # rows normalised first
        assert arr.toByteTree() == b"\x00" + n.to_bytes(4, "big") + b"".join(
            we.framed_point(full[i * w:i * w + case.nb], full[i * w + case.nb:(i + 1) * w]) for i in range(n))
        monkeypatch.setenv("VMN_EC_EXPORT_DEVICE", "1")
        for lo, hi, part in parts:
            assert part.toBytes() == full[lo * w:hi * w], (lo, hi)
        monkeypatch.delenv("VMN_EC_EXPORT_DEVICE")
        monkeypatch.delenv("VMN_EC_EXPORT_NORMALISE_MIN")


# ---- single elements -------------------------------------------------------------------------------------------------------
def test_single_elements(case):
    """shiftPush(el) and G.exp(base, E) import one element (import_one): every bad row is the library's format error, nothing
    stays allocated and the array works afterwards; the valid edge rows pass."""
    G, c, vmn = case.G, case.c, case.vmn
    base = case.f["kG"][:6]
    X = G.toElementArray(base)
    es = [1, 2, c.n - 1, 0, 3]
    E = G.ringArray(es)
    X.shiftPush(c.g).free()
    live0 = case.live()
    for r in case.bad:
        for call in (lambda: X.shiftPush(ints(r)), lambda: G.exp(ints(r), E)):
            with pytest.raises(vmn.VmnError) as ei:
                call()
            assert ei.value.status == VMN_ERR_FORMAT, r.label
            assert case.live() == live0, r.label
    assert X.toInts() == base
    identity = next(r for r in case.rows if r.label == "identity")
    for r, P in case.edges + [(identity, None)]:
        assert X.shiftPush(ints(r)).toInts() == [P] + base[:-1], r.label
    for r, P in case.edges:
        assert G.exp(ints(r), E).toInts() == [c.mul(e, P) for e in es], r.label
        G.releaseFixed(ints(r))


# ---- the widths around the framed import's old buffer ----------------------------------------------------------------------
@pytest.mark.parametrize("width", ["buffer", "beyond"])
@pytest.mark.parametrize("name", BEYOND_CURVES)
def test_widths_around_the_old_framed_buffer(vmn, gpu_ctx, name, width):
    """Coordinates of 4 NW + 4 and 4 NW + 5 bytes (vmn_group_set_wire_bytes takes any width up to 4096): the framed import
    once moved both coordinates into a per-thread buffer of 2 (4 NW + 4) bytes and refused anything wider, so a group of
    4 NW + 5-byte coordinates wrote byte trees it could not read back (seen on an MI355X before the fix: format_ok = 0 on the
    tree the group had just exported, 37 bytes over P-256 and 73 over brainpoolp512r1; 36 and 72 bytes passed).  It reads the
    coordinates where they lie now: both widths behave like every other."""
    case = Case(vmn, gpu_ctx, name, nbytes=we.widths(name)[width])
    try:
        G = case.G
        assert case.nb == we.widths(name)[width] == 4 * case.f["NW"] + (4 if width == "buffer" else 5)
        assert {"alias-x+", "alias-y", "lead-01-x", "lead-80-x", "lead-01-y", "lead-80-y"} <= {r.label for r in case.bad}
        X = G.toElementArray(we.flat(case.valid))
        assert X.toInts() == case.valid_points and X.toBytes() == we.flat(case.valid)
        bt = X.toByteTree()
        assert bt == we.framed(case.valid)
        back, fmt, rng = case.from_bytetree(bt)
        assert fmt, "the group cannot read the byte tree it wrote"
        assert rng and back.toInts() == case.valid_points and back.toByteTree() == bt
        flat = G.toElementArray(we.flat(case.rows), checked=False)
        tree, fmt, rng = case.from_bytetree(we.framed(case.rows))
        assert fmt and not rng and flat.all_in_range is False
        assert flat.toInts() == case.points == tree.toInts()
        for r in case.bad:
            if r.cls in (we.ALIAS, we.LEAD):
                above = (int.from_bytes(r.x, "big") | int.from_bytes(r.y, "big")) >> (32 * case.f["NW"])
                assert above or r.cls == we.ALIAS             # (an alias of a prime shorter than the packed words stays within them)
                one, fmt, rng = case.from_bytetree(we.framed([r]))
                assert fmt and not rng and one.toInts() == [None], r.label
                assert G.toElementArray(r.x + r.y, checked=False).all_in_range is False, r.label
        for label, m in we.header_mutants(case.valid, case.nb):
            arr, fmt, _ = case.from_bytetree(m)
            assert arr is None and not fmt, label
    finally:
        case.close()


# ---- edge points as operands -------------------------------------------------------------------------------------------------
def test_edge_points_as_operands(case):
    """The points of smallest and largest x and (0, +-sqrt b) -- a zero X limb vector, x = p - 1 or next to it -- through the
    group operations, against the oracle's affine arithmetic."""
    G, c = case.G, case.c
    pts = [P for _, P in case.edges] + [c.g, None]
    n = len(pts)
    others = (case.f["kG"][1:n] + [c.g])[:n]
    X, Y = G.toElementArray(pts), G.toElementArray(others)
    assert X.mul(Y).toInts() == c.mul_arrays(pts, others)
    assert Y.mul(X).toInts() == c.mul_arrays(pts, others)
    assert X.mul(X).toInts() == [c.add(P, P) for P in pts]
    neg = [c.neg(P) for P in pts]
    N = X.inv()
    assert N.toInts() == neg
    assert X.mul(N).toInts() == [None] * n and N.mul(X).toInts() == [None] * n
    assert X.exp(2).toInts() == [c.add(P, P) for P in pts]
    assert X.exp(c.n - 1).toInts() == neg
    es = ([1, c.n - 1, 2, 3, c.n - 2, 5, 4, 6] * 2)[:n]
    E = G.ringArray(es)
    small = [e if e < 8 else e - c.n for e in es]             # (n - k acts as -k: the oracle multiplies by k and negates)
    powers = [c.mul(k, P) if k >= 0 else c.neg(c.mul(-k, P)) for k, P in zip(small, pts)]
    assert X.exp(E).toInts() == powers
    assert X.expProd(E) == c.prod(powers)
    assert X.prod() == c.prod(pts)
