"""GPU suite: vmn_garray_from_segments (csrc/light_kernels.h k_rows_segments) and the reference's `vre` on top of it
(verificatum_vmn_amd/rearrange.py, tools/vre.py).

The expected values of the array call are the SOURCES' exported big-endian bytes (vmn_garray_to_be), sliced and joined with numpy
on the host; the expected files are assembled on the host from Python values by tests/keyed_layout_ref.py.  Neither comes from the
function under test.  After every call the sources export the bytes they exported before.

The large case.  light_grid launches at most num_cus * 8 workgroups of 256 threads, one thread per 16-byte chunk, and a
grid-stride loop takes the rest.  A row of a 2048-bit group holds one 32-bit word per 28-bit limb, 74 limbs padded to 76 words =
19 chunks (at least 74 / 4 rounded up whatever the padding).  On an MI355X num_cus = 256: the cap is 256 * 8 * 256 = 524 288
threads, and 30 000 rows are 30 000 * 19 = 570 000 chunks (9.1 MB), so 45 712 threads copy a second chunk.  The test asserts
30 000 * 19 > num_cus * 8 * 256 from the context's own num_cus.

Wall time on an MI355X (one run, pytest's call durations): the 90 cases of the module take 2.5 s; the tool's case (three
processes) 1.1 s, the cases of 65 536 segments 0.03 - 0.09 s, the large case 0.05 s, every other case at most 0.03 s."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden

import keyed_layout_ref as KL
from named_curves import ref_curve

pytestmark = pytest.mark.gpu

GROUPS = ["modp512", "modp2048", "modp3072", "P-256", "P-521"]
VMN_ERR_ARG = -1


def make_group(vmn, ctx, name):
    from oracle import pyref
    if name.startswith("modp"):
        bits = int(name[4:])
        if bits == 512:
            g, _ = load_golden(512)
            return vmn.ModPGroup(ctx, g["p"], g["q"], g["g"])
        p, q, g = pyref.modp_group(bits)
        return vmn.ModPGroup(ctx, p, q, g)
    return vmn.ECqPGroup(ctx, name, java_widths=True)


def rows_of(G, name, n, salt):
    """n rows of elem_bytes as a numpy array: numbers below the modulus (the array call moves rows, it does not ask for members),
    points of the curve."""
    eb = G.elem_bytes
    if name.startswith("modp"):
        rows = np.random.Generator(np.random.PCG64(salt)).integers(0, 256, size=(n, eb), dtype=np.uint8)
        rows[:, :eb - (G.p.bit_length() - 1) // 8] = 0                 # below 2^(8 k) <= 2^(bits - 1) < p
        rows[:, -1] |= 1
        return rows
    c, acc, pool = ref_curve(name), None, []
    for _ in range(23):
        acc = c.add(acc, c.g)
        pool.append(np.frombuffer(G.enc_el(acc), dtype=np.uint8))
    return np.stack([pool[(7 * i + salt) % 23] for i in range(n)])


class Sources:
    def __init__(self, vmn, ctx, name):
        self.G = make_group(vmn, ctx, name)
        self.eb = self.G.elem_bytes
        self.host = {"A": rows_of(self.G, name, 300, 1), "B": rows_of(self.G, name, 70, 2), "C": rows_of(self.G, name, 3, 3)}
        self.dev = {k: self.G.toElementArray(v.tobytes()) for k, v in self.host.items()}
        # the reference of every test: what the sources export, taken once
        self.be = {k: np.frombuffer(a.toBytes(), dtype=np.uint8).reshape(-1, self.eb).copy() for k, a in self.dev.items()}
        for k in self.be:
            assert np.array_equal(self.be[k], self.host[k]), k

    def check(self, segs):
        out = self.G.fromSegments([self.dev[k] for k, _, _ in segs], [f for _, f, _ in segs], [t for _, _, t in segs])
        parts = [self.be[k][f:t] for k, f, t in segs]
        want = np.concatenate(parts) if parts else np.zeros((0, self.eb), dtype=np.uint8)
        assert out.size() == len(want)
        got = np.frombuffer(out.toBytes(), dtype=np.uint8).reshape(-1, self.eb)
        assert np.array_equal(got, want), [(i, k) for i, k in enumerate(np.flatnonzero((got != want).any(axis=1))[:5])]
        out.free()
        for k, a in self.dev.items():                                   # the sources are read only
            assert a.size() == len(self.be[k]) and a.toBytes() == self.be[k].tobytes(), k

    def close(self):
        for a in self.dev.values():
            a.free()
        self.G.close()


@pytest.fixture(scope="module", params=GROUPS)
def src(request, vmn, gpu_ctx):
    s = Sources(vmn, gpu_ctx, request.param)
    yield s
    s.close()


SHAPES = {
    "whole-array": [("A", 0, 300)],
    "one-row-segments": [("A", 5, 6), ("B", 0, 1), ("A", 299, 300), ("C", 2, 3)],
    "empty-first-middle-last": [("A", 0, 0), ("B", 3, 10), ("A", 7, 7), ("C", 3, 3), ("C", 0, 3), ("B", 70, 70)],
    "all-empty": [("A", 0, 0), ("B", 5, 5), ("C", 3, 3)],
    "no-segments": [],
    "one-source-twice-overlapping": [("A", 0, 50), ("A", 25, 75), ("A", 0, 50), ("A", 74, 76)],
    "ends-at-63-64-65-255-256-257": [("A", 0, 63), ("B", 0, 1), ("B", 1, 2), ("A", 10, 200), ("C", 0, 1), ("C", 1, 2), ("A", 0, 5)],
    "concat": [("A", 0, 300), ("B", 0, 70), ("C", 0, 3)],
}


def test_the_boundary_shape_ends_where_it_says():
    ends = np.cumsum([t - f for _, f, t in SHAPES["ends-at-63-64-65-255-256-257"]]).tolist()
    assert ends[:6] == [63, 64, 65, 255, 256, 257]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_from_segments_is_the_host_slices_joined(src, shape):
    src.check(SHAPES[shape])


@pytest.mark.parametrize("nseg", [1, 2, 257, 65536])
def test_many_segments_of_one_row_out_of_three(src, nseg):
    src.check([("C", k % 3, k % 3 + 1) for k in range(nseg)])


def counted(ctx, fn):
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        out = fn()
        return out, {name: row[0] for name, row in ctx.timing_report().items() if row[0]}
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()


def test_one_launch_per_array_whatever_the_segments_and_none_for_an_empty_result(src, gpu_ctx):
    G, A, C3 = src.G, src.dev["A"], src.dev["C"]
    for segs in ([(A, 0, 300)], [(A, 0, 10), (C3, 0, 3)], [(C3, k % 3, k % 3 + 1) for k in range(257)]):
        out, counts = counted(gpu_ctx, lambda: G.fromSegments([a for a, _, _ in segs], [f for _, f, _ in segs], [t for _, _, t in segs]))
        assert counts.get("segments") == 1, (len(segs), counts)
        out.free()
    out, counts = counted(gpu_ctx, lambda: G.fromSegments([A, C3], [4, 1], [4, 1]))
    assert out.size() == 0 and "segments" not in counts, counts
    out.free()
    out, counts = counted(gpu_ctx, lambda: G.concat([A, C3]))
    assert out.size() == 303 and counts.get("segments") == 1
    out.free()


def test_the_stride_loop_runs(vmn, gpu_ctx):
    """30 000 rows of the 2048-bit group: more 16-byte chunks than light_grid launches threads (the module's head)."""
    n = 30000
    assert n * 19 > gpu_ctx.num_cus * 8 * 256, gpu_ctx.num_cus
    G = make_group(vmn, gpu_ctx, "modp2048")
    host = rows_of(G, "modp2048", n, 5)
    big, small = G.toElementArray(host.tobytes()), G.toElementArray(host[:3].tobytes())
    be = np.frombuffer(big.toBytes(), dtype=np.uint8).reshape(n, G.elem_bytes).copy()
    assert np.array_equal(be, host)
    for segs in ([(big, 0, n)], [(big, 1, 12345), (small, 0, 3), (big, 12000, n), (small, 1, 1), (big, 0, 1)]):
        out = G.fromSegments([a for a, _, _ in segs], [f for _, f, _ in segs], [t for _, _, t in segs])
        want = np.concatenate([(be if a is big else be[:3])[f:t] for a, f, t in segs])
        assert out.size() == len(want) and out.toBytes() == want.tobytes()
        out.free()
    assert big.toBytes() == be.tobytes()
    big.free()
    small.free()
    G.close()


def raw_call(vmn, G, handles, froms, tos, nseg=None):
    k = len(handles)
    hs = (C.c_void_p * max(k, 1))(*handles)
    lo = (C.c_size_t * max(k, 1))(*froms)
    hi = (C.c_size_t * max(k, 1))(*tos)
    out = C.c_void_p(0xdead)
    rc = vmn.lib().vmn_garray_from_segments(G._h, hs, lo, hi, C.c_size_t(k if nseg is None else nseg), C.byref(out))
    return rc, out.value


def test_argument_errors_give_no_array(vmn, gpu_ctx, src):
    G, A, B = src.G, src.dev["A"], src.dev["B"]
    assert raw_call(vmn, G, [A._h, B._h], [0, 0], [300, 71]) == (VMN_ERR_ARG, None)               # to > n
    assert raw_call(vmn, G, [A._h, B._h], [0, 5], [300, 4]) == (VMN_ERR_ARG, None)                # from > to
    assert raw_call(vmn, G, [A._h, None], [0, 0], [300, 0]) == (VMN_ERR_ARG, None)                # a null source
    assert raw_call(vmn, G, [A._h] * 65537, [0] * 65537, [1] * 65537) == (VMN_ERR_ARG, None)      # nseg = 65 537
    other = make_group(vmn, gpu_ctx, "modp512" if src.G.coord_bytes is not None else "P-256")
    alien = other.toElementArray([other.g] * 4)
    assert raw_call(vmn, G, [A._h, alien._h], [0, 0], [1, 1]) == (VMN_ERR_ARG, None)              # a source of another group
    alien.free()
    other.close()
    rc, h = raw_call(vmn, G, [A._h] * 65536, [0] * 65536, [1] * 65536)                            # 65 536 is allowed
    assert rc == 0 and h
    vmn.lib().vmn_garray_free(C.c_void_p(h))
    with pytest.raises(vmn.VmnError):
        G.fromSegments([A], [0], [301])
    with pytest.raises(ValueError):
        G.fromSegments([A, B], [0], [1, 2])
    src.check(SHAPES["concat"])                                                                   # and the sources are what they were


# ---- files: n = 10 on the 512-bit group and on P-256 ------------------------------------------------------------------------------
N = 10


class FileCase:
    """One group, a pool of its members as Python values, and lists of them as columns."""

    def __init__(self, vmn, ctx, name):
        from oracle import pyref
        self.curve = name != "modp512"
        self.G = make_group(vmn, ctx, name)
        if self.curve:
            c, acc, self.pool = ref_curve(name), None, []
            for _ in range(41):
                acc = c.add(acc, c.g)
                self.pool.append(acc)
        else:
            p = self.G.p
            self.pool = [pow(2 + v % (p - 3), 2, p) for v in pyref.stream_ints(b"rearrange", 41, p)]
        self.vb = self.G.nbytes

    def columns(self, count, n=N, salt=0):
        L = len(self.pool)
        return [[self.pool[(5 * i + 11 * c + salt) % L] for i in range(n)] for c in range(count)]

    def outsider(self):
        """An element of the right shape outside the group: a non-residue; a point off the curve."""
        if self.curve:
            x, y = self.pool[0]
            return (x, y ^ 1)
        return self.G.p - self.pool[0]                    # p = 3 mod 4: -1 is a non-residue

    def list_file(self, path, cols, kw, ciphs=True):
        tree = KL.list_tree(self.curve, self.vb, kw, cols) if ciphs else KL.wide_array_tree(self.curve, self.vb, kw, cols)
        with open(path, "wb") as f:
            f.write(tree)
        return tree


@pytest.fixture(scope="module", params=["modp512", "P-256"])
def case(request, vmn, gpu_ctx):
    c = FileCase(vmn, gpu_ctx, request.param)
    yield c
    c.G.close()


@pytest.fixture(scope="module")
def rear(vmn):
    from verificatum_vmn_amd import rearrange
    return rearrange


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("ciphs", [True, False])
def test_sub_then_cat_gives_the_input_file_again(case, rear, tmp_path, ciphs):
    kw, w = (2, 2) if ciphs else (1, 1)
    cols = case.columns((2 if ciphs else 1) * kw * w)
    p = lambda n: str(tmp_path / n)
    whole = case.list_file(p("in"), cols, kw, ciphs)
    rear.sub_files(case.G, p("in"), [p("a"), p("b")], rear.parse_intervals("0-3:3-10"), w, kw, ciphs)
    assert read(p("a")) == case.list_file(p("want"), [c[0:3] for c in cols], kw, ciphs)
    assert read(p("b")) == case.list_file(p("want"), [c[3:10] for c in cols], kw, ciphs)
    rear.cat_files(case.G, [p("a"), p("b")], p("out"), w, kw, ciphs)
    assert read(p("out")) == whole
    # intersecting intervals are the host's slices
    rear.sub_files(case.G, p("in"), [p("c"), p("d")], rear.parse_intervals("2-7:5-9"), w, kw, ciphs)
    assert read(p("c")) == case.list_file(p("want"), [c[2:7] for c in cols], kw, ciphs)
    assert read(p("d")) == case.list_file(p("want"), [c[5:9] for c in cols], kw, ciphs)
    # an empty input is allowed in -cat
    case.list_file(p("none"), [[] for _ in cols], kw, ciphs)
    rear.cat_files(case.G, [p("none"), p("a"), p("none"), p("b")], p("out2"), w, kw, ciphs)
    assert read(p("out2")) == whole


def test_shallow_is_the_file_assembled_from_the_inputs_component_trees(case, rear, tmp_path):
    kw = 1
    a, b = case.columns(6), case.columns(2, salt=3)                       # ciphertexts of widths 3 and 1
    p = lambda n: str(tmp_path / n)
    case.list_file(p("a"), a, kw)
    case.list_file(p("b"), b, kw)
    rear.shallow_files(case.G, [p("a"), p("b")], [p("o0"), p("o1")], [3, 1], kw, rear.parse_format("(0,2)x(1,0):(0,0-2)"), True)
    assert read(p("o0")) == KL.list_tree(case.curve, case.vb, kw, [a[2], b[0], a[5], b[1]])
    assert read(p("o1")) == KL.list_tree(case.curve, case.vb, kw, [a[0], a[1], a[3], a[4]])
    # under a key of width 2 a position is two arrays
    a2, b2 = case.columns(12, salt=5), case.columns(4, salt=7)
    case.list_file(p("a2"), a2, 2)
    case.list_file(p("b2"), b2, 2)
    rear.shallow_files(case.G, [p("a2"), p("b2")], [p("o2")], [3, 1], 2, rear.parse_format("(0,2)x(1,0)"), True)
    assert read(p("o2")) == KL.list_tree(case.curve, case.vb, 2, [a2[4], a2[5], b2[0], b2[1], a2[10], a2[11], b2[2], b2[3]])


@pytest.mark.parametrize("ciphs", [False, True])
def test_deep_joins_keywidths_one_and_two_into_three_and_back(case, rear, interface, tmp_path, ciphs):
    w, nests = 2, (2 if ciphs else 1)
    a, b = case.columns(nests * w, salt=1), case.columns(nests * 2 * w, salt=2)
    p = lambda n: str(tmp_path / n)
    fa, fb = case.list_file(p("a"), a, 1, ciphs), case.list_file(p("b"), b, 2, ciphs)
    rear.deep_files(case.G, [p("a"), p("b")], [p("joint")], [1, 2], w, rear.parse_format("(0,0)x(1,0-2)"), ciphs)
    want = []
    for h in range(nests):
        for l in range(w):
            want += [a[h * w + l], b[h * 2 * w + 2 * l], b[h * 2 * w + 2 * l + 1]]
    assert read(p("joint")) == case.list_file(p("want"), want, 3, ciphs)
    rear.deep_files(case.G, [p("joint")], [p("a.back"), p("b.back")], [3], w, rear.parse_format("(0,0):(0,1-3)"), ciphs)
    assert read(p("a.back")) == fa and read(p("b.back")) == fb
    if ciphs:                                                           # the joined list is a list under a key of width 3
        back = interface.read_ciphertexts(case.G, p("joint"), w, "raw", keywidth=3)
        assert back is not None and [x.toInts() for x in back] == want
        for x in back:
            x.free()


@pytest.fixture(scope="module")
def interface(vmn):
    from verificatum_vmn_amd import interface
    return interface


def test_deep_joined_list_is_accepted_at_keywidth_two(case, rear, interface, tmp_path):
    a, b = case.columns(2, salt=1), case.columns(2, salt=2)
    p = lambda n: str(tmp_path / n)
    case.list_file(p("a"), a, 1)
    case.list_file(p("b"), b, 1)
    rear.deep_files(case.G, [p("a"), p("b")], [p("joint")], [1, 1], 1, rear.parse_format("(0,0)x(1,0)"), True)
    back = interface.read_ciphertexts(case.G, p("joint"), 1, "raw", keywidth=2)
    assert back is not None and [x.toInts() for x in back] == [a[0], b[0], a[1], b[1]]
    for x in back:
        x.free()


def test_pkeys_makes_a_key_of_width_two_from_two_keys(case, rear, tmp_path):
    from types import SimpleNamespace
    from verificatum_vmn_amd import proofdir
    G, (g, y0, y1, y2) = case.G, [case.G.g] + case.pool[:3]
    p = lambda n: str(tmp_path / n)
    with open(p("k0"), "wb") as f:
        f.write(KL.public_key_tree(case.curve, case.vb, 1, g, [y0]))
    with open(p("k12"), "wb") as f:
        f.write(KL.public_key_tree(case.curve, case.vb, 2, g, [y1, y2]))
    assert rear.pkey_keywidth(G, read(p("k0"))) == 1 and rear.pkey_keywidth(G, read(p("k12"))) == 2
    rear.pkeys_files(G, [p("k0"), p("k12")], [p("wide"), p("three"), p("pair")], rear.parse_format("(0,0)x(1,1):(0,0)x(1,0-2):(1,1)"))
    assert read(p("wide")) == KL.public_key_tree(case.curve, case.vb, 2, g, [y0, y2])
    assert read(p("three")) == KL.public_key_tree(case.curve, case.vb, 3, g, [y0, y1, y2])
    assert read(p("pair")) == KL.public_key_tree(case.curve, case.vb, 1, g, [y2])                # a plain pair, no node of width 1
    got = proofdir._gpu_read_pkey(SimpleNamespace(grp=G, keywidth=2), p("wide"))
    assert got == [(g, g), (y0, y2)]
    # a key holding an element outside the group: an error naming the file, no output
    with open(p("bad"), "wb") as f:
        f.write(KL.public_key_tree(case.curve, case.vb, 1, g, [case.outsider()]))
    with pytest.raises(rear.RearrangeInputError, match="bad"):
        rear.pkeys_files(G, [p("k0"), p("bad")], [p("no")], rear.parse_format("(0,0)x(1,0)"))
    assert not os.path.exists(p("no"))


def test_refusals_create_no_output(case, rear, tmp_path):
    p = lambda n: str(tmp_path / n)
    cols = case.columns(2)
    case.list_file(p("good"), cols, 1)
    bad = [list(c) for c in cols]
    bad[1][4] = case.outsider()
    case.list_file(p("bad"), bad, 1)
    case.list_file(p("nine"), [c[:9] for c in cols], 1)
    outs = [p("o1"), p("o2")]
    # an input holding an element outside the group
    with pytest.raises(rear.RearrangeInputError, match="bad") as exc:
        rear.sub_files(case.G, p("bad"), outs, [(0, 3), (3, 10)], 1, 1, True)
    assert exc.value.path == p("bad")
    with pytest.raises(rear.RearrangeInputError, match="bad"):
        rear.cat_files(case.G, [p("good"), p("bad")], outs[0], 1, 1, True)
    with pytest.raises(rear.RearrangeInputError, match="bad"):
        rear.shallow_files(case.G, [p("good"), p("bad")], outs, [1, 1], 1, rear.parse_format("(0,0):(1,0)"), True)
    with pytest.raises(rear.RearrangeInputError, match="bad"):
        rear.deep_files(case.G, [p("good"), p("bad")], outs[:1], [1, 1], 1, rear.parse_format("(0,0)x(1,0)"), True)
    # a missing input, and one that is no tree of the stated shape
    with pytest.raises(rear.RearrangeInputError, match="missing"):
        rear.cat_files(case.G, [p("good"), p("missing")], outs[0], 1, 1, True)
    with pytest.raises(rear.RearrangeInputError, match="good"):
        rear.sub_files(case.G, p("good"), outs, [(0, 3), (3, 10)], 2, 1, True)
    with pytest.raises(rear.RearrangeInputError, match="good"):
        rear.sub_files(case.G, p("good"), outs, [(0, 3), (3, 10)], 1, 1, False)
    # an interval beyond the size: checked before anything is written, the first interval included
    with pytest.raises(rear.RearrangeFormatError) as exc:
        rear.sub_files(case.G, p("good"), outs, [(0, 3), (3, 11)], 1, 1, True)
    assert str(exc.value) == "Interval out of bounds! 3-11. Length of array is 10!"
    # inputs of lengths 10 and 9
    with pytest.raises(rear.RearrangeFormatError, match="differ in length"):
        rear.shallow_files(case.G, [p("good"), p("nine")], outs, [1, 1], 1, rear.parse_format("(0,0)x(1,0):(1,0)"), True)
    with pytest.raises(rear.RearrangeFormatError, match="differ in length"):
        rear.deep_files(case.G, [p("good"), p("nine")], outs[:1], [1, 1], 1, rear.parse_format("(0,0)x(1,0)"), True)
    # a count of outputs that differs from the format's; a position that does not exist
    with pytest.raises(rear.RearrangeFormatError):
        rear.shallow_files(case.G, [p("good")], outs, [1], 1, rear.parse_format("(0,0)"), True)
    with pytest.raises(rear.RearrangeFormatError, match="index 1"):
        rear.shallow_files(case.G, [p("good")], outs[:1], [1], 1, rear.parse_format("(0,1)"), True)
    assert not any(os.path.exists(o) for o in outs)


# ---- the tool's reason to exist (the reference's help text, ProtocolElGamalRearTool.java:734-739) ---------------------------------
def test_join_under_two_keys_permute_extract_and_open_under_the_first_secret(vmn, gpu_ctx, rear):
    g512, _ = load_golden(512)
    p, q, g = g512["p"], g512["q"], g512["g"]
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    n = 5
    x = [0x1234567 % q, 0x7654321 % q]
    y = [pow(g, xi, p) for xi in x]
    msgs = [[pow(g, 100 * k + i + 2, p) for i in range(n)] for k in range(2)]
    r = [[(977 * k + 31 * i + 5) % q for i in range(n)] for k in range(2)]
    lists = []
    for k in range(2):                                                     # list k: width 1 under the single key y_k
        u = [pow(g, r[k][i], p) for i in range(n)]
        v = [msgs[k][i] * pow(y[k], r[k][i], p) % p for i in range(n)]
        lists.append([G.toElementArray(u), G.toElementArray(v)])
    (joint,) = rear.rearrange_deep(lists, [1, 1], 1, rear.parse_format("(0,0)x(1,0)"), True)
    assert len(joint) == 4                                                 # one list under the combined key of width 2
    perm = [3, 0, 4, 1, 2]
    mixed = [a.permute(perm) for a in joint]                               # permuted as ONE list
    (first,) = rear.rearrange_deep([mixed], [2], 1, rear.parse_format("(0,0)"), True)
    assert len(first) == 2
    ux = first[0].exp(x[0])
    inv = ux.inv()
    opened = first[1].mul(inv)                                             # v * u^(-x) under the first secret alone
    assert opened.toInts() == [msgs[0][perm[i]] for i in range(n)]
    # the other half stays closed to the first secret and opens to the second
    (second,) = rear.rearrange_deep([mixed], [2], 1, rear.parse_format("(0,1)"), True)
    ux2 = second[0].exp(x[1])
    inv2 = ux2.inv()
    opened2 = second[1].mul(inv2)
    assert opened2.toInts() == [msgs[1][perm[i]] for i in range(n)]
    for a in lists[0] + lists[1] + joint + mixed + first + second + [ux, inv, opened, ux2, inv2, opened2]:
        a.free()
    G.close()


# ---- the tool, once, over P-256 (it names a modular group by its RFC 3526 size, which the 512-bit golden group is not) -------------
def test_the_tool_splits_joins_and_refuses(vmn, gpu_ctx, tmp_path):
    case = FileCase(vmn, gpu_ctx, "P-256")
    p = lambda n: str(tmp_path / n)
    cols = case.columns(4)                                                 # width 1 under a key of width 2
    whole = case.list_file(p("in"), cols, 2)
    with open(p("pk"), "wb") as f:
        f.write(KL.public_key_tree(True, case.vb, 2, case.G.g, case.pool[:2]))
    case.G.close()
    tool = [sys.executable, os.path.join(ROOT, "tools", "vre.py"), "--curve", "P-256", "-ciphs"]
    out = subprocess.run(tool + ["-sub", "-inter", "0-3:3-10", p("pk"), p("in"), p("a"), p("b")], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert read(p("a")) == KL.list_tree(True, case.vb, 2, [c[:3] for c in cols])
    out = subprocess.run(tool + ["-cat", p("pk"), p("a"), p("b"), p("out")], capture_output=True, timeout=300)
    assert out.returncode == 0 and read(p("out")) == whole, out.stderr.decode()[-2000:]
    out = subprocess.run(tool + ["-sub", "-inter", "0-3:3-11", p("pk"), p("in"), p("c"), p("d")], capture_output=True, timeout=300)
    assert out.returncode == 1 and b"Interval out of bounds! 3-11. Length of array is 10!" in out.stderr
    assert not os.path.exists(p("c")) and not os.path.exists(p("d"))
