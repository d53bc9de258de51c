"""GPU suite: ciphertext lists under a public key of width kappa in the `raw` and `native` interfaces
(verificatum_vmn_amd/interface.py with keywidth; include/vmnhip.h: vmn_garrays_from_hexlines_keyed, vmn_garrays_to_hexlines_keyed;
csrc/hexlines_layout.h) against the restatement of the nesting rule on Python integers and bytes (tests/keyed_layout_ref.py), by
exact equality of files and of arrays.  The 512-bit golden group and P-256 at the reference's 33-byte coordinates, N = 30 lines,
kappa = 2, omega in {1, 3}.

Wall time on an MI355X (one run, pytest's call durations): every case at most 0.03 s but the converter's (three processes, 0.8 s); the module under 2 s with its set-up."""
import ctypes as C

import pytest

from conftest import load_golden

import hexlines_cases as hc
import keyed_layout_ref as KL
from named_curves import ref_curve

pytestmark = pytest.mark.gpu

N, KW = 30, 2
SHAPES = [(KW, 1), (KW, 3)]


class Case:
    """One group, a pool of its elements as Python values, and lists of them as 2 kappa omega columns."""

    def __init__(self, vmn, ctx, name):
        from oracle import pyref
        self.curve = name != "modp512"
        if self.curve:
            self.G = vmn.ECqPGroup(ctx, name, java_widths=True)
            c, acc, self.pool = ref_curve(name), None, []
            for _ in range(41):
                acc = c.add(acc, c.g)
                self.pool.append(acc)
        else:
            g, _ = load_golden(512)
            p = g["p"]
            self.G = vmn.ModPGroup(ctx, p, g["q"], g["g"])
            self.pool = [pow(2 + v % (p - 3), 2, p) for v in pyref.stream_ints(b"keyed-lists", 41, p)]
        self.vb = self.G.nbytes

    def columns(self, count, salt=0):
        L = len(self.pool)
        return [[self.pool[(5 * i + 11 * c + salt) % L] for i in range(N)] for c in range(count)]

    def upload(self, cols):
        return [self.G.toElementArray(col) for col in cols]


@pytest.fixture(scope="module", params=["modp512", "P-256"])
def case(request, vmn, gpu_ctx):
    c = Case(vmn, gpu_ctx, request.param)
    yield c
    c.G.close()


@pytest.fixture(scope="module")
def interface(vmn):
    from verificatum_vmn_amd import interface
    return interface


def ints_of(arrays):
    return [a.toInts() for a in arrays]


def free(arrays):
    for a in arrays or []:
        a.free()


def read(path):
    with open(path, "rb") as f:
        return f.read()


@pytest.mark.parametrize("kw,w", SHAPES)
def test_a_keyed_list_written_raw_and_native_is_the_restated_file_and_reads_back(case, interface, tmp_path, kw, w):
    G, cols = case.G, case.columns(2 * kw * w)
    comps = case.upload(cols)
    assert interface.ciphertext_line_bytes(G, w, kw) == KL.line_bytes(case.curve, case.vb, kw, w)
    want = {"raw": KL.list_tree(case.curve, case.vb, kw, cols), "native": KL.native_text(case.curve, case.vb, kw, cols)}
    for fmt in ("raw", "native"):
        path = str(tmp_path / ("list." + fmt))
        interface.write_list(path, comps, fmt, keywidth=kw)
        assert read(path) == want[fmt], fmt
        report = {}
        back = interface.read_list(G, path, w, fmt, expected_n=N, report=report, keywidth=kw)
        assert back is not None and len(back) == 2 * kw * w and ints_of(back) == cols, fmt
        if fmt == "native":
            assert report == {"format_ok": True, "first_bad_line": 0, "all_in_range": True, "lines": N}
        free(back)
    # from one interface to the other and back: the same two files
    assert interface.convert_list(G, str(tmp_path / "list.native"), str(tmp_path / "conv.raw"), w, "native", "raw", keywidth=kw)
    assert interface.convert_list(G, str(tmp_path / "conv.raw"), str(tmp_path / "conv.native"), w, "raw", "native", keywidth=kw)
    assert read(str(tmp_path / "conv.raw")) == want["raw"] and read(str(tmp_path / "conv.native")) == want["native"]
    # read at the wrong shape: the keyed (kw, w) file is no unkeyed list of width kw * w unless w = 1, and no (w, kw) list
    if w > 1:
        for fmt in ("raw", "native"):
            assert interface.read_list(G, str(tmp_path / ("list." + fmt)), kw * w, fmt) is None
            assert interface.read_list(G, str(tmp_path / ("list." + fmt)), kw, fmt, keywidth=w) is None
    free(comps)


def test_width_one_under_a_key_is_byte_for_byte_the_unkeyed_list_of_that_width(case, interface, tmp_path):
    G, cols = case.G, case.columns(2 * KW)
    comps = case.upload(cols)
    for fmt in ("raw", "native"):
        keyed, plain = str(tmp_path / ("keyed." + fmt)), str(tmp_path / ("plain." + fmt))
        interface.write_list(keyed, comps, fmt, keywidth=KW)
        interface.write_list(plain, comps, fmt)
        assert read(keyed) == read(plain), fmt
        back = interface.read_list(G, plain, 1, fmt, keywidth=KW)
        assert ints_of(back) == cols
        free(back)
    free(comps)


def test_two_by_three_differs_from_the_unkeyed_width_six_text_in_the_predicted_framing_only(case, interface):
    kw, w = 2, 3
    G, cols = case.G, case.columns(2 * kw * w, salt=3)
    comps = case.upload(cols)
    keyed, plain = interface.format_native(comps, keywidth=kw), interface.format_native(comps)
    B, B6, E = KL.line_bytes(case.curve, case.vb, kw, w), hc.line_bytes(case.curve, case.vb, kw * w), KL.element_bytes(case.curve, case.vb)
    assert B == B6 + 2 * w * 5                                   # one node header per plaintext component and half
    off, off6 = KL.component_offsets(case.curve, case.vb, kw, w), hc.component_offsets(case.curve, case.vb, kw * w)
    klines, plines = keyed.split(b"\n")[:-1], plain.split(b"\n")[:-1]
    assert len(klines) == len(plines) == N
    node3, node2, node6 = KL.hdr(0, 3).hex().encode(), KL.hdr(0, 2).hex().encode(), KL.hdr(0, 6).hex().encode()
    for kl, pl in zip(klines, plines):
        assert len(kl) == 2 * B and len(pl) == 2 * B6
        # the element trees are the same digits, in the same order
        assert [kl[2 * o:2 * (o + E)] for o in off] == [pl[2 * o:2 * (o + E)] for o in off6]
        # what is left of the keyed line: node(u, v), per half node(3) and three times node(2); of the unkeyed: node(u, v), node(6)
        rest = b"".join(kl[2 * (a + E):2 * b] for a, b in zip([-E] + off, off + [B]))
        assert rest == node2 + (node3 + node2 + node2 + node2) * 2
        rest6 = b"".join(pl[2 * (a + E):2 * b] for a, b in zip([-E] + off6, off6 + [B6]))
        assert rest6 == node2 + node6 * 2
    free(comps)


def patch(line, at, value):
    return line[:2 * at] + b"%02x" % value + line[2 * at + 2:]


def framing_defects(case, kw, w, line, unkeyed_line):
    """[(label, replacement)] for one good line of a (kw, w) list, w > 1: the defects of tests/hexlines_cases.py that involve the
    framing, at the new node level."""
    off = KL.component_offsets(case.curve, case.vb, kw, w)
    return [("omega-count", patch(line, 9, w + 1)),                       # node(w; ...) of the u half says w + 1
            ("first-kappa-count", patch(line, off[0] - 1, kw + 1)),      # the first node(kappa; ...) says kappa + 1
            ("last-kappa-count", patch(line, off[-kw] - 1, kw - 1)),     # the last one, in the v half, says kappa - 1
            ("kappa-node-is-a-leaf", patch(line, off[kw] - 5, 1)),       # the tag of the second node(kappa; ...)
            ("missing-inner-node", unkeyed_line),                        # the kappa w elements directly under node(kappa w)
            ("short-line", line[:-2]),
            ("one-digit-short", line[:-1])]


@pytest.mark.parametrize("k", [0, N // 2, N - 1])
def test_framing_defects_at_the_new_level_are_reported_with_their_line(case, interface, tmp_path, k):
    kw, w = 2, 3
    G, cols = case.G, case.columns(2 * kw * w, salt=7)
    comps = case.upload(cols)
    lines = interface.format_native(comps, keywidth=kw).split(b"\n")[:-1]
    unkeyed = interface.format_native(comps).split(b"\n")[:-1]
    free(comps)
    for label, bad in framing_defects(case, kw, w, lines[k], unkeyed[k]):
        text = b"".join(l + b"\n" for l in lines[:k] + [bad] + lines[k + 1:])
        report = {}
        assert interface.parse_native(G, text, w, report=report, keywidth=kw) is None, label
        assert (report["format_ok"], report["first_bad_line"], report["lines"]) == (False, k, 0), (label, report)
    # two defects: the smaller index is named
    if k:
        a = framing_defects(case, kw, w, lines[0], unkeyed[0])[1][1]
        b = framing_defects(case, kw, w, lines[k], unkeyed[k])[5][1]
        report = {}
        assert interface.parse_native(G, b"".join(l + b"\n" for l in [a] + lines[1:k] + [b] + lines[k + 1:]), w, report=report, keywidth=kw) is None
        assert report["first_bad_line"] == 0
    # a line count that differs from the expected one
    report = {}
    assert interface.parse_native(G, b"".join(l + b"\n" for l in lines), w, expected_n=N + 1, report=report, keywidth=kw) is None
    assert (report["format_ok"], report["first_bad_line"]) == (False, N)


def test_json_cannot_hold_a_keyed_list(case, interface, tmp_path):
    G, cols = case.G, case.columns(2 * KW)
    comps = case.upload(cols)
    src = str(tmp_path / "list.raw")
    interface.write_list(src, comps, "raw", keywidth=KW)
    with pytest.raises(ValueError):
        interface.write_list(str(tmp_path / "list.json"), comps, "json", keywidth=KW)
    with pytest.raises(ValueError):
        interface.read_list(G, src, 1, "json", keywidth=KW)
    with pytest.raises(ValueError):
        interface.convert_list(G, src, str(tmp_path / "out.json"), 1, "raw", "json", keywidth=KW)
    with pytest.raises(ValueError):
        interface.write_plaintexts(str(tmp_path / "plain.json"), comps[:KW], "json", keywidth=KW)
    assert not (tmp_path / "list.json").exists() and not (tmp_path / "out.json").exists() and not (tmp_path / "plain.json").exists()
    free(comps)


@pytest.mark.parametrize("kw,w", SHAPES)
def test_raw_plaintexts_under_a_key(case, interface, tmp_path, kw, w):
    G, cols = case.G, case.columns(kw * w, salt=5)
    comps = case.upload(cols)
    path = str(tmp_path / "plain.raw")
    interface.write_plaintexts(path, comps, "raw", keywidth=kw)
    assert read(path) == KL.wide_array_tree(case.curve, case.vb, kw, cols)
    if not case.curve:                                            # (read_plaintexts sizes its arrays as a modular group's)
        back = interface.read_plaintexts(G, path, w, keywidth=kw)
        assert back is not None and ints_of(back) == cols
        free(back)
        if w > 1:
            assert interface.read_plaintexts(G, path, kw * w) is None
    free(comps)


def counted(ctx, fn):
    ctx.timing_enable(True)
    try:
        ctx.timing_reset()
        out = fn()
        return out, {name: row[0] for name, row in ctx.timing_report().items() if row[0]}
    finally:
        ctx.timing_enable(False)
        ctx.timing_reset()


def test_the_nesting_costs_no_launch(case, interface, gpu_ctx):
    """A keyed (2, 3) list against an unkeyed list of width 6 of the same N: the same launches in the hexlines family and in
    every other family, reading and writing."""
    kw, w = 2, 3
    G, cols = case.G, case.columns(2 * kw * w, salt=9)
    comps = case.upload(cols)
    keyed_text, c_kw = counted(gpu_ctx, lambda: interface.format_native(comps, keywidth=kw))
    plain_text, c_pw = counted(gpu_ctx, lambda: interface.format_native(comps))
    assert c_kw == c_pw and c_kw["hexlines"] >= 1, (c_kw, c_pw)
    keyed, c_kr = counted(gpu_ctx, lambda: interface.parse_native(G, keyed_text, w, keywidth=kw))
    plain, c_pr = counted(gpu_ctx, lambda: interface.parse_native(G, plain_text, kw * w))
    assert c_kr == c_pr and c_kr["hexlines"] >= 1, (c_kr, c_pr)
    assert gpu_ctx.timing_get("hexlines")[0] == 0                 # (counted() leaves the counters reset)
    assert ints_of(keyed) == ints_of(plain) == cols
    free(comps + keyed + plain)


def test_the_bounds_on_the_widths_apply_to_their_product(case, vmn):
    G = case.G
    line_bytes = lambda kw, w: vmn.lib().vmn_hexlines_line_bytes_keyed(G._h, C.c_size_t(kw), C.c_size_t(w))
    assert line_bytes(0, 1) == 0 and line_bytes(1, 0) == 0
    assert line_bytes(256, 256) == KL.line_bytes(case.curve, case.vb, 256, 256) and line_bytes(256, 257) == 0 and line_bytes(65537, 1) == 0
    assert line_bytes(1, 65536) == vmn.lib().vmn_hexlines_line_bytes(G._h, C.c_size_t(65536))
    assert line_bytes(65536, 1 << 48) == 0 and line_bytes(1 << 48, 65536) == 0      # (a product that wraps to 0 in 64 bits)
    hs = (C.c_void_p * 2)()
    n, bad, fmt, rng = C.c_size_t(), C.c_size_t(), C.c_int(), C.c_int()
    rc = vmn.lib().vmn_garrays_from_hexlines_keyed(G._h, C.c_size_t(0), C.c_size_t(1), b"", C.c_size_t(0), C.c_size_t(0), hs, C.byref(n),
                                                   C.byref(fmt), C.byref(bad), C.byref(rng))
    assert rc == -1                                               # VMN_ERR_ARG


def test_the_converter_takes_a_key_width(vmn, gpu_ctx, interface, tmp_path):
    """tools/vmnc_convert.py -keywidth 2 over P-256 (the tool names a modular group by its RFC 3526 size, which the 512-bit golden
    group is not): native -> raw gives the restated tree; with json it is a usage error."""
    import os
    import subprocess
    import sys
    from conftest import ROOT
    case = Case(vmn, gpu_ctx, "P-256")
    kw, w = 2, 3
    cols = case.columns(2 * kw * w, salt=13)
    comps = case.upload(cols)
    src, dst = str(tmp_path / "in.native"), str(tmp_path / "out.raw")
    interface.write_list(src, comps, "native", keywidth=kw)
    free(comps)
    case.G.close()
    tool = [sys.executable, os.path.join(ROOT, "tools", "vmnc_convert.py"), "-ciphs", "-width", str(w), "-keywidth", str(kw), "--curve", "P-256"]
    out = subprocess.run(tool + ["-ini", "native", "-outi", "raw", src, dst], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    assert read(dst) == KL.list_tree(case.curve, case.vb, kw, cols)
    # without the key width the same file is no list of width 3, and the line is named
    out = subprocess.run(tool[:5] + ["--curve", "P-256", "-ini", "native", "-outi", "raw", src, str(tmp_path / "no.raw")], capture_output=True, timeout=300)
    assert out.returncode == 1 and b"line 1 is not a ciphertext of width 3" in out.stderr and not (tmp_path / "no.raw").exists()
    usage = subprocess.run([sys.executable, tool[1], "-ciphs", "-keywidth", "2", "--bits", "2048", "-ini", "native", "-outi", "json", src, dst],
                           capture_output=True, timeout=60)
    assert usage.returncode == 2 and b"json" in usage.stderr
