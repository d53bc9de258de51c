"""GPU suite: ciphertext lists and plaintexts in the reference's json interface (include/vmnhip.h: vmn_garrays_from_jsonlines,
vmn_garrays_to_jsonlines, vmn_garrays_to_jsonplain, vmn_jsonlines_max_line_bytes; csrc/decimal_kernels.h: k_jsonlines_scan,
k_dec_to_rows, k_rows_to_dec, k_jsonlines_lengths / _offsets / _emit; verificatum_vmn_amd/interface.py; tools/vmnc_convert.py)
against tests/jsonlines_cases.py, the interface restated in Python, by exact equality: texts byte for byte, arrays through toBytes
and vmn_garray_equals, verdicts and the first bad line as parse() gives them.  The oracle of every value is int(str) / str(int).

Groups: the golden 512-, 1024-, 2048- and 3072-bit groups (D_max = 154, 309, 617, 925 digits: the top chunk of nine holds 1, 3, 5,
7 digits; the import runs one lane per element up to 2048 bits and two at 3072) at the Java wire width, and the 1024- and 2048-bit
ones at the modulus's own byte count as well, where 10^D_max exceeds 2^(8 nbytes): a number of D_max digits may not fit a leaf.
Python's limit of 4300 digits per conversion sits below a 16 384-bit value: larger moduli rest on the accumulator bounds stated
in csrc/decimal_kernels.h."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden

import hexlines_cases as hc
import jsonlines_cases as jc

pytestmark = pytest.mark.gpu

GROUPS = ["modp512", "modp1024", "modp1024-own", "modp2048", "modp2048-own", "modp3072"]
DMAX = {512: 154, 1024: 309, 2048: 617, 3072: 925}
WIDTHS = [1, 2, 3]
SIZES = [0, 1, 2, 63, 64, 65, 257, 1000]
ZEROS = [0, 1, 8, 9, 10]                     # leading zeros in front of a number: they shift the alignment of the chunks of nine
VMN_ERR_ARG, VMN_ERR_UNSUPPORTED = -1, -5


class Case:
    """One group: a pool of members as integers, and the calls of the C ABI as they are."""

    def __init__(self, vmn, ctx, name):
        from oracle import pyref
        self.vmn, self.ctx, self.name = vmn, ctx, name
        self.bits = int(name[4:].split("-")[0])
        g, _ = load_golden(self.bits)
        self.p, self.q = g["p"], g["q"]
        self.G = vmn.ModPGroup(ctx, g["p"], g["q"], g["g"], nbytes=self.bits // 8 if name.endswith("-own") else None)
        self.vb = self.G.nbytes
        self.dmax = jc.digits_of(self.p)
        self.pool = [pow(2 + v % (self.p - 3), 2, self.p) for v in pyref.stream_ints(b"jsonlines/" + name.encode(), 40, self.p)]
        self.pool[7] = 1                                               # short numbers among the long ones
        self.pool[11] = pow(3, 2 * 5, self.p)

    def rows(self, w, n, salt=0):
        L = len(self.pool)
        return [[self.pool[(5 * i + 11 * c + salt) % L] for c in range(2 * w)] for i in range(n)]

    def upload(self, rows, ncomp):
        """The component arrays of `rows` through from_be."""
        return [self.G.toElementArray(b"".join(r[c].to_bytes(self.vb, "big") for r in rows)) for c in range(ncomp)]

    def blocks(self, rows, ncomp):
        return [b"".join(r[c].to_bytes(self.vb, "big") for r in rows) for c in range(ncomp)]

    def parse(self, text, w, expected_n=0):
        """vmn_garrays_from_jsonlines as it is: (arrays | None, format_ok, first_bad_line, all_in_range, lines)."""
        vmn = self.vmn
        hs = (C.c_void_p * (2 * w))(*([0xdead] * (2 * w)))
        n, bad, fmt, rng = C.c_size_t(7), C.c_size_t(7), C.c_int(7), C.c_int(7)
        vmn._check(vmn.lib().vmn_garrays_from_jsonlines(self.G._h, C.c_size_t(w), text, C.c_size_t(len(text)), C.c_size_t(expected_n), hs,
                                                        C.byref(n), C.byref(fmt), C.byref(bad), C.byref(rng)))
        if not fmt.value:
            assert all(h is None for h in hs), "a defective text left an array behind"
            return None, False, bad.value, bool(rng.value), n.value
        return [vmn.PGroupElementArray(self.G, C.c_void_p(h)) for h in hs], True, bad.value, bool(rng.value), n.value

    def write(self, comps, w, plain=False, cap=None, fill=b"\xa5"):
        """vmn_garrays_to_jsonlines / _to_jsonplain as they are: (status, the whole buffer, written)."""
        lib = self.vmn.lib()
        n = comps[0].size()
        if cap is None:
            cap = max(1, n * lib.vmn_jsonlines_max_line_bytes(self.G._h, C.c_size_t(w)))
        hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
        out = C.create_string_buffer(fill * (cap + 8), cap + 8)
        written = C.c_size_t(12345)
        call = lib.vmn_garrays_to_jsonplain if plain else lib.vmn_garrays_to_jsonlines
        rc = call(hs, C.c_size_t(w), out, C.c_size_t(cap), C.byref(written))
        assert out.raw[cap:] == fill * 8, "the writer wrote behind cap"
        return rc, out.raw[:cap], written.value

    def leaf(self, v):
        """The leaf payload the byte-tree import is given for v: what does not fit a leaf is the all-0xff leaf."""
        return v.to_bytes(self.vb, "big") if v < 1 << (8 * self.vb) else b"\xff" * self.vb

    def from_bytetree(self, values):
        vmn = self.vmn
        bt = hc.eio.encode([self.leaf(v) for v in values])
        h, fmt, rng = C.c_void_p(), C.c_int(0), C.c_int(1)
        vmn._check(vmn.lib().vmn_garray_from_bytetree(self.G._h, bt, C.c_size_t(len(bt)), C.c_size_t(0), C.byref(h), C.byref(fmt), C.byref(rng)))
        assert fmt.value
        return vmn.PGroupElementArray(self.G, h), bool(rng.value)

    def live(self):
        return self.ctx.memory_stats()["live_bytes"]

    def close(self):
        self.G.close()


@pytest.fixture(scope="module")
def interface(vmn):
    from verificatum_vmn_amd import interface
    return interface


@pytest.fixture(scope="module", params=GROUPS)
def case(request, vmn, gpu_ctx):
    c = Case(vmn, gpu_ctx, request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def modp512(vmn, gpu_ctx):
    c = Case(vmn, gpu_ctx, "modp512")
    yield c
    c.close()


def free(arrays):
    for a in arrays or []:
        a.free()


# ---- 1. sizes ------------------------------------------------------------------------------------------------------------------
def test_sizes(case, interface):
    assert case.dmax == DMAX[case.bits] and case.dmax % 9 == {512: 1, 1024: 3, 2048: 5, 3072: 7}[case.bits]
    lib = case.vmn.lib()
    for w in (1, 2, 3, 65536):
        assert lib.vmn_jsonlines_max_line_bytes(case.G._h, C.c_size_t(w)) == jc.max_line_bytes(case.dmax, w) == interface.json_max_line_bytes(case.G, w)
    assert lib.vmn_jsonlines_max_line_bytes(case.G._h, C.c_size_t(0)) == 0 == lib.vmn_jsonlines_max_line_bytes(case.G._h, C.c_size_t(65537))
    assert lib.vmn_jsonlines_max_line_bytes(None, C.c_size_t(1)) == 0
    if case.name.endswith("-own"):
        assert 10 ** case.dmax > 1 << (8 * case.vb)                   # a number of D_max digits may not fit the leaf


# ---- 2. round trip through the text ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", WIDTHS)
def test_round_trip_through_the_text(case, interface, w):
    for n in SIZES:
        rows = case.rows(w, n, salt=n)
        want_text = jc.text_of(w, rows)
        back, fmt, _, rng, lines = case.parse(want_text, w)
        assert fmt and rng and lines == n and len(back) == 2 * w
        assert [a.toBytes() for a in back] == case.blocks(rows, 2 * w), n
        if n == 0:
            assert all(a.size() == 0 for a in back)
            rc, _, written = case.write(back, w)
            assert (rc, written) == (0, 0)
            free(back)
            continue
        comps = case.upload(rows, 2 * w)
        assert all(a.equals(b) for a, b in zip(back, comps))
        rc, buf, written = case.write(comps, w)
        assert rc == 0 and written == len(want_text), n
        assert buf[:written] == want_text, (n, "to_jsonlines differs from the restatement")
        assert interface.format_json(back) == want_text
        free(back + comps)


# ---- 3. decimal -> binary at its edges ------------------------------------------------------------------------------------------
def edge_values(case):
    p, vb, dmax = case.p, case.vb, case.dmax
    nw = (case.bits + 31) // 32
    vals = [1, 0, 2]
    for k in (8, 9, 10, 17, 18, 19):
        vals += [10 ** k - 1, 10 ** k]
    for j in (1, nw // 2, nw - 1, nw):                                # the first, a middle and the last word; 2^(32 nw) is past p
        vals += [(1 << (32 * j)) - 1, 1 << (32 * j), (1 << (32 * j)) + 1]
    vals += [10 ** (9 * (dmax // 9)) - 1, 10 ** dmax - 1]             # every chunk 999 999 999: the largest below p, the largest of D_max digits
    vals += [p - 1, p, p + 1, (1 << (8 * vb)) - 1, 1 << (8 * vb), 10 ** dmax, 10 ** dmax + 7, 3 * 10 ** (dmax + 20)]
    return vals


def test_edge_values_as_the_byte_tree_import_takes_them(case):
    """The arrays, all_in_range and the replaced entries are what vmn_garray_from_bytetree gives for the same values (a value
    that does not fit a leaf: for the all-0xff leaf) -- all of them in one text per count of leading zeros, in either slot, and
    each of them alone."""
    vals = edge_values(case)
    p, good = case.p, case.pool[0]
    assert any(v >= p for v in vals) and any(v >= 1 << (8 * case.vb) for v in vals) and any(len(str(v)) > case.dmax for v in vals)
    ref, ref_rng = case.from_bytetree(vals)
    goods, goods_rng = case.from_bytetree([good] * len(vals))
    assert not ref_rng and goods_rng
    for zeros in ZEROS:
        z = b"0" * zeros
        for slot in (0, 1):
            lines = []
            for v in vals:
                pair = (z + b"%d" % v, b"%d" % good) if slot == 0 else (b"%d" % good, z + b"%d" % v)
                lines.append(b'{"alpha":"%s","beta":"%s"}\n' % pair)
            back, fmt, _, rng, count = case.parse(b"".join(lines), 1)
            assert fmt and count == len(vals) and rng == ref_rng, (zeros, slot)
            assert back[slot].equals(ref) and back[slot].toBytes() == ref.toBytes(), (zeros, slot)
            assert back[1 - slot].equals(goods), (zeros, slot)
            free(back)
    for v in vals:                                                    # alone: the verdict of each
        one, one_rng = case.from_bytetree([v])
        back, fmt, _, rng, _ = case.parse(b'{"beta":"00%d","alpha":"%d"}' % (good, v), 1)
        assert fmt and rng == one_rng == (v < p), v
        assert back[0].equals(one) and back[0].toBytes() == one.toBytes(), v
        free(back + [one])
    # at width 3, in the fifth of the six slots
    rows = [[good] * 4 + [v] + [good] for v in vals]
    text = b"".join(b"[" + b",".join(b'{"alpha":"%d","beta":"%d"}' % (r[i], r[3 + i]) for i in range(3)) + b"]\n" for r in rows)
    back, fmt, _, rng, _ = case.parse(text, 3)
    assert fmt and not rng and back[4].equals(ref) and all(back[c].equals(goods) for c in (0, 1, 2, 3, 5))
    free(back + [ref, goods])


# ---- 4. binary -> decimal at its edges ------------------------------------------------------------------------------------------
def writer_values(case):
    p, dmax = case.p, case.dmax
    nw = (case.bits + 31) // 32
    vals = [1, 2, 9, 10, p - 1, p - 2]
    vals += [k * 10 ** 9 for k in (1, 7, 999999999)] + [10 ** 18 + 1, 10 ** 27 + 10 ** 9, 5 * 10 ** (dmax - 2)]      # zero chunks inside
    for d in range(1, dmax):                                          # around every digit count: floor(bits log10(2)) + 1 is off by one here
        vals += [10 ** d - 1, 10 ** d]
    vals += [(1 << (32 * j)) - 1 for j in (1, 2, nw // 2, nw - 1)] + [(1 << (case.bits - 1)) - 1]                  # words of all ones
    vals += [1 << m for m in range(1, case.bits - 1, 53)]
    vals += case.pool
    assert all(0 < v < p for v in vals)
    return vals + [1] * (len(vals) % 2)


def test_written_text_is_the_python_writers(case):
    vals = writer_values(case)
    half = len(vals) // 2
    rows = [[a, b] for a, b in zip(vals[:half], vals[half:])]
    comps = case.upload(rows, 2)
    want = jc.text_of(1, rows)
    rc, buf, written = case.write(comps, 1)
    assert rc == 0 and written == len(want)
    assert buf[:written] == want
    plain_rows = [[v] for v in vals]
    arr = case.upload(plain_rows, 1)
    want = jc.plain_text_of(1, plain_rows)
    rc, buf, written = case.write(arr, 1, plain=True)
    assert rc == 0 and written == len(want) and buf[:written] == want
    free(comps + arr)


# ---- 5. plaintext lines, round trips through files ------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 3])
def test_plaintext_lines(case, interface, tmp_path, w):
    for n in (1, 65, 257):
        rows = [r[:w] for r in case.rows(w, n, salt=2)]
        comps = case.upload(rows, w)
        want = jc.plain_text_of(w, rows)
        rc, buf, written = case.write(comps, w, plain=True)
        assert rc == 0 and written == len(want) and buf[:written] == want, n
        assert interface.format_json_plaintexts(comps) == want
        path = str(tmp_path / "plain")
        interface.write_plaintexts(path, comps, "json")
        assert open(path, "rb").read() == want
        interface.write_plaintexts(path, comps, "raw")
        leaves = [[r[c].to_bytes(case.vb, "big") for r in rows] for c in range(w)]
        assert open(path, "rb").read() == hc.eio.encode(leaves[0] if w == 1 else leaves)
        with pytest.raises(ValueError):
            interface.write_plaintexts(path, comps, "native")
        free(comps)


def test_round_trips_between_the_interfaces(case, interface, tmp_path):
    for w, n in ((1, 65), (3, 64)):
        rows = case.rows(w, n, salt=3)
        text = jc.text_of(w, rows)
        j1, raw, j2, nat, j3, nat2 = (str(tmp_path / name) for name in ("a.json", "a.raw", "b.json", "a.native", "c.json", "b.native"))
        open(j1, "wb").write(text)
        assert interface.convert_list(case.G, j1, raw, w, "json", "raw")
        assert interface.convert_list(case.G, raw, j2, w, "raw", "json")
        assert open(j2, "rb").read() == text                          # json -> raw -> json
        assert interface.convert_list(case.G, raw, nat, w, "raw", "native")
        assert interface.convert_list(case.G, nat, j3, w, "native", "json")
        assert interface.convert_list(case.G, j3, nat2, w, "json", "native")
        assert open(nat2, "rb").read() == open(nat, "rb").read() and open(j3, "rb").read() == text      # native -> json -> native
        a = interface.read_list(case.G, j1, w, "json", expected_n=n)
        b = interface.read_list(case.G, raw, w, "raw")
        assert a is not None and b is not None and all(x.equals(y) for x, y in zip(a, b))
        assert interface.read_list(case.G, j1, w, "json", expected_n=n + 1) is None
        for call in (lambda: interface.read_list(case.G, j1, w, "xml"), lambda: interface.write_list(j1 + "x", a, "xml"),
                     lambda: interface.convert_list(case.G, j1, j1 + "x", w, "json", "xml"),
                     lambda: interface.read_ciphertexts(case.G, j1, w, "json"), lambda: interface.write_ciphertexts(j1 + "x", a, "json")):
            with pytest.raises(ValueError):                           # (the last two: the two-interface calls stay what they were)
                call()
        assert not os.path.exists(j1 + "x")
        free(a + b)
    assert interface.read_list(case.G, str(tmp_path / "missing"), 1, "json") is None


# ---- 6. the catalogue ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,n", [(1, 5), (2, 4), (3, 5)])
def test_every_catalogue_text_gets_the_python_readers_verdict(case, w, n):
    rows = case.rows(w, n)
    want = case.blocks(rows, 2 * w)
    for label, text in jc.valid_variants(w, rows).items():
        assert jc.parse(text, w) == (True, 0, rows), label
        back, fmt, bad, rng, lines = case.parse(text, w, n)
        assert fmt and bad == 0 and rng == jc.in_range(rows, case.p) and lines == n, label
        assert [a.toBytes() for a in back] == want, label
        free(back)
    live0 = case.live()
    for label, text, k in jc.defects(w, rows):
        ok, bad, _ = jc.parse(text, w)
        assert not ok and bad == k, label
        back, fmt, got, _, lines = case.parse(text, w)
        assert back is None and not fmt and lines == 0, label
        assert got == bad, (label, got, bad)
        assert case.live() == live0, label


@pytest.mark.parametrize("n", [1, 2, 65, 257])
def test_defects_at_other_sizes(modp512, n):
    case = modp512
    rows = case.rows(1, n)
    where = None if n <= 2 else [0, 63, 64, n - 1]
    for label, text, k in jc.defects(1, rows, where):
        back, fmt, got, _, _ = case.parse(text, 1)
        assert back is None and not fmt and got == k == jc.parse(text, 1)[1], label


def test_values_out_of_range_in_catalogue_form(modp512):
    """A text that is well formed and holds p: the arrays exist, all_in_range is false, as parse() + in_range() say."""
    case = modp512
    rows = case.rows(2, 4)
    rows[2][3] = case.p
    for label, text in jc.valid_variants(2, rows).items():
        back, fmt, _, rng, lines = case.parse(text, 2)
        assert fmt and lines == 4 and rng is False and not jc.in_range(rows, case.p), label
        assert back[3].toInts()[2] == 1                               # replaced, as the byte-tree import replaces it
        free(back)


# ---- 7. the writer's buffer, the line count, the empty text, misuse --------------------------------------------------------------
def test_a_buffer_one_byte_short_is_an_argument_error(case):
    for w, plain in ((1, False), (3, False), (1, True), (3, True)):
        ncomp = w if plain else 2 * w
        rows = [r[:ncomp] for r in case.rows(w, 9)]
        comps = case.upload(rows, ncomp)
        want = jc.plain_text_of(w, rows) if plain else jc.text_of(w, rows)
        rc, buf, written = case.write(comps, w, plain, cap=len(want))            # exactly enough
        assert rc == 0 and written == len(want) and buf == want
        rc, buf, written = case.write(comps, w, plain, cap=len(want) - 1)
        assert rc == VMN_ERR_ARG and written == 0 and buf == b"\xa5" * (len(want) - 1)
        free(comps)


@pytest.mark.parametrize("w", [1, 3])
def test_expected_size_and_the_empty_text(case, w):
    n = 5
    text = jc.text_of(w, case.rows(w, n))
    for expected in (1, n - 1, n + 1, 1000):
        assert jc.parse(text, w, expected)[:2] == (False, min(n, expected))
        assert case.parse(text, w, expected)[:3] == (None, False, min(n, expected))
    broken = b"{}\n" + text                                           # a count mismatch is reported as such, whatever the lines hold
    assert case.parse(broken, w, n)[:3] == (None, False, n) and case.parse(broken, w)[:3] == (None, False, 0)
    back, fmt, _, rng, lines = case.parse(b"", w)
    assert (fmt, rng, lines) == (True, True, 0) and len(back) == 2 * w and all(a.size() == 0 for a in back)
    free(back)
    assert case.parse(b"", w, 3)[:3] == (None, False, 0)
    assert case.parse(b"\n", w)[:3] == (None, False, 0)               # one blank line is a line


def test_misuse_is_an_argument_error(modp512):
    case, lib = modp512, modp512.vmn.lib()
    text = jc.text_of(1, case.rows(1, 2))
    hs = (C.c_void_p * 2)()
    n, bad, fmt, rng = C.c_size_t(0), C.c_size_t(0), C.c_int(0), C.c_int(0)
    args = (C.c_size_t(len(text)), C.c_size_t(0), hs, C.byref(n), C.byref(fmt), C.byref(bad), C.byref(rng))
    assert lib.vmn_garrays_from_jsonlines(case.G._h, C.c_size_t(0), text, *args) == VMN_ERR_ARG
    assert lib.vmn_garrays_from_jsonlines(None, C.c_size_t(1), text, *args) == VMN_ERR_ARG
    assert lib.vmn_garrays_from_jsonlines(case.G._h, C.c_size_t(1), None, *args) == VMN_ERR_ARG
    a, b = case.upload(case.rows(1, 3), 2)
    short = case.upload(case.rows(1, 2), 1)[0]
    out = C.create_string_buffer(1 << 16)
    written = C.c_size_t(0)
    for pair in ((a, short), (a, None)):
        hs = (C.c_void_p * 2)(*[x._h if x is not None else None for x in pair])
        assert lib.vmn_garrays_to_jsonlines(hs, C.c_size_t(1), out, C.c_size_t(1 << 16), C.byref(written)) == VMN_ERR_ARG
        assert lib.vmn_garrays_to_jsonplain(hs, C.c_size_t(2), out, C.c_size_t(1 << 16), C.byref(written)) == VMN_ERR_ARG
    hs = (C.c_void_p * 2)(a._h, b._h)
    assert lib.vmn_garrays_to_jsonlines(hs, C.c_size_t(1), None, C.c_size_t(1 << 16), C.byref(written)) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_jsonlines(hs, C.c_size_t(0), out, C.c_size_t(1 << 16), C.byref(written)) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_jsonlines(hs, C.c_size_t(1), out, C.c_size_t(1 << 16), None) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_jsonlines(None, C.c_size_t(1), out, C.c_size_t(1 << 16), C.byref(written)) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_jsonlines(hs, C.c_size_t(1), out, C.c_size_t(1 << 16), C.byref(written)) == 0
    assert out.raw[:written.value] == jc.text_of(1, case.rows(1, 3))
    free([a, b, short])


# ---- 8. curves, non-members, the tool ------------------------------------------------------------------------------------------
def test_a_curve_group_is_unsupported(vmn, gpu_ctx, interface):
    G = vmn.ECqPGroup(gpu_ctx, "P-256")
    lib = vmn.lib()
    assert lib.vmn_jsonlines_max_line_bytes(G._h, C.c_size_t(1)) == 0
    text = b'{"alpha":"1","beta":"2"}\n'
    hs = (C.c_void_p * 2)(0xdead, 0xdead)
    n, bad, fmt, rng = C.c_size_t(0), C.c_size_t(0), C.c_int(1), C.c_int(0)
    rc = lib.vmn_garrays_from_jsonlines(G._h, C.c_size_t(1), text, C.c_size_t(len(text)), C.c_size_t(0), hs, C.byref(n), C.byref(fmt), C.byref(bad),
                                        C.byref(rng))
    assert rc == VMN_ERR_UNSUPPORTED and not fmt.value and all(h is None for h in hs)
    assert b"modular groups only" in lib.vmn_last_error()
    pts = [G.toElementArray([G.g] * 3) for _ in range(2)]
    out = C.create_string_buffer(4096)
    written = C.c_size_t(5)
    hs = (C.c_void_p * 2)(*[a._h for a in pts])
    assert lib.vmn_garrays_to_jsonlines(hs, C.c_size_t(1), out, C.c_size_t(4096), C.byref(written)) == VMN_ERR_UNSUPPORTED
    assert lib.vmn_garrays_to_jsonplain(hs, C.c_size_t(2), out, C.c_size_t(4096), C.byref(written)) == VMN_ERR_UNSUPPORTED
    assert written.value == 0 and out.raw == bytes(4096)
    with pytest.raises(vmn.VmnError):
        interface.parse_json(G, text, 1)
    free(pts)
    G.close()


def test_a_non_residue_in_one_line_is_no_list(modp512, interface, tmp_path):
    case = modp512
    p = case.p
    rows = case.rows(1, 9)
    rows[4][1] = p - rows[4][1]                                       # -x of a square: in range, no member (p = 3 mod 4)
    assert pow(rows[4][1], case.q, p) != 1
    text = jc.text_of(1, rows)
    path = str(tmp_path / "nonresidue.json")
    open(path, "wb").write(text)
    report = {}
    assert interface.read_list(case.G, path, 1, "json", report=report) is None
    assert report == dict(format_ok=True, first_bad_line=0, all_in_range=True, lines=9)
    back, fmt, _, rng, _ = case.parse(text, 1)                        # the arrays themselves are in range: membership is a call of its own
    assert fmt and rng and not back[1].isMember() and back[0].isMember()
    free(back)
    rows[4][1] = p                                                    # out of range: no list either, and the report says which
    assert interface.parse_json(case.G, jc.text_of(1, rows), 1, report=report) is None
    assert report["format_ok"] and not report["all_in_range"]
    bad = jc.text_of(1, rows[:3]) + b'{"alpha":"1"}\n'
    assert interface.parse_json(case.G, bad, 1, report=report) is None and report["first_bad_line"] == 3 and not report["format_ok"]


def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmnc_convert.py")] + list(args), capture_output=True, text=True,
                          timeout=120)


def test_the_tool_converts_and_names_the_line(tmp_path):
    from oracle import pyref
    p, q, g = pyref.modp_group(2048)
    w, n = 2, 7
    rows = [[pow(g, 3 + 5 * i + c, p) for c in range(2 * w)] for i in range(n)]
    src, raw, again, plain = (str(tmp_path / name) for name in ("in.json", "mid.raw", "out.json", "plain.json"))
    text = b"".join(jc.dumps_line(w, r) + b"\r\n" for r in rows)
    open(src, "wb").write(text)
    common = ["-width", str(w), "--bits", "2048"]
    r = run_tool("-ciphs", "-ini", "json", "-outi", "raw", *common, src, raw)
    assert r.returncode == 0, r.stderr[-2000:]
    r = run_tool("-ciphs", "-ini", "raw", "-outi", "json", *common, raw, again)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(again, "rb").read() == jc.text_of(w, rows)             # the same list, in the writer's own form
    cols = [[r[c].to_bytes(257, "big") for r in rows] for c in range(w)]          # the u half of the list as w plaintext columns
    open(raw, "wb").write(hc.eio.encode(cols))
    r = run_tool("-plain", "-outi", "json", *common, raw, plain)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(plain, "rb").read() == jc.plain_text_of(w, [r[:w] for r in rows])
    k = 4
    lines = text.split(b"\r\n")
    lines[k] = lines[k].replace(b'"beta"', b'"gamma"', 1)
    open(src, "wb").write(b"\r\n".join(lines))
    os.remove(raw)
    r = run_tool("-ciphs", "-ini", "json", "-outi", "raw", *common, src, raw)
    assert r.returncode == 1 and ("line %d " % (k + 1)) in r.stderr and not os.path.exists(raw), (r.returncode, r.stderr[-2000:])
