"""GPU suite: plaintexts as text over curve groups -- messages encoded as points and decoded again (include/vmnhip.h:
vmn_ec_group_encode_length, vmn_ec_arrays_from_textlines, vmn_ec_arrays_to_textlines; csrc/ec_encode_kernels.h: k_ec_encode_search,
k_ec_encode_root, k_ec_textlines_fold; verificatum_vmn_amd/interface.py; tools/vmn_point_texts.py) against
tests/point_encode_cases.py, the rule restated on Python integers, by exact equality: arrays through toBytes, texts byte for byte.

Curves: P-192, P-224 (Tonelli-Shanks, s = 96), secp224k1 (s = 2), prime239v1 (a top byte that is not full), P-256, P-256 at the
reference's 33-byte coordinates, brainpoolp256r1 (general a), secp256k1 (a = 0), P-384, brainpoolp512r1, P-521.
n in {0, 1, 2, 63, 64, 65, 257, 1000}, 1, 2 and 3 components; every sample from 63 lines on holds points accepted at the counters
0, 1, 2, 3 and at one of 6 or more, the unlucky one between two lucky ones (tests/test_point_encode_catalogue.py asserts that)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden

import encode_cases as ec
import point_encode_cases as pe

pytestmark = pytest.mark.gpu

VMN_ERR_ARG, VMN_ERR_UNSUPPORTED = -1, -5


class Case:
    """One curve group and the calls of the C ABI as they are."""

    def __init__(self, vmn, ctx, name):
        self.vmn, self.ctx, self.name = vmn, ctx, name
        self.G = vmn.ECqPGroup(ctx, name.replace("-java", ""), java_widths=name.endswith("-java"))
        self.vb = self.G.nbytes
        self.p = self.G.p
        self.L = pe.encode_length(self.p)

    def encode(self, text, ncomp, group=None):
        """vmn_ec_arrays_from_textlines as it is: (status, arrays | None, fits, first_long_line, lines)."""
        vmn, G = self.vmn, group or self.G
        hs = (C.c_void_p * ncomp)(*([0xdead] * ncomp))
        n, long_line, fits = C.c_size_t(7), C.c_size_t(7), C.c_int(7)
        rc = vmn.lib().vmn_ec_arrays_from_textlines(G._h if G is not None else None, C.c_size_t(ncomp), text, C.c_size_t(len(text)), hs,
                                                    C.byref(n), C.byref(fits), C.byref(long_line))
        if rc != 0 or not fits.value:
            if rc != VMN_ERR_ARG:                                          # (a refused argument list touches nothing)
                assert all(h is None for h in hs), "a refused text left an array behind"
            return rc, None, False, long_line.value, n.value
        return rc, [vmn.PGroupElementArray(G, C.c_void_p(h)) for h in hs], True, long_line.value, n.value

    def decode(self, comps, cap=None, fill=b"\xa5", flags=True):
        """vmn_ec_arrays_to_textlines as it is: (status, the whole buffer, written, all_wellformed, all_utf8)."""
        lib = self.vmn.lib()
        n = comps[0].size()
        if cap is None:
            cap = max(1, n * (len(comps) * self.L + 1))
        hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
        out = C.create_string_buffer(fill * (cap + 8), cap + 8)
        written, wf, utf8 = C.c_size_t(12345), C.c_int(7), C.c_int(7)
        rc = lib.vmn_ec_arrays_to_textlines(hs, C.c_size_t(len(comps)), out, C.c_size_t(cap), C.byref(written),
                                            C.byref(wf) if flags else None, C.byref(utf8) if flags else None)
        assert out.raw[cap:] == fill * 8, "the writer wrote behind cap"
        return rc, out.raw[:cap], written.value, wf.value, utf8.value

    def upload(self, columns):
        return [self.G.toElementArray(pe.block(col, self.vb)) for col in columns]

    def live(self):
        return self.ctx.memory_stats()["live_bytes"]

    def close(self):
        self.G.close()


@pytest.fixture(scope="module")
def interface(vmn):
    from verificatum_vmn_amd import interface
    return interface


@pytest.fixture(scope="module", params=pe.GPU_CURVES)
def case(request, vmn, gpu_ctx):
    c = Case(vmn, gpu_ctx, request.param)
    yield c
    c.close()


@pytest.fixture(scope="module")
def p256(vmn, gpu_ctx):
    c = Case(vmn, gpu_ctx, "P-256")
    yield c
    c.close()


@pytest.fixture(params=("default", "1"))
def export_path(request, monkeypatch):
    """Both exports of the arrays: the Fermat inversion per point (the default at these sizes) and the batched normalisation."""
    if request.param != "default":
        monkeypatch.setenv("VMN_EC_EXPORT_NORMALISE_MIN", request.param)
    else:
        monkeypatch.delenv("VMN_EC_EXPORT_NORMALISE_MIN", raising=False)
    return request.param


def free(arrays):
    for a in arrays or []:
        a.free()


# ---- 1. the encode length, and the groups that have none ---------------------------------------------------------------------------
def test_encode_length(case, interface):
    lib = case.vmn.lib()
    assert lib.vmn_ec_group_encode_length(case.G._h) == pe.ENCODE_LENGTH[case.p.bit_length()] == interface.point_encode_length(case.G) == case.L
    assert lib.vmn_ec_group_encode_length(None) == 0


def test_modular_groups_and_a_null_group_are_refused(vmn, gpu_ctx, p256, interface):
    lib = vmn.lib()
    g, _ = load_golden(512)
    modp = vmn.ModPGroup(gpu_ctx, g["p"], g["q"], g["g"])
    try:
        assert lib.vmn_ec_group_encode_length(modp._h) == 0 == interface.point_encode_length(modp)
        before = p256.live()
        rc, arrays, fits, _, n = p256.encode(b"vote\n", 1, group=modp)
        assert rc == VMN_ERR_UNSUPPORTED and arrays is None and n == 0 and p256.live() == before
        with pytest.raises(vmn.VmnError):
            interface.encode_point_texts(modp, b"vote\n")
        members = modp.toElementArray([pow(g["g"], k, g["p"]) for k in (1, 2, 3)])
        hs = (C.c_void_p * 1)(members._h)
        out, written = C.create_string_buffer(4096), C.c_size_t(5)
        assert lib.vmn_ec_arrays_to_textlines(hs, C.c_size_t(1), out, C.c_size_t(4096), C.byref(written), None, None) == VMN_ERR_UNSUPPORTED
        assert written.value == 0
        members.free()
    finally:
        modp.close()
    hs = (C.c_void_p * 1)()
    n, first, fits = C.c_size_t(0), C.c_size_t(0), C.c_int(0)
    assert lib.vmn_ec_arrays_from_textlines(None, C.c_size_t(1), b"vote\n", C.c_size_t(5), hs, C.byref(n), C.byref(fits), C.byref(first)) == VMN_ERR_ARG


# ---- 2. encoding: the arrays are the restatement's points, bit for bit, and decode to the text ----------------------------------------
@pytest.mark.parametrize("ncomp", pe.NCOMPS)
def test_encoded_arrays_equal_the_restatement_and_decode_to_the_text(case, ncomp, export_path):
    name = case.name
    before = case.live()
    for n in pe.NS:
        text = pe.sample_text(name, ncomp, n)
        want, _ = pe.encode_text(text, name, ncomp)
        rc, arrays, fits, _, lines = case.encode(text, ncomp)
        assert rc == 0 and fits and lines == n and len(arrays) == ncomp
        for c in range(ncomp):
            assert arrays[c].size() == n
            assert arrays[c].toBytes() == pe.block(want[c], case.vb), (n, c, "the encoded array differs from the restatement")
        # and back: the same text, the verdicts those of the restatement
        rc, buf, written, wf, utf8 = case.decode(arrays)
        want_text, want_wf, want_utf8 = pe.decode_text(want, name) if n else (b"", True, True)
        assert rc == 0 and buf[:written] == want_text == text and (wf, utf8) == (int(want_wf), int(want_utf8)) and wf == 1, n
        assert buf[written:] == b"\xa5" * (len(buf) - written)
        free(arrays)
    assert case.live() == before


def test_line_ends_empty_lines_and_an_open_last_line(case, interface):
    L = case.L
    body = [b"first", b"", "zweite: grüße".encode(), b"", b"", b"x" * L, ec.G_CLEF * 3]
    for text in (b"\n".join(body) + b"\n", b"\r\n".join(body) + b"\r\n", b"\r".join(body) + b"\r", b"\n".join(body) + b"\nopen",
                 b"a\r\n\rb\n\r\nc", b"\n", b"\r\n", b"\r", b"\n\r", b"lonely", b""):
        for ncomp in (1, 2):
            lines = ec.split_lines(text)
            want, _ = pe.encode_text(text, case.name, ncomp)
            report = {}
            arrays = interface.encode_point_texts(case.G, text, ncomp, report)
            assert report == dict(fits=True, first_long_line=0, lines=len(lines)) and len(arrays) == ncomp
            assert [a.toBytes() for a in arrays] == [pe.block(col, case.vb) for col in want], text
            assert interface.decode_point_texts(arrays, report) == b"".join(ln + b"\n" for ln in lines)
            assert report["all_wellformed"] and report["all_utf8"]
            free(arrays)


@pytest.mark.parametrize("ncomp", pe.NCOMPS)
def test_a_line_that_does_not_fit_is_named_and_leaves_nothing(case, ncomp, interface):
    L = case.L
    n = 65
    lines = ec.split_lines(pe.sample_text(case.name, ncomp, n))
    warm = interface.encode_point_texts(case.G, b"\n".join(lines) + b"\n", ncomp)          # (the pool has seen these sizes)
    free(warm)
    for at in (0, 31, n - 1):
        bad = list(lines)
        bad[at] = b"y" * (ncomp * L + 1)
        bad[n - 1] = bad[n - 1] if at == n - 1 else b"z" * (ncomp * L + 7)          # a later long line is not the one named
        before = case.live()
        rc, arrays, fits, first, _ = case.encode(b"\n".join(bad) + b"\n", ncomp)
        assert rc == 0 and arrays is None and not fits and first == at
        assert case.live() == before
        report = {}
        assert interface.encode_point_texts(case.G, b"\n".join(bad), ncomp, report) is None          # (an open last line)
        assert report["fits"] is False and report["first_long_line"] == at
    exact = [b"w" * (ncomp * L)] * 3
    arrays = interface.encode_point_texts(case.G, b"\n".join(exact), ncomp)
    assert arrays is not None and interface.decode_point_texts(arrays) == b"".join(ln + b"\n" for ln in exact)
    free(arrays)


# ---- 3. decoding arrays built from crafted points ---------------------------------------------------------------------------------------
def test_y_and_the_counter_are_ignored(case, export_path):
    name = case.name
    msgs = pe.messages(name, 1) + list(ec.STRIPPED)
    points = [pe.encode_piece(m, name)[0] for m in msgs]
    want = b"".join(m.replace(b"\n", b"").replace(b"\r", b"") + b"\n" for m in msgs)
    for column in (points, [pe.negated(P, name) for P in points], [P if i % 2 else pe.negated(P, name) for i, P in enumerate(points)]):
        arrays = case.upload([column])
        rc, buf, written, wf, utf8 = case.decode(arrays)
        assert rc == 0 and buf[:written] == want and wf == 1
        free(arrays)
    column = [pe.encode_piece(b"twice", name)[0], pe.other_counter(b"twice", name), pe.negated(pe.other_counter(b"twice", name), name)]
    assert column[0][0] != column[1][0]
    arrays = case.upload([column])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"twice\n" * 3 and (wf, utf8) == (1, 1)
    free(arrays)


def test_ill_formed_points_give_empty_pieces_and_are_reported(case, export_path):
    name = case.name
    good = [pe.encode_piece(m, name)[0] for m in (b"before", b"", "da €".encode(), b"after")]
    for P in pe.ill_formed_points(name):
        for bad in (P, pe.negated(P, name)):
            column = [good[0], good[1], bad, good[2], bad, good[3]]
            arrays = case.upload([column])
            rc, buf, written, wf, utf8 = case.decode(arrays)
            assert rc == 0 and buf[:written] == b"before\n\n\nda \xe2\x82\xac\n\nafter\n" and (wf, utf8) == (0, 1), P
            assert (buf[:written], False, True) == pe.decode_text([column], name)
            free(arrays)
    # in a second component: the line keeps the first component's piece
    bad = pe.ill_formed_points(name)[0]
    arrays = case.upload([[good[0], good[3]], [bad, good[2]]])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"before\nafterda \xe2\x82\xac\n" and (wf, utf8) == (0, 1)
    free(arrays)
    # the flags may be NULL
    arrays = case.upload([[good[0], None]])
    rc, buf, written, _, _ = case.decode(arrays, flags=False)
    assert rc == 0 and buf[:written] == b"before\n\n"
    free(arrays)


def test_terminators_are_removed_and_text_that_is_not_utf8_is_reported(case, export_path):
    name, L = case.name, case.L
    inner = b"\n" + b"m" * (L - 2) + b"\r"                                          # at both ends of a full point
    msgs = list(ec.STRIPPED) + [inner, b"a\n" * (L // 2), b"\r" * L]
    column = [pe.encode_piece(m, name)[0] for m in msgs]
    arrays = case.upload([column])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and (wf, utf8) == (1, 1)
    assert buf[:written] == b"".join(m.replace(b"\n", b"").replace(b"\r", b"") + b"\n" for m in msgs) == pe.decode_text([column], name)[0]
    free(arrays)
    # C3 0A A9: not UTF-8 as it stands (Java decodes before it strips), written as C3 A9
    arrays = case.upload([[pe.encode_piece(b"fine", name)[0], pe.encode_piece(ec.C3_0A_A9, name)[0]]])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"fine\n\xc3\xa9\n" and (wf, utf8) == (1, 0)
    free(arrays)
    fine = pe.encode_piece("schön".encode(), name)[0]
    for payload in ec.BAD_UTF8 + (b"x" * (L - 2) + ec.G_CLEF[:2],):                 # (the last: cut off by the end of the point)
        column = [fine, pe.encode_piece(payload, name)[0], fine]
        arrays = case.upload([column])
        rc, buf, written, wf, utf8 = case.decode(arrays)
        assert rc == 0 and buf[:written] == "schön\n".encode() + payload + b"\n" + "schön\n".encode() and (wf, utf8) == (1, 0), payload
        assert (buf[:written], True, False) == pe.decode_text([column], name)
        free(arrays)
    # a character that straddles two components is one character; its halves in two LINES are none
    euro = ec.EURO
    halves = [pe.encode_piece(b"k" * (L - 1) + euro[:1], name)[0], pe.encode_piece(euro[1:] + b"!", name)[0]]
    arrays = case.upload([[halves[0]], [halves[1]]])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"k" * (L - 1) + euro + b"!\n" and (wf, utf8) == (1, 1)
    free(arrays)
    arrays = case.upload([halves])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"k" * (L - 1) + euro[:1] + b"\n" + euro[1:] + b"!\n" and (wf, utf8) == (1, 0)
    free(arrays)


# ---- 4. the buffer and the arguments -------------------------------------------------------------------------------------------------------
def test_cap(case):
    name, L = case.name, case.L
    for ncomp in (1, 2):
        text = pe.sample_text(name, ncomp, 65)
        cols, _ = pe.encode_text(text, name, ncomp)
        arrays = case.upload(cols)
        before = case.live()
        rc, buf, written, _, _ = case.decode(arrays, cap=len(text))
        assert rc == 0 and written == len(text) and buf == text
        rc, buf, written, _, _ = case.decode(arrays, cap=len(text) - 1)
        assert rc == VMN_ERR_ARG and written == 0 and buf == b"\xa5" * (len(text) - 1), "a short buffer must stay untouched"
        rc, buf, written, _, _ = case.decode(arrays, cap=65 * (ncomp * L + 1))
        assert rc == 0 and buf[:written] == text and buf[written:] == b"\xa5" * (len(buf) - written)
        assert case.live() == before
        free(arrays)


def test_arguments(p256):
    case = p256
    lib = case.vmn.lib()
    text = b"abc\n"
    hs = (C.c_void_p * 3)()
    n, first, fits, written = C.c_size_t(0), C.c_size_t(0), C.c_int(0), C.c_size_t(0)
    args = (C.c_size_t(len(text)), hs, C.byref(n), C.byref(fits), C.byref(first))
    assert lib.vmn_ec_arrays_from_textlines(case.G._h, C.c_size_t(0), text, *args) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_from_textlines(case.G._h, C.c_size_t(65537), text, *args) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_from_textlines(case.G._h, C.c_size_t(1), None, *args) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_from_textlines(case.G._h, C.c_size_t(1), text, C.c_size_t(len(text)), hs, None, C.byref(fits), C.byref(first)) == VMN_ERR_ARG
    a = case.upload([[pe.encode_piece(b"one", case.name)[0]] * 2])[0]
    b = case.upload([[pe.encode_piece(b"two", case.name)[0]] * 3])[0]
    out = C.create_string_buffer(1 << 12)
    one, two = (C.c_void_p * 1)(a._h), (C.c_void_p * 2)(a._h, b._h)
    assert lib.vmn_ec_arrays_to_textlines(two, C.c_size_t(2), out, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG      # sizes differ
    assert lib.vmn_ec_arrays_to_textlines(one, C.c_size_t(0), out, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_to_textlines(one, C.c_size_t(1), out, C.c_size_t(1 << 12), None, None, None) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_to_textlines(None, C.c_size_t(1), out, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_to_textlines(one, C.c_size_t(1), None, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG
    assert lib.vmn_ec_arrays_to_textlines(one, C.c_size_t(1), out, C.c_size_t(1 << 12), C.byref(written), None, None) == 0
    assert out.raw[:written.value] == b"one\none\n"
    free([a, b])


# ---- 5. the Python functions, the tool and the demo ciphertexts ----------------------------------------------------------------------------
def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmn_point_texts.py")] + list(args), capture_output=True, text=True,
                          timeout=120)


class Tape:
    """Exponents from a hashed stream (what demo_point_ciphertexts asks of its random source)."""

    def __init__(self, tag, q):
        self.tag, self.q, self.calls = tag, q, 0

    def ring_array(self, n):
        self.calls += 1
        nb = (self.q.bit_length() + 7) // 8 + 8
        raw = ec.stream(self.tag + b"/%d" % self.calls, n * nb)
        return [int.from_bytes(raw[i * nb:(i + 1) * nb], "big") % self.q for i in range(n)]


def test_the_python_functions_and_the_tool_agree_with_the_c_calls_on_a_file(p256, interface, tmp_path):
    case = p256
    text = pe.sample_text(case.name, 2, 65)
    src, raw, back, long_text = (str(tmp_path / f) for f in ("in.txt", "plain.bt", "back.txt", "long.txt"))
    open(src, "wb").write(text)
    rc, arrays, fits, _, _ = case.encode(text, 2)
    assert rc == 0 and fits
    report = {}
    mine = interface.read_point_texts(case.G, src, 2, report)
    assert report == dict(fits=True, first_long_line=0, lines=65)
    assert [a.toBytes() for a in mine] == [a.toBytes() for a in arrays]
    assert interface.read_point_texts(case.G, str(tmp_path / "nowhere"), 2) is None
    interface.write_plaintexts(raw + ".mine", mine, "raw")
    interface.write_decoded_point_plaintexts(back + ".mine", mine)
    assert open(back + ".mine", "rb").read() == text == case.decode(arrays)[1][:len(text)]
    r = run_tool("-encode", "-width", "2", "--curve", "P-256", "--wire", "natural", src, raw)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(raw, "rb").read() == open(raw + ".mine", "rb").read()
    r = run_tool("-decode", "-width", "2", "--curve", "P-256", "--wire", "natural", raw, back)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(back, "rb").read() == text
    open(long_text, "wb").write(b"short\n" + b"x" * (2 * case.L + 1) + b"\n")
    os.remove(raw)
    r = run_tool("-encode", "-width", "2", "--curve", "P-256", "--wire", "natural", long_text, raw)
    assert r.returncode == 1 and "line 2 " in r.stderr and not os.path.exists(raw), (r.returncode, r.stderr[-2000:])
    free(arrays + mine)


@pytest.mark.parametrize("width", (1, 3))
def test_demo_point_ciphertexts_open_to_the_demo_texts(p256, interface, width):
    G = p256.G
    n = 65
    x = int.from_bytes(ec.stream(b"point-texts/secret", 40), "big") % G.q
    y = G.k_exp(G.g, x)
    texts = interface.demo_texts(n, width * p256.L)
    assert texts == ec.demo_texts(n, width * 26)
    before = p256.live()
    W = interface.demo_point_ciphertexts(G, y, n, Tape(b"point-texts/tape", G.q), width)
    assert len(W) == 2 * width and all(a.size() == n for a in W)
    plain = []
    for u, v in zip(W[:width], W[width:]):
        s = u.exp(x)
        si = s.inv()
        plain.append(v.mul(si))
        free([s, si])
    want, _ = pe.encode_text(texts, "P-256", width)
    assert [a.toBytes() for a in plain] == [pe.block(col, p256.vb) for col in want]
    assert all(a.toBytes() != m.toBytes() for a, m in zip(W[width:], plain))           # (encrypted, not the messages themselves)
    report = {}
    assert interface.decode_point_texts(plain, report) == texts and report == dict(all_wellformed=True, all_utf8=True)
    free(W + plain)
    assert p256.live() == before
