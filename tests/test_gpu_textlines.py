"""GPU suite: plaintexts as text -- messages encoded as elements of a safe-prime group and decoded again (include/vmnhip.h:
vmn_group_encode_length, vmn_garrays_from_textlines, vmn_garrays_to_textlines; csrc/encode_kernels.h: k_textlines_records / _fold /
_lengths / _emit; csrc/modp_kernels.h: k_jacobi_fix, k_jacobi_fix_lanes; verificatum_vmn_amd/interface.py; tools/vmn_texts.py)
against tests/encode_cases.py, the rule restated on Python integers, by exact equality: arrays through toBytes, texts byte for byte.

Groups: the golden groups of 512, 1024 and 2048 bits (one lane per element), 3072 and 4096 bits (the element's own lanes), at the
bytes of the modulus, and the 1024-bit group once more at the reference's wider leaf width.  n in {0, 1, 2, 63, 64, 65, 257, 1000},
1, 2 and 3 components, messages of 0, 1, L - 1, L, L + 1, ncomp L - 1 and ncomp L bytes."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from conftest import ROOT, load_golden

import encode_cases as ec

pytestmark = pytest.mark.gpu

GROUPS = ["modp512", "modp1024", "modp1024-java", "modp2048", "modp3072", "modp4096"]
VMN_ERR_ARG, VMN_ERR_UNSUPPORTED = -1, -5


class Case:
    """One group and the calls of the C ABI as they are."""

    def __init__(self, vmn, ctx, name):
        self.vmn, self.ctx, self.name = vmn, ctx, name
        self.bits = int(name[4:].split("-")[0])
        g, _ = load_golden(self.bits)
        self.p, self.q = g["p"], g["q"]
        self.G = vmn.ModPGroup(ctx, g["p"], g["q"], g["g"], nbytes=None if name.endswith("-java") else self.bits // 8)
        self.vb = self.G.nbytes
        self.L = ec.encode_length(self.p)

    def encode(self, text, ncomp, group=None):
        """vmn_garrays_from_textlines as it is: (status, arrays | None, fits, first_long_line, lines)."""
        vmn, G = self.vmn, group or self.G
        hs = (C.c_void_p * ncomp)(*([0xdead] * ncomp))
        n, long_line, fits = C.c_size_t(7), C.c_size_t(7), C.c_int(7)
        rc = vmn.lib().vmn_garrays_from_textlines(G._h, C.c_size_t(ncomp), text, C.c_size_t(len(text)), hs, C.byref(n), C.byref(fits),
                                                  C.byref(long_line))
        if rc != 0 or not fits.value:
            assert all(h is None for h in hs), "a refused text left an array behind"
            return rc, None, False, long_line.value, n.value
        return rc, [vmn.PGroupElementArray(G, C.c_void_p(h)) for h in hs], True, long_line.value, n.value

    def decode(self, comps, cap=None, fill=b"\xa5", flags=True):
        """vmn_garrays_to_textlines as it is: (status, the whole buffer, written, all_wellformed, all_utf8)."""
        lib = self.vmn.lib()
        n = comps[0].size()
        if cap is None:
            cap = max(1, n * (len(comps) * self.L + 1))
        hs = (C.c_void_p * len(comps))(*[a._h for a in comps])
        out = C.create_string_buffer(fill * (cap + 8), cap + 8)
        written, wf, utf8 = C.c_size_t(12345), C.c_int(7), C.c_int(7)
        rc = lib.vmn_garrays_to_textlines(hs, C.c_size_t(len(comps)), out, C.c_size_t(cap), C.byref(written),
                                          C.byref(wf) if flags else None, C.byref(utf8) if flags else None)
        assert out.raw[cap:] == fill * 8, "the writer wrote behind cap"
        return rc, out.raw[:cap], written.value, wf.value, utf8.value

    def upload(self, columns):
        return [self.G.toElementArray(b"".join(v.to_bytes(self.vb, "big") for v in col)) for col in columns]

    def block(self, column):
        return b"".join(v.to_bytes(self.vb, "big") for v in column)

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


# ---- 1. the encode length, and the groups that have none ---------------------------------------------------------------------------
def test_encode_length(case, interface):
    lib = case.vmn.lib()
    assert lib.vmn_group_encode_length(case.G._h) == ec.ENCODE_LENGTH[case.bits] == interface.encode_length(case.G) == case.L
    assert lib.vmn_group_encode_length(None) == 0


def test_curves_and_other_cofactors_are_unsupported(vmn, gpu_ctx, modp512, interface):
    lib = vmn.lib()
    curve = vmn.ECqPGroup(gpu_ctx, "P-256")
    other = vmn.ModPGroup(gpu_ctx, ec.COFACTOR_P, ec.COFACTOR_Q, ec.COFACTOR_G, nbytes=64)
    try:
        for G in (curve, other):
            assert lib.vmn_group_encode_length(G._h) == 0 == interface.encode_length(G)
            rc, arrays, fits, _, n = modp512.encode(b"vote\n", 1, group=G)
            assert rc == VMN_ERR_UNSUPPORTED and arrays is None and n == 0
            with pytest.raises(vmn.VmnError):
                interface.encode_texts(G, b"vote\n")
        members = other.toElementArray([pow(ec.COFACTOR_G, k, ec.COFACTOR_P) for k in (1, 2, 3)])
        hs = (C.c_void_p * 1)(members._h)
        out, written = C.create_string_buffer(4096), C.c_size_t(5)
        assert lib.vmn_garrays_to_textlines(hs, C.c_size_t(1), out, C.c_size_t(4096), C.byref(written), None, None) == VMN_ERR_UNSUPPORTED
        assert written.value == 0
        members.free()
    finally:
        curve.close()
        other.close()


# ---- 2. encoding: the arrays are the restatement's elements, bit for bit, and members -----------------------------------------------
@pytest.mark.parametrize("ncomp", ec.NCOMPS)
def test_encoded_arrays_equal_the_restatement_and_decode_to_the_text(case, ncomp, interface):
    p, L = case.p, case.L
    signs = set()
    for n in ec.NS:
        text = ec.sample_text(L, ncomp, n, tag=case.name.encode())
        want, _ = ec.encode_text(text, p, ncomp)
        rc, arrays, fits, _, lines = case.encode(text, ncomp)
        assert rc == 0 and fits and lines == n and len(arrays) == ncomp
        for c in range(ncomp):
            assert arrays[c].size() == n
            assert arrays[c].toBytes() == case.block(want[c]), (n, c, "the encoded array differs from the restatement")
            assert arrays[c].isMember()
            signs |= {e == ec.value_of(piece, L) for e, line in zip(want[c], ec.split_lines(text))
                      for piece in [ec.pieces(line, ncomp, L)[c]]}
        # and back: the same text, the verdicts those of the restatement
        rc, buf, written, wf, utf8 = case.decode(arrays)
        want_text, want_wf, want_utf8 = ec.decode_text(want, p) if n else (b"", True, True)
        assert rc == 0 and buf[:written] == want_text == text and (wf, utf8) == (int(want_wf), int(want_utf8)), n
        assert buf[written:] == b"\xa5" * (len(buf) - written)
        free(arrays)
    assert signs == {True, False}, "the sample must hold values that are kept and values that are negated"


def test_line_ends_empty_lines_and_an_open_last_line(case, interface):
    L = case.L
    body = [b"first", b"", "zweite Zeile: grüße".encode(), b"", b"", b"x" * L, ec.G_CLEF * 3]
    for text in (b"\n".join(body) + b"\n", b"\r\n".join(body) + b"\r\n", b"\r".join(body) + b"\r", b"\n".join(body) + b"\nopen",
                 b"a\r\n\rb\n\r\nc", b"\n", b"\r\n", b"\r", b"\n\r", b"lonely", b""):
        for ncomp in (1, 2):
            lines = ec.split_lines(text)
            want, _ = ec.encode_text(text, case.p, ncomp)
            report = {}
            arrays = interface.encode_texts(case.G, text, ncomp, report)
            assert report == dict(fits=True, first_long_line=0, lines=len(lines)) and len(arrays) == ncomp
            assert [a.toBytes() for a in arrays] == [case.block(col) for col in want], text
            # the round trip: every line end normalised to \n
            assert interface.decode_texts(arrays, report) == b"".join(ln + b"\n" for ln in lines)
            assert report["all_wellformed"] and report["all_utf8"]
            free(arrays)


@pytest.mark.parametrize("ncomp", ec.NCOMPS)
def test_a_line_that_does_not_fit_is_named_and_leaves_nothing(case, ncomp, interface):
    L = case.L
    n = 65
    lines = ec.split_lines(ec.sample_text(L, ncomp, n))
    warm = interface.encode_texts(case.G, b"\n".join(lines) + b"\n", ncomp)          # (the pool has seen these sizes)
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
        assert interface.encode_texts(case.G, b"\n".join(bad), ncomp, report) is None          # (an open last line)
        assert report["fits"] is False and report["first_long_line"] == at
    exact = [b"w" * (ncomp * L)] * 3
    arrays = interface.encode_texts(case.G, b"\n".join(exact), ncomp)
    assert arrays is not None and interface.decode_texts(arrays) == b"".join(ln + b"\n" for ln in exact)
    free(arrays)


# ---- 3. decoding arrays built from crafted integers ------------------------------------------------------------------------------------
def test_v_and_p_minus_v_decode_alike(case):
    p, L = case.p, case.L
    msgs = [m for m in ec.messages(L, 1)] + list(ec.STRIPPED)
    vs = [ec.value_of(m, L) for m in msgs]
    want = b"".join(m.replace(b"\n", b"").replace(b"\r", b"") + b"\n" for m in msgs)
    for column in (vs, [p - v for v in vs], [v if i % 2 else p - v for i, v in enumerate(vs)]):
        arrays = case.upload([column])
        rc, buf, written, wf, utf8 = case.decode(arrays)
        assert rc == 0 and buf[:written] == want and wf == 1
        free(arrays)


def test_ill_formed_elements_give_empty_pieces_and_are_reported(case):
    p, L = case.p, case.L
    good = [ec.encode_piece(m, p) for m in (b"before", b"", "dazwischen €".encode(), b"after")]
    for v in ec.ill_formed_values(p):
        for bad in (ec.member_of(v, p), p - ec.member_of(v, p)):
            column = [good[0], good[1], bad, good[2], bad, good[3]]
            arrays = case.upload([column])
            rc, buf, written, wf, utf8 = case.decode(arrays)
            assert rc == 0 and buf[:written] == b"before\n\n\ndazwischen \xe2\x82\xac\n\nafter\n" and (wf, utf8) == (0, 1)
            assert (buf[:written], False, True) == ec.decode_text([column], p)
            free(arrays)
    # in a second component: the line keeps the first component's piece
    bad = ec.member_of(ec.ill_formed_values(p)[0], p)
    arrays = case.upload([[good[0], good[3]], [bad, good[2]]])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"before\nafterdazwischen \xe2\x82\xac\n" and (wf, utf8) == (0, 1)
    free(arrays)
    # the flags may be NULL
    arrays = case.upload([[good[0], bad]])
    rc, buf, written, _, _ = case.decode(arrays, flags=False)
    assert rc == 0 and buf[:written] == b"before\n\n"
    free(arrays)


def test_line_terminators_inside_a_message_are_removed(case):
    p, L = case.p, case.L
    inner = b"\n" + b"m" * (L - 2) + b"\r"                                          # at both ends of a full element
    msgs = list(ec.STRIPPED) + [inner, b"a\n" * (L // 2), b"\r" * L]
    column = [ec.member_of(ec.value_of(m, L), p) for m in msgs]
    arrays = case.upload([column])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and (wf, utf8) == (1, 1)
    assert buf[:written] == b"".join(m.replace(b"\n", b"").replace(b"\r", b"") + b"\n" for m in msgs) == ec.decode_text([column], p)[0]
    free(arrays)
    # C3 0A A9: not UTF-8 as it stands (Java decodes before it strips), written as C3 A9
    arrays = case.upload([[ec.member_of(ec.value_of(b"fine", L), p), ec.member_of(ec.value_of(ec.C3_0A_A9, L), p)]])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"fine\n\xc3\xa9\n" and (wf, utf8) == (1, 0)
    free(arrays)


def test_text_that_is_not_utf8_is_reported_and_written_unchanged(case):
    p, L = case.p, case.L
    fine = ec.member_of(ec.value_of("schön".encode(), L), p)
    for payload in ec.BAD_UTF8 + (b"x" * (L - 2) + ec.G_CLEF[:2],):                 # (the last: cut off by the end of the element)
        assert not ec.utf8_wellformed(payload)
        column = [fine, ec.member_of(ec.value_of(payload, L), p), fine]
        arrays = case.upload([column])
        rc, buf, written, wf, utf8 = case.decode(arrays)
        assert rc == 0 and buf[:written] == "schön\n".encode() + payload + b"\n" + "schön\n".encode() and (wf, utf8) == (1, 0), payload
        free(arrays)
    # a character that straddles two components is one character; its halves in two LINES are none
    euro = ec.EURO
    halves = [ec.member_of(ec.value_of(b"k" * (L - 1) + euro[:1], L), p), ec.member_of(ec.value_of(euro[1:] + b"!", L), p)]
    arrays = case.upload([[halves[0]], [halves[1]]])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"k" * (L - 1) + euro + b"!\n" and (wf, utf8) == (1, 1)
    free(arrays)
    arrays = case.upload([halves])
    rc, buf, written, wf, utf8 = case.decode(arrays)
    assert rc == 0 and buf[:written] == b"k" * (L - 1) + euro[:1] + b"\n" + euro[1:] + b"!\n" and (wf, utf8) == (1, 0)
    free(arrays)


# ---- 4. the buffer ------------------------------------------------------------------------------------------------------------------------
def test_cap(case):
    p, L = case.p, case.L
    for ncomp in (1, 2):
        text = ec.sample_text(L, ncomp, 65)
        cols, _ = ec.encode_text(text, p, ncomp)
        arrays = case.upload(cols)
        rc, buf, written, _, _ = case.decode(arrays, cap=len(text))
        assert rc == 0 and written == len(text) and buf == text
        rc, buf, written, _, _ = case.decode(arrays, cap=len(text) - 1)
        assert rc == VMN_ERR_ARG and written == 0 and buf == b"\xa5" * (len(text) - 1), "a short buffer must stay untouched"
        rc, buf, written, _, _ = case.decode(arrays, cap=65 * (ncomp * L + 1))
        assert rc == 0 and buf[:written] == text and buf[written:] == b"\xa5" * (len(buf) - written)
        free(arrays)


def test_arguments(case):
    lib = case.vmn.lib()
    text = b"abc\n"
    hs = (C.c_void_p * 3)()
    n, first, fits, written = C.c_size_t(0), C.c_size_t(0), C.c_int(0), C.c_size_t(0)
    args = (C.c_size_t(len(text)), hs, C.byref(n), C.byref(fits), C.byref(first))
    assert lib.vmn_garrays_from_textlines(case.G._h, C.c_size_t(0), text, *args) == VMN_ERR_ARG
    assert lib.vmn_garrays_from_textlines(case.G._h, C.c_size_t(65537), text, *args) == VMN_ERR_ARG
    assert lib.vmn_garrays_from_textlines(None, C.c_size_t(1), text, *args) == VMN_ERR_ARG
    assert lib.vmn_garrays_from_textlines(case.G._h, C.c_size_t(1), None, *args) == VMN_ERR_ARG
    assert lib.vmn_garrays_from_textlines(case.G._h, C.c_size_t(1), text, C.c_size_t(len(text)), hs, None, C.byref(fits), C.byref(first)) == VMN_ERR_ARG
    a = case.upload([[ec.encode_piece(b"one", case.p)] * 2])[0]
    b = case.upload([[ec.encode_piece(b"two", case.p)] * 3])[0]
    out = C.create_string_buffer(1 << 12)
    one, two = (C.c_void_p * 1)(a._h), (C.c_void_p * 2)(a._h, b._h)
    assert lib.vmn_garrays_to_textlines(two, C.c_size_t(2), out, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG      # sizes differ
    assert lib.vmn_garrays_to_textlines(one, C.c_size_t(0), out, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_textlines(one, C.c_size_t(1), out, C.c_size_t(1 << 12), None, None, None) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_textlines(None, C.c_size_t(1), out, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_textlines(one, C.c_size_t(1), None, C.c_size_t(1 << 12), C.byref(written), None, None) == VMN_ERR_ARG
    assert lib.vmn_garrays_to_textlines(one, C.c_size_t(1), out, C.c_size_t(1 << 12), C.byref(written), None, None) == 0
    assert out.raw[:written.value] == b"one\none\n"
    free([a, b])


# ---- 5. end to end: demo ciphertexts through a whole session, and the tool ---------------------------------------------------------------
def run_tool(*args):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "vmn_texts.py")] + list(args), capture_output=True, text=True,
                          timeout=120)


def test_demo_ciphertexts_through_a_session_come_out_as_the_demo_texts(entry, vmn, gpu_ctx, interface, tmp_path):
    import mirror
    import session_cases as S
    mods = mirror.load(entry, ("proofdir", "randomsource", "fiatshamir", "native"))
    pd, rs = mods["proofdir"], mods["randomsource"]
    grpd, _ = load_golden(512)
    p, q, g = grpd["p"], grpd["q"], grpd["g"]
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    params = S.gpu_params(G, "ModPGroup(512)", {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(g, "x")})
    n = 65
    tape = rs.InsecureShaRandomSource(b"textlines-tape", q)
    coeffs = tape.ring_array(S.THR)
    shares = [None] + [sum(c * pow(l, d, q) for d, c in enumerate(coeffs)) % q for l in range(1, S.K + 1)]
    poly = [G.k_exp(G.g, c) for c in coeffs]
    y = poly[0]
    texts = interface.demo_texts(n, interface.encode_length(G))
    assert texts == ec.demo_texts(n, 59) and texts[:60] == b"0" * 59 + b"\n"
    W = interface.demo_ciphertexts(G, y, n, tape)
    assert len(W) == 2 and all(a.size() == n and a.isMember() for a in W)
    nizkp = str(tmp_path / "nizkp")
    written, plain = pd.write_session(nizkp, G, params, "mixing", W, y, rs.InsecureShaRandomSource(b"textlines-prover", q), S.K, S.THR,
                                      poly=poly, shares=shares)
    assert pd.verify_session(nizkp, G, written).accepted
    report = {}
    decoded = interface.decode_texts(plain, report)
    assert report == dict(all_wellformed=True, all_utf8=True)
    assert sorted(decoded.split(b"\n")) == sorted(texts.split(b"\n")) and decoded != texts          # the same votes, mixed
    # the file the session left behind, by the library and by the tool
    mine, tools = str(tmp_path / "mine.txt"), str(tmp_path / "tool.txt")
    from_file = interface.read_plaintexts(G, pd.plaintexts_file(nizkp), 1)
    interface.write_decoded_plaintexts(mine, from_file)
    assert open(mine, "rb").read() == decoded
    r = run_tool("-decode", "--params", os.path.join(nizkp, "params.json"), pd.plaintexts_file(nizkp), tools)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(tools, "rb").read() == decoded
    # and the way back: the tool's -encode, a line too long named from 1
    raw, long_text = str(tmp_path / "again.bt"), str(tmp_path / "long.txt")
    r = run_tool("-encode", "--params", os.path.join(nizkp, "params.json"), mine, raw)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(raw, "rb").read() == open(pd.plaintexts_file(nizkp), "rb").read()
    open(long_text, "wb").write(b"short\n" + b"x" * 60 + b"\n")
    os.remove(raw)
    r = run_tool("-encode", "--params", os.path.join(nizkp, "params.json"), long_text, raw)
    assert r.returncode == 1 and "line 2 " in r.stderr and not os.path.exists(raw), (r.returncode, r.stderr[-2000:])
    back = interface.read_texts(G, mine, 1)
    assert [a.toBytes() for a in back] == [a.toBytes() for a in from_file]
    free(back + from_file + list(plain) + list(W))
    G.close()
