"""CPU suite: the restatement of the safe-prime message encoding (tests/encode_cases.py) checks itself over the five golden
groups: every encoded element lies in the group and is v or p - v, decoding inverts encoding, both signs occur, the UTF-8
verdict is that of bytes.decode, lines are split as Java's readLine splits them, and the hard-coded group of another cofactor
is the one the seeded search finds.  No GPU, no library."""
import pytest

from conftest import load_golden

import encode_cases as ec


@pytest.fixture(scope="module", params=ec.GROUP_BITS)
def group(request):
    grpd, _ = load_golden(request.param)
    return request.param, grpd["p"], grpd["q"]


def test_the_golden_groups_are_safe_primes_that_hold_the_table(group):
    bits, p, q = group
    L = ec.encode_length(p)
    assert L == ec.ENCODE_LENGTH[bits]
    assert p == 2 * q + 1 and p % 4 == 3 and 1 << (8 * (L + 4)) <= q
    assert ec.jacobi(p - 1, p) == -1


def test_every_row_is_a_member_and_decodes_to_itself(group):
    bits, p, q = group
    L = ec.encode_length(p)
    kept = negated = 0
    for ncomp in ec.NCOMPS:
        for msg in ec.messages(L, ncomp):
            elements = ec.encode_message(msg, p, ncomp)
            assert len(elements) == ncomp
            for piece, e in zip(ec.pieces(msg, ncomp, L), elements):
                v = ec.value_of(piece, L)
                assert 0 < v < 1 << (8 * (L + 4))
                assert e in (v, p - v) and pow(e, q, p) == 1
                assert ec.jacobi(e, p) == 1 and ec.jacobi(p - e, p) == -1
                kept += e == v
                negated += e != v
                assert ec.decode_element(e, p) == (piece, True) == ec.decode_element(p - e, p)
            line, wellformed, utf8 = ec.decode_line(elements, p)
            assert line == msg + b"\n" and wellformed
            assert utf8 == _decodes(msg)
    assert kept >= 1 and negated >= 1, "both signs must occur in every group's sample"


def _decodes(data: bytes) -> bool:
    try:
        data.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def test_the_utf8_verdict_is_that_of_bytes_decode():
    samples = list(ec.BAD_UTF8) + list(ec.STRIPPED) + [ec.C3_0A_A9, b"", b"plain", ec.E_ACUTE, ec.EURO, ec.G_CLEF,
                                                       b"\xe0\x9f\xbf", b"\xe0\xa0\x80", b"\xed\x9f\xbf", b"\xee\x80\x80", b"\xf0\x8f\xbf\xbf",
                                                       b"\xf0\x90\x80\x80", b"\xf4\x8f\xbf\xbf", b"\xf5\x80\x80\x80", b"\xc1\xbf", b"\xc2\x80",
                                                       b"\xdf\xbf", b"\xc2", b"\xc2\xc2\x80", b"\xe2\x82\xac\xe2\x82"]
    samples += [ec.stream(b"utf8/%d" % k, 1 + k % 9) for k in range(400)]
    samples += [m for m in ec.messages(59, 2)]
    for s in samples:
        assert ec.utf8_wellformed(s) == _decodes(s), s
    assert not any(ec.utf8_wellformed(s) for s in ec.BAD_UTF8) and not ec.utf8_wellformed(ec.C3_0A_A9)


def test_ill_formed_values_and_stripping(group):
    bits, p, q = group
    L = ec.encode_length(p)
    for v in ec.ill_formed_values(p):
        e = ec.member_of(v, p)
        assert pow(e, q, p) == 1 and 0 < v <= q
        assert ec.decode_element(e, p) == (b"", False) == ec.decode_element(p - e, p)
    good = ec.encode_piece(b"kept", p)
    bad = ec.member_of(ec.ill_formed_values(p)[0], p)
    assert ec.decode_text([[good, bad, good]], p) == (b"kept\n\nkept\n", False, True)
    for payload in ec.STRIPPED:
        line, wf, utf8 = ec.decode_line([ec.member_of(ec.value_of(payload, L), p)], p)
        assert line == payload.replace(b"\n", b"").replace(b"\r", b"") + b"\n" and wf and utf8
    line, wf, utf8 = ec.decode_line([ec.member_of(ec.value_of(ec.C3_0A_A9, L), p)], p)
    assert (line, wf, utf8) == (b"\xc3\xa9\n", True, False)
    # the bytes behind the message are ignored
    v = int.from_bytes((2).to_bytes(4, "big") + b"hi" + b"\xaa" * (L - 2), "big")
    assert ec.decode_element(ec.member_of(v, p), p) == (b"hi", True)


def test_lines_are_split_as_readline_splits_them():
    assert ec.split_lines(b"") == []
    assert ec.split_lines(b"a\nb\r\nc\rd") == [b"a", b"b", b"c", b"d"]
    assert ec.split_lines(b"\n\n") == [b"", b""] and ec.split_lines(b"\r\n") == [b""] and ec.split_lines(b"\n\r") == [b"", b""]
    assert ec.split_lines(b"x\n") == [b"x"] and ec.split_lines(b"x") == [b"x"]
    text = b"one\r\n\r\ntwo\rthree\n\nopen"
    assert ec.split_lines(text) == [ln.encode() for ln in text.decode().splitlines()]


def test_texts_round_trip_and_long_lines_are_named(group):
    bits, p, q = group
    L = ec.encode_length(p)
    for ncomp in ec.NCOMPS:
        text = ec.sample_text(L, ncomp, 40)
        cols, _ = ec.encode_text(text, p, ncomp)
        assert len(cols) == ncomp and all(len(c) == 40 for c in cols)
        assert ec.decode_text(cols, p)[0] == text
        long_line = b"x" * (ncomp * L + 1)
        for at in (0, 20, 39):
            lines = ec.split_lines(text)
            lines[at] = long_line
            assert ec.encode_text(b"\n".join(lines) + b"\n", p, ncomp) == (None, at)


def test_demo_texts():
    assert ec.demo_texts(3, 5) == b"00000\n00001\n00002\n"
    assert ec.demo_texts(30, 1) == b"".join(bytes([65 + i % 26]) + b"\n" for i in range(30)) and ec.demo_texts(30, 1)[52:54] == b"A\n"
    assert ec.demo_texts(0, 59) == b""


def test_the_group_of_another_cofactor_is_the_one_the_search_finds():
    p, q, g = ec.search_cofactor_group()
    assert (p, q, g) == (ec.COFACTOR_P, ec.COFACTOR_Q, ec.COFACTOR_G)
    assert p.bit_length() == 512 and (p - 1) % q == 0 and (p - 1) // q > 2 and ec.is_probable_prime(p) and ec.is_probable_prime(q)
    assert 1 < g < p and pow(g, q, p) == 1
