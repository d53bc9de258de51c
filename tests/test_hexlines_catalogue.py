"""CPU suite: the catalogue of tests/hexlines_cases.py holds what it claims, and catches mutants of its own reader.

The GPU suite (tests/test_gpu_hexlines.py) compares vmn_garrays_from_hexlines with parse() on these texts; here parse() is pinned:
against Python's own line splitting where the two agree by definition, on every valid variant, on every defect at the line the
catalogue built it at, and by four mutants -- \\r\\n counted twice, a case-sensitive hex check, the length check dropped, the first
defect found reported instead of the smallest index -- each of which some text of the catalogue must expose."""
import pytest

import hexlines_cases as hc

SHAPES = [(False, 64, 1), (False, 65, 3), (True, 32, 1), (True, 33, 3)]
IDS = ["%s-%d-w%d" % ("curve" if c else "modp", vb, w) for c, vb, w in SHAPES]


def test_line_splitting_is_readline():
    s = hc.split_lines
    assert s(b"") == []
    assert s(b"ab") == [b"ab"]
    assert s(b"ab\n") == [b"ab"] == s(b"ab\r") == s(b"ab\r\n")
    assert s(b"ab\ncd") == [b"ab", b"cd"] == s(b"ab\rcd") == s(b"ab\r\ncd")
    assert s(b"ab\n\ncd") == [b"ab", b"", b"cd"]
    assert s(b"ab\n\rcd") == [b"ab", b"", b"cd"]             # \n\r is two terminators, \r\n one
    assert s(b"ab\r\rcd") == [b"ab", b"", b"cd"]
    assert s(b"ab\r\n\r\n") == [b"ab", b""]
    assert s(b"\n") == [b""] and s(b"\r\n") == [b""] and s(b"\n\n") == [b"", b""]
    for text in (b"a\nb\nc\n", b"a\r\nb\r\nc", b"a\rb\r\nc\n", b"\n\na"):
        assert s(text) == [l.encode() for l in text.decode().splitlines()]      # (str.splitlines agrees on these three terminators)


@pytest.mark.parametrize("curve,vb,w", SHAPES, ids=IDS)
def test_sizes_and_offsets(curve, vb, w):
    rows = hc.synthetic_rows(curve, vb, w, 3)
    B = hc.line_bytes(curve, vb, w)
    for r in rows:
        line = hc.line_of(curve, w, r)
        assert len(line) == 2 * B and set(line) <= hc.LOWER_HEX
        raw = bytes.fromhex(line.decode())
        for c, off in enumerate(hc.component_offsets(curve, vb, w)):
            tree, end = hc.eio.decode(raw, off)
            assert tree == hc.element_tree(curve, r[c]) and end == off + hc.element_bytes(curve, vb)
        assert hc.decode_line(curve, vb, w, line) == r
    assert hc.line_bytes(False, 256, 1) == 527 and hc.line_bytes(True, 33, 3) == 501


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("curve,vb,w", SHAPES, ids=IDS)
def test_valid_variants_hold_the_rows(curve, vb, w, n):
    rows = hc.synthetic_rows(curve, vb, w, n)
    variants = hc.valid_variants(curve, w, rows)
    assert {"lf", "crlf", "cr", "mixed", "no-final-terminator", "upper", "mixed-case"} <= set(variants)
    for label, text in variants.items():
        assert hc.parse(text, curve, vb, w) == (True, 0, rows), label
        assert hc.parse(text, curve, vb, w, n) == (True, 0, rows), label
        assert hc.parse(text, curve, vb, w, n + 1) == (False, n, None), label
    if n > 1:
        assert len(set(variants.values())) == len(variants)
        assert hc.parse(variants["lf"], curve, vb, w, n - 1) == (False, n - 1, None)
    assert b"\r\n" in variants["mixed"] or n < 2
    assert any(c in b"ABCDEF" for c in variants["mixed-case"]) and any(c in b"abcdef" for c in variants["mixed-case"])
    assert hc.parse(b"", curve, vb, w) == (True, 0, [])
    assert hc.parse(b"", curve, vb, w, 2) == (False, 0, None)


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("curve,vb,w", SHAPES, ids=IDS)
def test_defects_are_defects_at_the_line_they_were_built_at(curve, vb, w, n):
    rows = hc.synthetic_rows(curve, vb, w, n)
    cat = hc.defects(curve, vb, w, rows)
    labels = {label.split("@")[0] for label, _, _ in cat}
    want = {"nonhex-first", "nonhex-last", "one-short", "two-long", "blank", "second-terminator-at-the-end", "space-in-front",
            "node-count-3", "leaf-tag-2", "leaf-length+1"} | ({"inner-count-2"} if w > 1 else set())
    assert want <= labels
    assert {k for _, _, k in cat} >= set(hc.positions(n)) | {n}
    if n >= 2:
        assert any(label.startswith("framing@") for label, _, _ in cat) and any(label.startswith("text@") for label, _, _ in cat)
    good = hc.valid_variants(curve, w, rows)["lf"]
    for label, text, k in cat:
        assert text != good
        assert hc.parse(text, curve, vb, w) == (False, k, None), label


@pytest.mark.parametrize("mutant", hc.MUTANTS)
def test_the_catalogue_catches_every_mutant_of_the_reader(mutant):
    exposed = []
    for curve, vb, w in SHAPES:
        rows = hc.synthetic_rows(curve, vb, w, 5)
        for label, text in hc.valid_variants(curve, w, rows).items():
            if hc.parse(text, curve, vb, w, mutant=mutant) != hc.parse(text, curve, vb, w):
                exposed.append(label)
        for label, text, _ in hc.defects(curve, vb, w, rows):
            if hc.parse(text, curve, vb, w, mutant=mutant) != hc.parse(text, curve, vb, w):
                exposed.append(label)
    assert exposed, mutant
    by = {hc.CRLF_TWICE: "crlf", hc.CASE_SENSITIVE: "upper", hc.NO_LENGTH: "two-long", hc.FIRST_FOUND: "framing@"}[mutant]
    assert any(label.startswith(by) for label in exposed), (mutant, exposed)
