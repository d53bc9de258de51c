"""CPU suite: the catalogue of tests/jsonlines_cases.py holds what it claims, and catches mutants of its own reader.

The GPU suite (tests/test_gpu_jsonlines.py) compares vmn_garrays_from_jsonlines with parse() on these texts; here parse() is
pinned: against Python's own json module where the two agree by definition (every accepted line is JSON holding the row), on
every valid variant, on every defect at the line the catalogue built it at, and by four mutants -- a reader that wants alpha
first, one that refuses leading zeros, one that reports the first defect found instead of the smallest index, one that lets
further keys pass -- each of which some text of the catalogue must expose."""
import json

import pytest

import jsonlines_cases as jc
from hexlines_cases import split_lines

SHAPES = [1, 2, 3]

# every defect the interface names (include/vmnhip.h) -> the label of the catalogue that holds it
NAMED_DEFECTS = {
    "a missing key": "missing-key", "a duplicate key": "duplicate-key", "an unknown key": "unknown-key", "an extra key": "extra-key",
    "an empty number": "empty-number", "a sign": "sign-minus", "a non-digit inside a number": "non-digit-inside",
    "a backslash": "backslash", "a byte >= 0x80": "high-byte", "a pair too many": "pair-count-one-more",
    "text behind the closing bracket": "text-behind", "a blank line": "blank",
}


def test_the_writer_writes_json_and_the_reader_reads_it_back():
    for w in SHAPES:
        rows = jc.synthetic_rows(w, 4)
        text = jc.text_of(w, rows)
        assert b" " not in text and text.endswith(b"\n") and text.count(b"\n") == 4
        for line, row in zip(text.split(b"\n"), rows):
            obj = json.loads(line)
            pairs = [obj] if w == 1 else obj
            assert [int(p["alpha"]) for p in pairs] + [int(p["beta"]) for p in pairs] == row
            assert all(list(p) == ["alpha", "beta"] for p in pairs)
            assert jc.decode_line(w, line) == row
        assert jc.parse(text, w) == (True, 0, rows)
        plain = jc.plain_text_of(w, [r[:w] for r in rows])
        for line, row in zip(plain.split(b"\n"), rows):
            got = json.loads(line)
            assert [int(v) for v in ([got] if w == 1 else got)] == row[:w]
    assert jc.line_of(1, [0, 10]) == b'{"alpha":"0","beta":"10"}'
    assert jc.line_of(2, [1, 2, 3, 4]) == b'[{"alpha":"1","beta":"3"},{"alpha":"2","beta":"4"}]'
    assert jc.plain_line_of(1, [7]) == b'"7"' and jc.plain_line_of(3, [7, 0, 9]) == b'["7","0","9"]'
    assert jc.max_line_bytes(3, 1) == len(b'{"alpha":"999","beta":"999"}\n')
    assert jc.max_line_bytes(3, 2) == len(b'[{"alpha":"999","beta":"999"},{"alpha":"999","beta":"999"}]\n')


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("w", SHAPES)
def test_valid_variants_hold_the_rows(w, n):
    rows = jc.synthetic_rows(w, n)
    variants = jc.valid_variants(w, rows)
    assert {"lf", "crlf", "cr", "mixed-terminators", "no-final-terminator", "swapped-keys", "json-dumps-spaces", "tabs-and-spaces",
            "leading-zeros-1", "leading-zeros-9", "every-variant-mixed"} <= set(variants)
    for label, text in variants.items():
        assert jc.parse(text, w) == (True, 0, rows), label
        assert jc.parse(text, w, n) == (True, 0, rows), label
        assert jc.parse(text, w, n + 1) == (False, n, None), label
        for line in split_lines(text):                                # every accepted line is JSON
            json.loads(line)
    if n > 1:
        assert len(set(variants.values())) == len(variants)
        assert jc.parse(variants["lf"], w, n - 1) == (False, n - 1, None)
    assert b'"beta":"' in variants["swapped-keys"][:12 + (w > 1)]
    assert b'": "' in variants["json-dumps-spaces"] and b'", "' in variants["json-dumps-spaces"] and b"\t" in variants["tabs-and-spaces"]
    assert not variants["no-final-terminator"].endswith((b"\n", b"\r"))
    assert jc.parse(b"", w) == (True, 0, [])
    assert jc.parse(b"", w, 2) == (False, 0, None)


@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("w", SHAPES)
def test_defects_are_defects_at_the_line_they_were_built_at(w, n):
    rows = jc.synthetic_rows(w, n)
    cat = jc.defects(w, rows)
    labels = {label.split("@")[0] for label, _, _ in cat}
    assert set(NAMED_DEFECTS.values()) <= labels
    assert ({"list-at-width-1"} if w == 1 else {"bare-map-at-width-w", "pair-count-one-less"}) <= labels
    assert {k for _, _, k in cat} >= set(jc.positions(n)) | {n}
    for name in set(NAMED_DEFECTS.values()):                          # each at the first, a middle and the last line
        assert {k for label, _, k in cat if label.split("@")[0] == name} == set(jc.positions(n))
    good = jc.valid_variants(w, rows)["lf"]
    later = 0
    for label, text, k in cat:
        assert text != good
        assert jc.parse(text, w) == (False, k, None), label
        bad = [i for i, line in enumerate(split_lines(text)) if jc.line_defect(w, line)]
        assert bad[0] == k
        later += len(bad) > 1
    if n >= 2:
        assert later >= len(NAMED_DEFECTS)                            # a second, later defect rides along


@pytest.mark.parametrize("mutant", jc.MUTANTS)
def test_the_catalogue_catches_every_mutant_of_the_reader(mutant):
    exposed = []
    for w in SHAPES:
        rows = jc.synthetic_rows(w, 5)
        for label, text in jc.valid_variants(w, rows).items():
            if jc.parse(text, w, mutant=mutant) != jc.parse(text, w):
                exposed.append(label)
        for label, text, _ in jc.defects(w, rows):
            if jc.parse(text, w, mutant=mutant) != jc.parse(text, w):
                exposed.append(label)
    assert exposed, mutant
    by = {jc.ORDER_SENSITIVE: "swapped-keys", jc.NO_LEADING_ZEROS: "leading-zeros", jc.FIRST_FOUND: "two-defects",
          jc.EXTRA_KEY_TOLERANT: "extra-key"}[mutant]
    assert any(label.startswith(by) for label in exposed), (mutant, exposed)
