"""CPU suite: the tokenizer of the json ciphertext interface (csrc/jsonlines_layout.h) as host code under AddressSanitizer and
UBSan, through a stand-alone program (tests/jsonlines_layout_harness.cpp) that walks every line of a text as k_jsonlines_scan
does and prints its verdict and the digit spans.  Over the whole catalogue of tests/jsonlines_cases.py the verdicts equal the
Python reader's, line by line, the smallest defective line is the one parse() names, and the spans spell the values."""
import os
import subprocess

import pytest

from conftest import ROOT

import jsonlines_cases as jc
from hexlines_cases import split_lines

SHAPES = [(1, 5), (2, 4), (3, 5)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jsonlines") / "jsonlines_layout_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "jsonlines_layout_harness.cpp")], check=True)
    return exe


def walk(exe, tmp_path, w, text):
    """[None | row] per line of the text, as the header's tokenizer sees it."""
    path = str(tmp_path / "text")
    with open(path, "wb") as f:
        f.write(text)
    r = subprocess.run([exe, "lines", str(w), path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    out = []
    for line in r.stdout.split("\n")[:-1]:
        if line == "bad":
            out.append(None)
            continue
        row = [None] * (2 * w)
        for item in line.split(" ")[1:]:
            c, begin, count = (int(v) for v in item.split(":"))
            assert row[c] is None
            digits = text[begin:begin + count]
            assert digits.isdigit() or count == 0
            assert count == 0 or digits[0:1] != b"0"            # leading zeros are stripped
            row[c] = int(digits or b"0")
        out.append(row)
    return out


def verdict(lines):
    bad = [k for k, row in enumerate(lines) if row is None]
    return (False, bad[0], None) if bad else (True, 0, lines)


@pytest.mark.parametrize("w,n", SHAPES)
def test_the_tokenizer_is_the_python_reader_on_the_catalogue(harness, tmp_path, w, n):
    rows = jc.synthetic_rows(w, n)
    texts = [(label, text) for label, text in jc.valid_variants(w, rows).items()] + [(label, text) for label, text, _ in jc.defects(w, rows)]
    assert len(texts) > 100
    for label, text in texts:
        got = walk(harness, tmp_path, w, text)
        lines = split_lines(text)
        assert len(got) == len(lines), label
        for k, line in enumerate(lines):
            assert (got[k] is None) == jc.line_defect(w, line), (label, k)
            if got[k] is not None:
                assert got[k] == jc.decode_line(w, line), (label, k)
        assert verdict(got) == jc.parse(text, w), label


def test_long_numbers_and_the_eight_digit_steps(harness, tmp_path):
    """Digit runs of every length around the eight-byte steps, a non-digit at every offset of such a step, and a number that the
    end of the text closes (the last line has no terminator and its last bytes are digits)."""
    for length in list(range(1, 27)) + [617, 925, 4000]:
        v = int("7" + "0123456789"[length % 10] * (length - 1))
        text = jc.text_of(1, [[v, 1], [2, v]])
        assert walk(harness, tmp_path, 1, text) == [[v, 1], [2, v]]
        cut = text[:-3]                                             # ..."beta":"ddd  -- the text ends inside the number
        assert walk(harness, tmp_path, 1, cut) == [[v, 1], None]
        for off in range(min(length, 17)):
            at = text.index(b'"alpha":"') + 9 + off
            broken = text[:at] + b"a" + text[at + 1:]
            assert walk(harness, tmp_path, 1, broken) == [None, [2, v]], (length, off)


def test_the_sizes_the_interface_documents(harness):
    for dmax, w in ((154, 1), (617, 1), (617, 3), (925, 2)):
        r = subprocess.run([harness, "sizes", str(dmax), str(w)], capture_output=True, text=True)
        assert r.returncode == 0
        cipher, plain = (int(v) for v in r.stdout.split())
        top = 10 ** dmax - 1
        assert cipher == len(jc.text_of(w, [[top] * (2 * w)])) == jc.max_line_bytes(dmax, w)
        assert plain == len(jc.plain_text_of(w, [[top] * w]))


def test_usage_errors(harness):
    for args in ([], ["lines", "0", "/dev/null"], ["rows", "1", "/dev/null"], ["sizes", "0", "1"]):
        assert subprocess.run([harness] + args, capture_output=True).returncode == 2
