"""CPU suite: the grammar of the reference's ``vre`` (verificatum_vmn_amd/rearrange.py) against tests/golden/rearrange_formats.json,
strings and what ProtocolElGamalRearParser.java:53-299 makes of them -- derived by reading the parser, not by running this code.
The parser restates the Java: ``String.split`` drops trailing empty strings and keeps leading and inner ones, a number is what
``Integer.parseInt`` reads (ASCII digits only here), and the messages are the reference's."""
import json
import os

import pytest

from conftest import ROOT

with open(os.path.join(ROOT, "tests", "golden", "rearrange_formats.json"), encoding="utf-8") as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def rear(vmn):
    from verificatum_vmn_amd import rearrange
    return rearrange


def tuples(x):
    return [tuple(v) for v in x]


def check(rear, case, call, shape):
    if "error" in case:
        with pytest.raises(rear.RearrangeFormatError) as exc:
            call()
        assert str(exc.value) == case["error"], case
        assert isinstance(exc.value, ValueError)
    else:
        assert call() == shape(case["out"]), case


def test_golden_covers_the_minimum():
    """The strings the feature was specified with are all in the golden file."""
    have = {k: {c["in"] for c in GOLDEN[k]} for k in ("interval", "intervals", "positions", "source", "format", "widths")}
    assert {"0-3", "3-3", "5", "1-2-3", "-1-2", "1-", "2147483648-2147483649"} <= have["interval"]
    assert {"", ":", "0-1::2-3", "0-1:"} <= have["intervals"]
    assert {"(0-2,1-3)", "(+1,0)", "(0,)", "(0,1,2)", "( 0,0)", "(-3,0)", "(1_0,0)", "(0-2,0)"} <= have["positions"]
    assert {"(0,1)x(3,2)", "(0,1)x", "x(0,1)"} <= have["source"]
    assert {"(0,0-2):(0-1,4)"} <= have["format"]
    assert {"2:1:5", "0"} <= have["widths"]


@pytest.mark.parametrize("case", GOLDEN["interval"], ids=lambda c: repr(c["in"]))
def test_interval(rear, case):
    check(rear, case, lambda: rear.parse_interval(case["in"]), tuple)


@pytest.mark.parametrize("case", GOLDEN["intervals"], ids=lambda c: repr(c["in"]))
def test_intervals(rear, case):
    check(rear, case, lambda: rear.parse_intervals(case["in"]), tuples)


@pytest.mark.parametrize("case", GOLDEN["positions"], ids=lambda c: "%r%s" % (c["in"], "-strict" if c["strict"] else ""))
def test_positions(rear, case):
    check(rear, case, lambda: rear.parse_positions(case["in"], case["strict"]), tuples)


@pytest.mark.parametrize("case", GOLDEN["source"], ids=lambda c: repr(c["in"]))
def test_source(rear, case):
    check(rear, case, lambda: rear.parse_source(case["in"]), tuples)


@pytest.mark.parametrize("case", GOLDEN["format"], ids=lambda c: repr(c["in"]))
def test_format(rear, case):
    check(rear, case, lambda: rear.parse_format(case["in"]), lambda out: [tuples(row) for row in out])


@pytest.mark.parametrize("case", GOLDEN["widths"], ids=lambda c: repr(c["in"]))
def test_widths(rear, case):
    check(rear, case, lambda: rear.parse_widths(case["in"]), list)


def test_java_split_and_parse_int(rear):
    """The two pieces of Java the grammar stands on."""
    assert rear.java_split("", ":") == [""] and rear.java_split("a", ":") == ["a"]
    assert rear.java_split(":", ":") == [] and rear.java_split("a::", ":") == ["a"]
    assert rear.java_split(":a", ":") == ["", "a"] and rear.java_split("a::b", ":") == ["a", "", "b"]
    assert rear.parse_int("-2147483648") == -2 ** 31 and rear.parse_int("+0") == 0 and rear.parse_int("-0") == 0
    for bad in ("", "+", "-", " 1", "1 ", "1_0", "0x1", "1.0", "2147483648", "-2147483649", "١", "１", "1\n"):
        with pytest.raises(Exception) as exc:
            rear.parse_int(bad)
        assert not isinstance(exc.value, (ValueError, TypeError)), bad          # the parser's own NumberFormatException, not int()'s
