"""CPU suite: the host's schedule builder of the curve powers under one scalar (csrc/ec_shared_schedule.h) as host code under
AddressSanitizer and UBSan, through a stand-alone program (tests/ec_shared_schedule_harness.cpp).  For every scalar of the
catalogue (tests/ec_shared_cases.py), every forced window 2 ... 6 and the chosen one, the program checks the digits of the
recoding (odd, below 2^(w-1) in magnitude, at most one among w consecutive positions, a positive top digit, at most one
position longer than the scalar), walks the schedule over plain integers and compares with the scalar modulo the order, checks
that the doublings do not exceed its bits, that the first step loads a row, that only a scalar = 0 modulo the order has an
empty schedule, and that schedules appended to ONE buffer are found at their first / count.  Here: the reduction against
Python's, the extreme digits, and the chosen window as a minimiser of the stated cost."""
import os
import subprocess

import pytest

from conftest import ROOT

import ec_shared_cases as X
from oracle.pyref_ec import Curve

ORDERS = {"P-256": Curve("P-256").n, "P-521": Curve("P-521").n}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ec_shared") / "ec_shared_schedule_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "ec_shared_schedule_harness.cpp")], check=True)
    return exe


def run(exe, w, q, scalars):
    """(window, [(e mod q, steps, adds, dbls, min digit, max digit)])"""
    r = subprocess.run([exe, str(w), "%x" % q] + ["%x" % e for e in scalars], capture_output=True, text=True)
    lines = r.stdout.split("\n")
    assert r.returncode == 0 and lines[0].startswith("ok "), (w, scalars, r.returncode, r.stdout[-500:], r.stderr[-2000:])
    rows = [line.split() for line in lines[1:] if line]
    assert len(rows) == len(scalars)
    return int(lines[0].split()[1]), [(int(v[0], 16),) + tuple(int(t) for t in v[1:]) for v in rows]


@pytest.fixture(scope="module")
def forced(harness):
    """{(curve, w): rows of the whole catalogue in ONE buffer under the forced window w}"""
    return {(name, w): run(harness, w, q, [e for _, e in X.catalogue(q)])[1] for name, q in ORDERS.items() for w in X.WINDOWS}


@pytest.mark.parametrize("name", sorted(ORDERS))
def test_every_scalar_of_the_catalogue_under_every_forced_window(name, forced):
    q = ORDERS[name]
    cat = X.catalogue(q)
    for w in X.WINDOWS:
        rows = forced[(name, w)]
        for (label, e), (red, steps, adds, dbls, dmin, dmax) in zip(cat, rows):
            r = e % q
            assert red == r, (label, w)
            assert (steps == 0) == (r == 0), (label, w)
            assert dbls <= r.bit_length(), (label, w)
            if r:
                assert steps - 2 <= adds <= steps - 1, (label, w)        # (a last step of trailing zeros adds nothing)
                assert adds <= r.bit_length() // w + 1, (label, w)


@pytest.mark.parametrize("name", sorted(ORDERS))
def test_the_extreme_digits_are_reached(name, forced):
    q = ORDERS[name]
    labels = [label for label, _ in X.catalogue(q)]
    for w in X.WINDOWS:
        D = (1 << (w - 1)) - 1
        red, steps, adds, dbls, dmin, dmax = forced[(name, w)][labels.index("extreme%d" % w)]
        assert (dmin, dmax) == (-D, D) and (steps, adds, dbls) == (2, 1, 2 * w + 3), w
        # 2^200 - 1 is the digits -1 and +1 under every window: the carry runs through 199 ones
        red, steps, adds, dbls, dmin, dmax = forced[(name, w)][labels.index("2^200-1")]
        assert (dmin, dmax, steps, adds, dbls) == (-1, 1, 2, 1, 200), w


@pytest.mark.parametrize("name", sorted(ORDERS))
def test_the_chosen_window_minimises_the_stated_cost(name, harness, forced):
    q = ORDERS[name]
    cat = X.catalogue(q)
    for i, (label, e) in enumerate(cat):
        chosen, rows = run(harness, 0, q, [e])
        costs = {}
        for w in X.WINDOWS:
            red, steps, adds, dbls, dmin, dmax = forced[(name, w)][i]
            costs[w] = X.cost(w, adds, dbls) if steps else 0.0
        assert costs[chosen] == min(costs.values()), (label, chosen, costs)
        assert rows[0][:4] == forced[(name, chosen)][i][:4], label             # alone in its buffer as among the others


def test_one_window_for_several_scalars_by_the_sum(harness, forced):
    """A call with several scalars: ONE window, the cheapest by the sum over their recodings; a zero scalar adds nothing."""
    q = ORDERS["P-256"]
    cat = X.catalogue(q)
    labels = [label for label, _ in cat]
    for group in (["full0", "2^200", "q-1"], ["0", "full1", "1"], ["3", "2^5-1", "extreme6"], ["full0", "full1", "full2", "full3"]):
        idx = [labels.index(g) for g in group]
        chosen, rows = run(harness, 0, q, [cat[i][1] for i in idx])
        sums = {}
        for w in X.WINDOWS:
            sums[w] = sum(X.cost(w, forced[("P-256", w)][i][2], forced[("P-256", w)][i][3]) for i in idx if forced[("P-256", w)][i][1])
        assert sums[chosen] == min(sums.values()), (group, chosen, sums)
        for i, row in zip(idx, rows):
            assert row[:4] == forced[("P-256", chosen)][i][:4], (group, labels[i])
    chosen, rows = run(harness, 0, q, [0, q, 2 * q])                         # every scalar = 0 modulo the order: nothing to walk
    assert [row[:4] for row in rows] == [(0, 0, 0, 0)] * 3


def test_the_op_count_of_a_full_length_scalar(forced):
    """The figures of DESIGN.md §5 for a 256-bit scalar under w = 5: about 43 additions behind the first step on at most 256
    doublings, about 2540 in the library's prices with the table of 8 rows (7 additions, one doubling) -- against the 256
    doublings, 52 + 32 additions = about 3060 of the fixed unsigned window."""
    cat = X.catalogue(ORDERS["P-256"])
    seen = 0
    for i, (label, e) in enumerate(cat):
        if label.startswith("full"):
            red, steps, adds, dbls = forced[("P-256", 5)][i][:4]
            assert 36 <= adds <= 50 and 250 <= dbls <= 256, (label, adds, dbls)
            assert 2400 <= X.cost(5, adds, dbls) <= 2700 < X.EC_DBL * 256 + X.EC_ADD * (52 + 32), label
            seen += 1
    assert seen == 4
