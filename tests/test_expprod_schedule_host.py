"""CPU suite: the host's schedule builder of vmn_garray_expprod_arrays (csrc/expprod_schedule.h) as host code under
AddressSanitizer and UBSan, through a stand-alone program (tests/expprod_schedule_harness.cpp) that walks every schedule over a
table of subset products modulo 2^61 - 1 and compares with the plain powers.  The exponent sets are the catalogue's
(tests/expprod_arrays_cases.py), per sign as the modular launch cuts them and all together as the curve launch takes them."""
import os
import subprocess

import pytest

from conftest import ROOT

import expprod_arrays_cases as X


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("expprod") / "expprod_schedule_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "expprod_schedule_harness.cpp")], check=True)
    return exe


def run(exe, bits, ints):
    r = subprocess.run([exe, str(bits), "4"] + ["%x" % v for v in ints], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (bits, ints, r.returncode, r.stdout, r.stderr[-2000:])
    return [int(v) for v in r.stdout.split()[1:]]


def test_every_exponent_set_of_the_catalogue(harness):
    seen = set()
    for case in X.catalogue():
        sets = [[abs(c) for c in case["ints"]], [c for c in case["ints"] if c > 0], [-c for c in case["ints"] if c < 0]]
        for ints in sets:
            key = tuple(ints)
            if not ints or key in seen:
                continue
            seen.add(key)
            bits = max(1, max(c.bit_length() for c in ints))
            steps, mults, squarings = run(harness, bits, ints)
            if any(ints):
                assert squarings == bits - 1, (case["name"], ints)          # ONE chain: the top bit opens it
            else:
                assert steps == 0
            run(harness, bits + 70, ints)                                   # bitlen well above the true length


def test_the_named_edges(harness):
    L = X.launch_limit()
    q = X.group("g14")["q"]
    assert run(harness, 8, [0, 0, 0]) == [0, 0, 0]                          # all exponents 0
    assert run(harness, 1, [1]) == [1, 0, 0]                                # a copy
    assert run(harness, 3, [5, 0, 2])[0] == 3                               # an exponent 0 among others
    assert run(harness, 64, [1 << 63, 1 << 20, 1]) == [3, 2, 63]            # one-bit exponents: the zero columns merge
    steps, mults, squarings = run(harness, q.bit_length(), [1 << (q.bit_length() - 1), 1])      # lengths differ by bits(q) - 1
    assert (steps, mults, squarings) == (2, 1, q.bit_length() - 1)
    for k in (L, L + 1):                                                    # the launch limit and one more (a third group)
        steps, mults, squarings = run(harness, 8, [0xff] * k)
        assert squarings == 7 and steps == 8 * ((k + 3) // 4)
