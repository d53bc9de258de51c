"""CPU suite: the rule of a prover's secret permutation (csrc/permutation_layout.h) as host code under AddressSanitizer and UBSan,
through a stand-alone program (tests/permutation_layout_harness.cpp): the key width at its edges, and -- over key files of the
catalogue of tests/permutation_cases.py -- the header's reference order and a digit-by-digit counting sort that reads the keys
through the header's plane / digit extraction as the kernels do, both against the restatement."""
import os
import subprocess

import pytest

from conftest import ROOT

import permutation_cases as pc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("permutation") / "permutation_layout_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "permutation_layout_harness.cpp")], check=True)
    return exe


def order(exe, tmp_path, rows):
    path = str(tmp_path / "keys")
    with open(path, "w") as f:
        f.write("".join(bytes(r).hex() + "\n" for r in rows))
    r = subprocess.run([exe, "order", str(rows.shape[1]), path], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout[-300:], r.stderr[-3000:])
    pairs = [tuple(int(v) for v in line.split()) for line in r.stdout.split("\n")[:-1]]
    assert len(pairs) == len(rows)
    return [p[0] for p in pairs], [p[1] for p in pairs]


def test_the_key_width(harness):
    for n in (0, 1, 2, 3, 4, 5, 1 << 16, (1 << 16) + 1, (1 << 32) - 1):
        for rbitlen in (0, 100, 256):
            r = subprocess.run([harness, "width", str(n), str(rbitlen)], capture_output=True, text=True)
            kb = pc.key_bits(n, rbitlen)
            assert r.returncode == 0 and r.stdout.split() == [str(kb), str(pc.key_bytes(n, rbitlen)), str((1 << (kb % 8 or 8)) - 1)], (n, rbitlen)
    for n, rbitlen in ((1 << 32, 100), (5, -1), (5, 257)):            # out of range: no width
        r = subprocess.run([harness, "width", str(n), str(rbitlen)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.split() == ["0", "0", "0"], (n, rbitlen)


@pytest.mark.parametrize("n,rbitlen,seedlen", [(0, 100, 32), (1, 100, 32), (2, 0, 32), (65, 0, 32), (257, 100, 48), (4097, 100, 32), (1025, 256, 64)])
def test_the_order_of_prg_keys(harness, tmp_path, n, rbitlen, seedlen):
    seed, h = pc.seed_of(b"host/%d" % n, seedlen), pc.HASH_OF_SEEDLEN[seedlen]
    pi, inv = order(harness, tmp_path, pc.key_rows(seed, n, rbitlen, h))
    assert pi == pc.restate(seed, n, rbitlen, h)
    assert [inv[j] for j in pi] == list(range(n))


@pytest.mark.parametrize("name,make", [(name, make) for name, make, _ in pc.CRAFTED])
def test_the_order_of_crafted_keys(harness, tmp_path, name, make):
    for vb in (1, 5, 64):
        rows = make(700, vb)
        pi, inv = order(harness, tmp_path, rows)
        want_pi, want_inv = pc.lexsort_rows(rows)
        assert pi == want_pi.tolist() and inv == want_inv.tolist(), (name, vb)
