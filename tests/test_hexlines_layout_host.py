"""CPU suite: the line layout of the native ciphertext interface (csrc/hexlines_layout.h) as host code under AddressSanitizer
and UBSan, through a stand-alone program (tests/hexlines_layout_harness.cpp) that prints the template, the mask and the
component offsets of a (group kind, leaf width, ciphertext width).  They are compared with the byte trees tests/hexlines_cases.py
builds with eio.encode: the template is the tree of all-zero values, the mask marks exactly the bytes that do not change when
every value byte is set (1: the outer nodes, 2: inside an element tree), an element tree begins at every offset."""
import os
import subprocess

import pytest

from conftest import ROOT

import hexlines_cases as hc

CASES = [(False, vb, w) for vb in (64, 65, 256, 257, 384) for w in (1, 2, 3)] + [(True, vb, w) for vb in (32, 33, 66) for w in (1, 2, 3)]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hexlines") / "hexlines_layout_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "hexlines_layout_harness.cpp")], check=True)
    return exe


def layout(exe, curve, vb, w):
    r = subprocess.run([exe, "curve" if curve else "modp", str(vb), str(w)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    items = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    return (int(items["B"]), int(items["E"]), bytes.fromhex(items["template"]), bytes.fromhex(items["mask"]),
            [int(v) for v in items["offsets"].split()])


@pytest.mark.parametrize("curve,vb,w", CASES, ids=["%s-%d-w%d" % ("curve" if c else "modp", vb, w) for c, vb, w in CASES])
def test_layout_is_the_byte_tree(harness, curve, vb, w):
    B, E, tmpl, mask, offsets = layout(harness, curve, vb, w)
    assert B == hc.line_bytes(curve, vb, w) and E == hc.element_bytes(curve, vb)
    zero, ones = bytes(vb), b"\xff" * vb
    tree = lambda v: hc.eio.encode(hc.ciphertext_tree(curve, w, [(v, v) if curve else v] * (2 * w)))
    assert tmpl == tree(zero) and len(tmpl) == B
    framing = [a == b for a, b in zip(tree(zero), tree(ones))]              # the bytes no value reaches
    assert [m != 0 for m in mask] == framing
    assert offsets == hc.component_offsets(curve, vb, w)
    inside = [False] * B
    for off in offsets:
        sub, end = hc.eio.decode(tmpl, off)
        assert sub == hc.element_tree(curve, (zero, zero) if curve else zero) and end == off + E
        inside[off:end] = [True] * E
    assert set(mask) <= {0, 1, 2}
    for k in range(B):
        assert mask[k] == (0 if not framing[k] else 2 if inside[k] else 1), k
    assert sum(1 for m in mask if m == 1) == 5 + (10 if w > 1 else 0)


def test_the_sizes_the_interface_documents(harness):
    assert layout(harness, False, 256, 1)[0] == 527
    assert layout(harness, True, 33, 3)[0] == 501


def test_usage_errors(harness):
    for args in ([], ["ring", "32", "1"], ["modp", "0", "1"], ["modp", "32", "0"]):
        assert subprocess.run([harness] + args, capture_output=True).returncode == 2
