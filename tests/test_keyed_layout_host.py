"""CPU suite: the line layout of the native interface under a public key of width kappa (csrc/hexlines_layout.h,
make_layout(curve, value_bytes, keywidth, width)) as host code under AddressSanitizer and UBSan, through a stand-alone program
(tests/keyed_layout_harness.cpp), against the restatement of the nesting rule in tests/keyed_layout_ref.py; and that
restatement against itself and against the unkeyed catalogue (tests/hexlines_cases.py) where the two must give the same bytes."""
import os
import subprocess

import pytest

from conftest import ROOT

import hexlines_cases as hc
import keyed_layout_ref as KL

CASES = [(curve, vb, kw, w) for curve, vb in ((False, 64), (False, 65), (True, 32), (True, 33)) for kw in (1, 2, 3) for w in (1, 2, 3)]
IDS = ["%s-%d-k%d-w%d" % ("curve" if c else "modp", vb, kw, w) for c, vb, kw, w in CASES]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("keyedlayout") / "keyed_layout_harness")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "keyed_layout_harness.cpp")], check=True)
    return exe


def layout(exe, curve, vb, kw, w):
    r = subprocess.run([exe, "curve" if curve else "modp", str(vb), str(kw), str(w)], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[-2000:])
    items = dict(line.split(" ", 1) for line in r.stdout.strip().split("\n"))
    return (int(items["B"]), int(items["E"]), bytes.fromhex(items["template"]), bytes.fromhex(items["mask"]),
            [int(v) for v in items["offsets"].split()])


def values(curve, vb, byte, count):
    v = int.from_bytes(bytes([byte]) * vb, "big")
    return [(v, v) if curve else v] * count


@pytest.mark.parametrize("curve,vb,kw,w", CASES, ids=IDS)
def test_layout_is_the_nested_byte_tree(harness, curve, vb, kw, w):
    B, E, tmpl, mask, offsets = layout(harness, curve, vb, kw, w)
    assert B == KL.line_bytes(curve, vb, kw, w) and E == KL.element_bytes(curve, vb)
    tree = lambda byte: KL.ciphertext_tree(curve, vb, kw, values(curve, vb, byte, 2 * kw * w))
    assert tmpl == tree(0) and len(tmpl) == B
    framing = [a == b for a, b in zip(tree(0), tree(0xfe))]                  # the bytes no value reaches
    assert [m != 0 for m in mask] == framing
    assert offsets == KL.component_offsets(curve, vb, kw, w) and len(offsets) == 2 * kw * w
    # an element tree begins at every offset; mask classes as before: 1 the nodes above the element trees, 2 inside them
    zero = values(curve, vb, 0, 1)[0]
    inside = [False] * B
    for off in offsets:
        assert tmpl[off:off + E] == KL.element_tree(curve, vb, zero)
        inside[off:off + E] = [True] * E
    assert set(mask) <= {0, 1, 2}
    for k in range(B):
        assert mask[k] == (0 if not framing[k] else 2 if inside[k] else 1), k
    assert sum(1 for m in mask if m == 1) == 5 + 2 * ((5 if w > 1 else 0) + w * (5 if kw > 1 else 0))


def test_the_size_at_key_width_two_and_width_three(harness):
    """B = 5 + 10 + 2 (3 * 5 + 6 E), from the rule: node(u, v); per half node(3; ...), three times node(2; ...), six element trees."""
    for curve, vb in ((False, 64), (True, 33)):
        E = 15 + 2 * vb if curve else 5 + vb
        want = 5 + 2 * 5 + 2 * (3 * 5 + 6 * E)
        B, _, _, _, offsets = layout(harness, curve, vb, 2, 3)
        assert B == want == KL.line_bytes(curve, vb, 2, 3)
        # flat order c = l kappa + j: after node(u, v), node(3) and the first node(2) the components follow in pairs, 5 bytes apart
        first = 5 + 5 + 5
        u = [first + l * (5 + 2 * E) + j * E for l in range(3) for j in range(2)]
        assert offsets[:6] == u and offsets[6:] == [o + 5 + 3 * (5 + 2 * E) for o in u]


@pytest.mark.parametrize("curve,vb", [(False, 64), (False, 65), (True, 33)])
@pytest.mark.parametrize("kw", [1, 2, 3, 5])
def test_width_one_under_a_key_is_the_unkeyed_layout_of_that_width(harness, curve, vb, kw):
    assert layout(harness, curve, vb, kw, 1) == layout(harness, curve, vb, 1, kw)
    # ... which is the layout the existing interface has at that width
    B, E, tmpl, _, offsets = layout(harness, curve, vb, 1, kw)
    assert B == hc.line_bytes(curve, vb, kw) and offsets == hc.component_offsets(curve, vb, kw)
    assert tmpl == hc.eio.encode(hc.ciphertext_tree(curve, kw, [(bytes(vb), bytes(vb)) if curve else bytes(vb)] * (2 * kw)))


def test_usage_errors(harness):
    for args in ([], ["ring", "32", "1", "1"], ["modp", "0", "1", "1"], ["modp", "32", "0", "1"], ["modp", "32", "1", "0"], ["modp", "32", "1"]):
        assert subprocess.run([harness] + args, capture_output=True).returncode == 2


# ---- the restatement against itself and against the unkeyed catalogue --------------------------------------------------------------
def test_restated_trees_without_a_key_are_the_unkeyed_trees():
    curve, vb, w, n = False, 8, 3, 4
    rows = hc.synthetic_rows(curve, vb, w, n)
    comps = [[int.from_bytes(r[c], "big") for r in rows] for c in range(2 * w)]
    assert KL.native_text(curve, vb, 1, comps) == hc.text_of(curve, w, rows)
    assert KL.native_text(curve, vb, w, comps) == hc.text_of(curve, w, rows)          # omega = 1 under a key of width w
    assert KL.list_tree(curve, vb, 1, comps) == KL.list_tree(curve, vb, w, comps)
    assert KL.read_list(curve, 1, w, KL.list_tree(curve, vb, 1, comps)) == comps


def test_restated_trees_at_two_by_three():
    curve, vb, xb, kw, w, n = True, 5, 4, 2, 3, 3
    comps = [[(c * 16 + i + 1, c + 2 * i + 7) if (c, i) != (4, 1) else None for i in range(n)] for c in range(2 * kw * w)]
    buf = KL.list_tree(curve, vb, kw, comps)
    E = KL.element_bytes(curve, vb)
    assert len(buf) == 5 + 2 * (5 + w * (5 + kw * (5 + n * E)))
    assert KL.read_list(curve, kw, w, buf) == comps
    tree, _ = KL.decode(buf)
    assert [len(tree), len(tree[0]), len(tree[0][0]), len(tree[0][0][0])] == [2, w, kw, n]
    wide = KL.wide_array_tree(curve, vb, kw, comps[:kw * w])
    assert KL.read_wide_array(curve, kw, w, wide) == comps[:kw * w] and wide == buf[5:5 + len(wide)]
    # one line of the native text is the ciphertext's tree; its size is the layout's
    text = KL.native_text(curve, vb, kw, comps)
    assert len(text) == n * (2 * KL.line_bytes(curve, vb, kw, w) + 1)
    # ring elements: (Z_q^2)^3 is node(3; node(2 leaves)), Z_q^2 node(2 leaves), one value a leaf
    assert KL.decode(KL.ring_tree(xb, kw, list(range(6))))[0] == [[(2 * l + j).to_bytes(xb, "big") for j in range(2)] for l in range(3)]
    assert KL.reply_tree(xb, 2, (7, 9)) == KL.node([KL.leaf((7).to_bytes(xb, "big")), KL.leaf((9).to_bytes(xb, "big"))])
    assert KL.reply_tree(xb, 1, (7,)) == KL.leaf((7).to_bytes(xb, "big"))
    # the key, the polynomial, a commitment
    g, y = (1, 2), ((3, 4), (5, 6))
    pk, _ = KL.decode(KL.public_key_tree(curve, vb, kw, g, y))
    assert [[KL.element_of(curve, e) for e in half] for half in pk] == [[g, g], list(y)]
    coeffs = [((1, 1), (2, 2)), ((3, 3), (4, 4))]
    poly, _ = KL.decode(KL.polynomial_tree(curve, vb, kw, coeffs))
    assert [[KL.element_of(curve, e) for e in arr] for arr in poly] == [[(1, 1), (3, 3)], [(2, 2), (4, 4)]]
    com, _ = KL.decode(KL.commitment_tree(curve, vb, kw, y, [(c, c) for c in range(1, 7)]))
    assert len(com) == 2 and len(com[0]) == 2 and [len(com[1])] + [len(c) for c in com[1]] == [3, 2, 2, 2]
