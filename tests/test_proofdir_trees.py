"""CPU suite: the byte trees the proof directory writes and hashes for group elements (verificatum-vmn_amd/fiatshamir.py:
group_element_tree, product_element_tree, wide_element_tree, array_tree_size), against bytes written out by hand here.

A curve point is node(leaf(x), leaf(y)) = 00 00000002 | 01 <cw:4> x | 01 <cw:4> y with cw the group's coordinate wire width
(33 for P-256 at the reference's widths), the point at infinity the same node with both leaves 0xff; an element of a modular
group is one leaf.  The helpers are pure: no context, no library, no GPU."""
import importlib.util
import os

import pytest

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("fiatshamir_under_test", os.path.join(ROOT, "verificatum-vmn_amd", "fiatshamir.py"))
fs = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fs)

GX = "6b17d1f2e12c4247f8bce6e563a440f277037d812deb33a0f4a13945d898c296"      # the generator of P-256
GY = "4fe342e2fe1a7f9b8ee7eb4a7c0f9e162bce33576b315ececbb6406837bf51f5"
# 2 * generator
DX = "7cf27b188d034f7e8a52380304b51ac3c08969e277f21b35a60b48fc47669978"
DY = "07775510db8ed040293d9ac69f7430dbba7dade63ce982299e04b79d227873d1"
NODE2, NODE3 = "0000000002", "0000000003"
LEAF33 = "0100000021"


def point_hex(x, y):
    return NODE2 + LEAF33 + "00" + x + LEAF33 + "00" + y


G_NODE, D_NODE = point_hex(GX, GY), point_hex(DX, DY)
INF_NODE = NODE2 + LEAF33 + "ff" * 33 + LEAF33 + "ff" * 33


class CurveStandIn:
    """What the helpers use of a curve group: the coordinate width and the fixed-width encoding x || y (infinity: 0xff bytes)."""

    def __init__(self, cw):
        self.coord_bytes = cw

    def enc_el(self, el):
        cw = self.coord_bytes
        return b"\xff" * (2 * cw) if el is None else el[0].to_bytes(cw, "big") + el[1].to_bytes(cw, "big")


class ModPStandIn:
    """What the helpers use of a modular group: the fixed-width encoding."""

    def __init__(self, nbytes):
        self.nbytes = nbytes

    def enc_el(self, el):
        return int(el).to_bytes(self.nbytes, "big")


G = (int(GX, 16), int(GY, 16))
D = (int(DX, 16), int(DY, 16))


def test_a_p256_point_at_the_reference_width_is_a_node_of_two_33_byte_leaves():
    enc = bytes.fromhex("00" + GX + "00" + GY)
    tree = fs.group_element_tree(enc, 33)
    assert tree == bytes.fromhex(G_NODE)
    assert len(tree) == 15 + 2 * 33
    assert CurveStandIn(33).enc_el(G) == enc


def test_the_point_at_infinity_is_the_node_of_two_ff_leaves():
    assert fs.group_element_tree(b"\xff" * 66, 33) == bytes.fromhex(INF_NODE)
    assert fs.product_element_tree(CurveStandIn(33), [None]) == bytes.fromhex(INF_NODE)


def test_an_encoding_that_is_not_two_coordinates_is_refused():
    with pytest.raises(ValueError):
        fs.group_element_tree(b"\x00" * 65, 33)


def test_an_element_of_a_modular_group_is_one_leaf():
    assert fs.group_element_tree(bytes.fromhex("0005"), None) == bytes.fromhex("0100000002" "0005")
    assert fs.group_element_tree(bytes.fromhex("0005")) == bytes.fromhex("0100000002" "0005")


def test_keys_of_width_1_and_3_over_a_curve():
    K = CurveStandIn(33)
    assert fs.product_element_tree(K, [G, D]) == bytes.fromhex(NODE2 + G_NODE + D_NODE)
    wide = fs.product_element_tree(K, [G, G, G, D, None, D])
    assert wide == bytes.fromhex(NODE2 + NODE3 + G_NODE * 3 + NODE3 + D_NODE + INF_NODE + D_NODE)
    assert fs.product_element_tree(K, [D]) == bytes.fromhex(D_NODE)


def test_a_wide_commitment_component_over_a_curve():
    K = CurveStandIn(33)
    assert fs.wide_element_tree(K, [G, D, None]) == bytes.fromhex(NODE3 + G_NODE + D_NODE + INF_NODE)
    assert fs.wide_element_tree(K, [D]) == bytes.fromhex(D_NODE)           # omega = 1: the element tree itself


@pytest.mark.parametrize("nbytes", [2, 65, 257])
def test_over_a_modular_group_the_new_helpers_write_what_element_tree_writes(nbytes):
    M = ModPStandIn(nbytes)
    for els in ([7], [7, 11], [1, 2, 3, 4], [1, 2, 3, 4, 5, 6], [2 ** (8 * nbytes) - 1] * 6):
        assert fs.product_element_tree(M, els) == fs.element_tree(M, els)
    assert fs.product_element_tree(M, [7, 11]) == b"\x00\x00\x00\x00\x02" + fs.leaf(M.enc_el(7)) + fs.leaf(M.enc_el(11))
    assert fs.wide_element_tree(M, [7]) == fs.leaf(M.enc_el(7))
    assert fs.wide_element_tree(M, [7, 11, 13]) == b"\x00\x00\x00\x00\x03" + b"".join(fs.leaf(M.enc_el(x)) for x in (7, 11, 13))
    assert fs.array_tree_size(9, nbytes) == 5 + 9 * (5 + nbytes)


@pytest.mark.parametrize("cw", [25, 29, 33, 41, 49, 65, 66])
def test_an_array_of_n_points_takes_5_plus_n_times_15_plus_2_cw_bytes(cw):
    """The coordinate widths of the named curves at the reference's widths (192 ... 521 bits: floor(bits / 8) + 1) and 65, the
    plain width of a 520-bit coordinate."""
    K = CurveStandIn(cw)
    for n in (0, 1, 7, 40):
        assert fs.array_tree_size(n, 2 * cw, cw) == 5 + n * (15 + 2 * cw)
        pts = [None if i % 3 == 2 else (i + 1, 2 * i + 5) for i in range(n)]
        tree = b"\x00" + n.to_bytes(4, "big") + b"".join(fs.group_element_tree(K.enc_el(pt), cw) for pt in pts)
        assert len(tree) == fs.array_tree_size(n, 2 * cw, cw)
        assert fs.array_tree_size(n, 2 * cw, cw) != 5 + n * (5 + 2 * cw) or n == 0      # never the modular rule
