"""CPU suite: the one reader of the proof directory's byte trees (verificatum-vmn_amd/fiatshamir.py: Cursor) and the readers
written on it (verificatum-vmn_amd/proofdir.py: the nests of element trees of a decryption commitment and of the public key, the
decryption reply, the boolean lists, the nests of arrays of every list file; verificatum-vmn_amd/interface.py: read_plaintexts),
over the stand-in groups of tests/test_keyed_trees.py, a modular group and a curve, against the trees tests/keyed_layout_ref.py
builds.  For every shape: the full tree parses to the values it was built from; every proper prefix, the tree with one byte behind
it and the tree read at a neighbouring shape are "no such tree", and none of them raises."""
import pytest

import keyed_layout_ref as KL
from test_keyed_trees import GROUPS, SHAPES, WireGroup, elements

N = 3                                                   # elements per array


class Array:
    """What the readers ask of a device array; remembers the bytes it was imported from."""

    def __init__(self, bt, n, member=True):
        self.bt, self.n, self.member, self.freed = bytes(bt), n, member, False

    def size(self):
        return self.n

    def isMember(self):
        return self.member

    def free(self):
        self.freed = True


class ArrayGroup(WireGroup):
    """WireGroup with the array side: the size of an array's tree and an import that accepts exactly such a tree."""

    def __init__(self, G):
        super().__init__(G.curve, G.nbytes, G.exp_bytes)
        self.elem_bytes, self.made = (2 if G.curve else 1) * G.nbytes, []

    def array_tree_size(self, n):
        return 5 + n * KL.element_bytes(self.curve, self.nbytes)

    def toElementArrayFromByteTree(self, bt, size=0):
        bt = bytes(bt)
        n = int.from_bytes(bt[1:5], "big")
        if bt[:1] != b"\0" or (size and n != size) or len(bt) != self.array_tree_size(n):
            raise ValueError("no array tree")
        pos = 5
        for _ in range(n):
            got = self.element_from_tree(bt, pos)
            if got is None:
                raise ValueError("no element tree")
            pos = got[1]
        self.made.append(Array(bt, n))
        return self.made[-1]


@pytest.fixture(scope="module")
def mods(entry):
    import mirror
    return mirror.load(entry, ("proofdir", "fiatshamir", "interface"))


def neighbours(kw, w):
    return [(kw + 1, w), (kw, w + 1)] + ([(1, 1)] if (kw, w) != (1, 1) else [])


def broken(tree):
    """Every proper prefix, and the tree with one byte behind it."""
    return [tree[:cut] for cut in range(len(tree))] + [tree + b"\0"]


cases = pytest.mark.parametrize("G", GROUPS, ids=["modp", "curve"])
shapes = pytest.mark.parametrize("kw,w", SHAPES)


@cases
@shapes
def test_a_nest_of_element_trees(mods, G, kw, w, tmp_path):
    """node(y', B') of a decryption commitment, and node(g', y) of the public key (both halves of width 1)."""
    pd = mods["proofdir"]
    yp, Bp, key = elements(G, kw, 40), elements(G, kw * w, 60), elements(G, 2 * kw, 80)
    tree = KL.commitment_tree(G.curve, G.nbytes, kw, yp, Bp)
    assert pd._read_element_nests(G, tree, (1, w), kw) == [yp, Bp]
    key_tree = KL.ciphertext_tree(G.curve, G.nbytes, kw, key)
    assert pd._read_element_nests(G, key_tree, (1, 1), kw) == [key[:kw], key[kw:]]
    path = str(tmp_path / "key.bt")
    with open(path, "wb") as f:
        f.write(key_tree)
    one = lambda rows: rows[0] if kw == 1 else tuple(rows)
    ctx = type("ctx", (), {"grp": G, "keywidth": kw})
    assert pd.GPU_ENGINES.read_pkey(ctx, path) == [one(key[:kw]), one(key[kw:])]
    assert pd.GPU_ENGINES.read_pkey(ctx, path + ".missing") is None and pd._read_element_nests(G, None, (1, w), kw) is None
    for bad in broken(tree):
        assert pd._read_element_nests(G, bad, (1, w), kw) is None
    for kw2, w2 in neighbours(kw, w):
        assert pd._read_element_nests(G, tree, (1, w2), kw2) is None


@cases
@shapes
def test_a_reply(mods, G, kw, w):
    pd = mods["proofdir"]
    kx = [(1 << (8 * G.exp_bytes)) - 1 - j for j in range(kw)]                       # rows far above any q: handed on
    tree = KL.reply_tree(G.exp_bytes, kw, kx)
    assert pd._read_reply(G, tree, kw) == (kx[0] if kw == 1 else tuple(kx))
    for bad in broken(tree):
        assert pd._read_reply(G, bad, kw) is None
    for kw2 in {kw + 1, max(1, kw - 1), 1} - {kw}:
        assert pd._read_reply(G, tree, kw2) is None


@shapes
def test_a_boolean_list(mods, kw, w):
    pd = mods["proofdir"]
    flags = [(i * 5) % 3 == 0 for i in range(kw * w + 2)]
    tree = pd._booleans_tree(flags)
    assert tree == KL.leaf(bytes(flags)) and pd._parse_booleans(tree, len(flags)) == flags
    for bad in broken(tree) + [tree[:-1] + b"\2", b"\0" + tree[1:]]:                  # also: a byte that is no flag, a node's tag
        assert pd._parse_booleans(bad, len(flags)) is None
    assert pd._parse_booleans(tree, len(flags) + 1) is None and pd._parse_booleans(tree, len(flags) - 1) is None
    assert pd._parse_booleans(None, len(flags)) is None


def arrays_of(G, count):
    return [elements(G, N, 10 * c) for c in range(count)]


@cases
@shapes
def test_a_nest_of_arrays_cut_by_an_item_reader_that_knows_only_the_size(mods, G, kw, w):
    fs = mods["fiatshamir"]
    A = ArrayGroup(G)
    trees = [KL.array_tree(G.curve, G.nbytes, a) for a in arrays_of(G, kw * w)]
    tree = KL.nest(trees, kw)
    item = lambda c: c.take(A.array_tree_size(c.children()))

    def read(buf, w_, kw_):
        try:
            cur = fs.Cursor(buf)
            got = cur.nested(w_, kw_, item)
            cur.end()
            return got
        except fs.NoSuchTree:
            return None
    assert read(tree, w, kw) == trees
    for bad in broken(tree):
        assert read(bad, w, kw) is None
    for kw2, w2 in neighbours(kw, w):
        assert read(tree, w2, kw2) is None


@cases
@shapes
def test_the_readers_of_array_files(mods, G, kw, w, tmp_path):
    """read_array_nests under its three callers' shapes: a list file (two nests, n from the first header or given), a file of
    factors or plaintexts (one nest, membership checked), the polynomial in the exponent."""
    pd = mods["proofdir"]
    A = ArrayGroup(G)
    comps = arrays_of(G, 2 * kw * w)
    trees = [KL.array_tree(G.curve, G.nbytes, a) for a in comps]
    tree = KL.list_tree(G.curve, G.nbytes, kw, comps)
    for n in (0, N):
        assert [a.bt for a in pd.parse_ciphertexts(A, tree, w, n, kw)] == trees
    assert pd.parse_ciphertexts(A, tree, w, N + 1, kw) is None
    for bad in broken(tree):
        A.made.clear()
        assert pd.parse_ciphertexts(A, bad, w, 0, kw) is None and all(a.freed for a in A.made)
    for kw2, w2 in neighbours(kw, w):
        assert pd.parse_ciphertexts(A, tree, w2, 0, kw2) is None
    # arrays of different sizes are no list
    short = KL.list_tree(G.curve, G.nbytes, kw, comps[:-1] + [comps[-1][:-1]])
    assert pd.parse_ciphertexts(A, short, w, 0, kw) is None
    # one nest: the factors of a party, the plaintexts
    wide = KL.wide_array_tree(G.curve, G.nbytes, kw, comps[:kw * w])
    path = str(tmp_path / "wide.bt")
    for data, want in [(wide, trees[:kw * w])] + [(bad, None) for bad in broken(wide)]:
        with open(path, "wb") as f:
            f.write(data)
        got = pd._read_wide_array(A, path, w, N, kw)
        assert (got if got is None else [a.bt for a in got]) == want
    assert pd._read_wide_array(A, path + ".missing", w, N, kw) is None


def test_read_plaintexts_splits_a_curve_file_by_the_arrays_own_sizes(mods, tmp_path):
    """A raw plaintext file of two arrays of three points: each array is 5 + 3 * (15 + 2 cw) bytes, not the 5 + 3 * (5 + 2 cw)
    of a modular group's leaves of 2 cw bytes, which read_plaintexts once took it to be and so refused the file."""
    interface = mods["interface"]
    A = ArrayGroup(GROUPS[1])
    assert A.curve and A.array_tree_size(N) == 5 + N * (15 + 2 * A.nbytes) != 5 + N * (5 + A.elem_bytes)
    comps = arrays_of(A, 2)
    trees = [KL.array_tree(True, A.nbytes, a) for a in comps]
    path = str(tmp_path / "Plaintexts.bt")
    with open(path, "wb") as f:
        f.write(KL.wide_array_tree(True, A.nbytes, 1, comps))
    got = interface.read_plaintexts(A, path, 2)
    assert got is not None and [a.bt for a in got] == trees and [a.size() for a in got] == [N, N]
    # one array at width 1, and the keyed nest
    with open(path, "wb") as f:
        f.write(trees[0])
    assert [a.bt for a in interface.read_plaintexts(A, path, 1)] == trees[:1]
    with open(path, "wb") as f:
        f.write(KL.wide_array_tree(True, A.nbytes, 2, comps))
    assert [a.bt for a in interface.read_plaintexts(A, path, 1, keywidth=2)] == trees
    assert interface.read_plaintexts(A, path, 2, keywidth=2) is None and interface.read_plaintexts(A, path + ".missing", 2) is None
