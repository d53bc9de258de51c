"""CPU suite: the host-side trees of a session under a public key of width kappa (verificatum-vmn_amd/fiatshamir.py:
nested_tree, product_element_tree, wide_element_tree; verificatum-vmn_amd/proofdir.py: the commitment and reply of the decryption,
their readers, the session's control flow with a key of kappa rows) against tests/keyed_layout_ref.py.  No GPU: a stand-in group
that knows its wire widths is all these functions ask of a group."""
import pytest

import keyed_layout_ref as KL
import session_cases as S


class WireGroup:
    """The wire side of a group: leaves of vb bytes, or points of two such coordinates."""

    def __init__(self, curve, vb, xb):
        self.curve, self.nbytes, self.exp_bytes, self.coord_bytes = curve, vb, xb, vb if curve else None

    def enc_el(self, el):
        if not self.curve:
            return int(el).to_bytes(self.nbytes, "big")
        if el is None:
            return b"\xff" * (2 * self.nbytes)
        return int(el[0]).to_bytes(self.nbytes, "big") + int(el[1]).to_bytes(self.nbytes, "big")

    def element_tree(self, el):
        return KL.element_tree(self.curve, self.nbytes, el)

    def element_from_tree(self, buf, pos=0):
        try:
            tree, end = KL.decode(buf, pos)
            if self.curve:
                ok = isinstance(tree, list) and len(tree) == 2 and all(isinstance(t, bytes) and len(t) == self.nbytes for t in tree)
            else:
                ok = isinstance(tree, bytes) and len(tree) == self.nbytes
            return (KL.element_of(self.curve, tree), end) if ok and end <= len(buf) else None
        except IndexError:
            return None


@pytest.fixture(scope="module")
def mods(entry):
    import mirror
    return mirror.load(entry, ("proofdir", "fiatshamir"))


GROUPS = [WireGroup(False, 8, 4), WireGroup(True, 5, 4)]
SHAPES = [(1, 1), (1, 3), (2, 1), (2, 3), (3, 2)]


def elements(G, count, salt=0):
    return [(c + salt + 1, 2 * c + salt + 3) if G.curve else 7 * c + salt + 1 for c in range(count)]


@pytest.mark.parametrize("G", GROUPS, ids=["modp", "curve"])
@pytest.mark.parametrize("kw,w", SHAPES)
def test_the_trees_of_fiatshamir_are_the_restated_trees(mods, G, kw, w):
    fs = mods["fiatshamir"]
    els = elements(G, 2 * kw * w)
    assert fs.product_element_tree(G, els, kw) == KL.ciphertext_tree(G.curve, G.nbytes, kw, els)
    assert fs.wide_element_tree(G, els[:kw * w], kw) == KL.nest([KL.element_tree(G.curve, G.nbytes, e) for e in els[:kw * w]], kw)
    trees = [bytes([c]) * 3 for c in range(kw * w)]
    assert fs.nested_tree(trees, kw) == KL.nest(trees, kw)
    # width 1 under a key is the unkeyed form of that width; key width 1 is the form the functions had
    assert fs.product_element_tree(G, els[:2 * kw], kw) == fs.product_element_tree(G, els[:2 * kw])
    assert fs.nested_tree(trees, 1) == (trees[0] if len(trees) == 1 else fs._hdr(0, len(trees)) + b"".join(trees))
    with pytest.raises(ValueError):
        fs.nested_tree(trees + [b"x"], kw + 1 if (len(trees) + 1) % (kw + 1) else kw + 2)


@pytest.mark.parametrize("G", GROUPS, ids=["modp", "curve"])
@pytest.mark.parametrize("kw,w", SHAPES)
def test_the_decryption_commitment_and_reply(mods, G, kw, w, tmp_path):
    pd = mods["proofdir"]
    yp, Bp = elements(G, kw, 40), elements(G, kw * w, 60)
    kx = [1000 + j for j in range(kw)]
    one = lambda rows: rows[0] if kw == 1 else tuple(rows)
    tree = pd._commitment_tree(G, one(yp), tuple(Bp), kw)
    assert tree == KL.commitment_tree(G.curve, G.nbytes, kw, yp, Bp)
    path = str(tmp_path / "c.bt")
    with open(path, "wb") as f:
        f.write(tree)
    assert pd._read_commitment(G, path, w, kw) == (one(yp), tuple(Bp))
    reply = pd._reply_tree(G, one(kx), kw)
    assert reply == KL.reply_tree(G.exp_bytes, kw, kx) and pd._read_reply(G, reply, kw) == one(kx)
    # read at another shape, truncated, or with a byte behind the end: no such file
    if (kw, w) != (1, 1):
        assert pd._read_commitment(G, path, 1, 1) is None
    assert pd._read_reply(G, reply, kw + 1) is None and pd._read_reply(G, reply + b"\0", kw) is None and pd._read_reply(G, reply[:-1], kw) is None
    for bad in (tree[:-1], tree + b"\0"):
        with open(path, "wb") as f:
            f.write(bad)
        assert pd._read_commitment(G, path, w, kw) is None


def test_the_session_flow_with_a_key_of_two_rows(mods, tmp_path):
    """run_session with keywidth 2 over the stub engines: the key's first half must be (g, g), the second the polynomial's
    element 0, the wide key repeats the rows with period 2, and bas.pk / bas.y_l show the rows."""
    pd = mods["proofdir"]
    nizkp = str(tmp_path / "nizkp")
    S.tiny_session(pd, nizkp)
    G = S.TinyGroup()
    seen = {}

    def engines(pk, poly):
        stub = S.StubEngines(pd)
        eng = stub.engines
        eng.read_pkey = lambda ctx, path: (seen.update(keywidth=ctx.keywidth), pk)[1]
        eng.read_poly = lambda ctx, path, thr: poly
        verify_pos = eng.verify_pos

        def spy(ctx, *a):
            seen["pkey"] = list(ctx.pkey)
            return verify_pos(ctx, *a)
        eng.verify_pos = spy
        return eng
    poly = [(13, 3), (5, 9)]
    tv = {}
    v = pd.run_session(nizkp, G, S.tiny_params(), pd.SessionParams(), engines([(2, 2), (13, 3)], poly), tv, keywidth=2)
    assert v.accepted and seen["keywidth"] == 2 and seen["pkey"] == [2, 2, 13, 3]         # (the stub session has width 1)
    assert tv["bas.pk"] == "((2, 2), (d, 3))"
    y = lambda l: (13 * pow(5, l, 23) % 23, 3 * pow(9, l, 23) % 23)
    assert tv["bas.y_l"] == "(" + ",".join("(%x, %x)" % y(l) for l in (1, 2)) + ")"
    # params.json's entry is read when no key width is given
    tv2 = {}
    pd.run_session(nizkp, G, S.tiny_params(keywidth=2), pd.SessionParams(), engines([(2, 2), (13, 3)], poly), tv2)
    assert tv2["bas.pk"] == tv["bas.pk"]
    for pk, message in (([(2, 4), (13, 3)], "Basic public key is not the standard generator!"),
                        ([(4, 2), (13, 3)], "Basic public key is not the standard generator!"),
                        ([(2, 2), (13, 4)], "Mismatching public keys!")):
        with pytest.raises(pd.SessionFormatError, match=message):
            pd.run_session(nizkp, G, S.tiny_params(), pd.SessionParams(), engines(pk, poly), keywidth=2)
    with pytest.raises(pd.SessionFormatError, match="Key width is not positive!"):
        pd.run_session(nizkp, G, S.tiny_params(), pd.SessionParams(), engines([(2, 2), (13, 3)], poly), keywidth=0)
