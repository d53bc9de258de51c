"""The rows of tests/ec_wire_edges.py are not vacuous: every class of row is there for every curve and coordinate width, or
the catalogue says why it cannot be; every alias is out of range and a point of the curve once reduced; decode() is
libcrypto's verdict at the natural width; and five mutants of decode() (never of a kernel), most of which random valid points
cannot tell from it, are caught on every curve where they can be told apart at all.  No GPU: the kernels meet these rows in
tests/test_gpu_ec_wire_edges.py."""
import ctypes

import pytest

import ec_wire_edges as we
import named_curves as nc

CASES = [(name, w) for name in we.NAMES for w in we.WIDTHS]
B_IS_A_SQUARE = {"P-192", "P-256", "P-384", "P-521", "prime239v1"}


def test_curves_are_one_per_kernel_instantiation():
    """The table of the module against the library's own (csrc/vmnhip.hip kCurves) and csrc/ec_instances.h."""
    table, _ = nc.library_table()
    got = set()
    for name, kind, S in we.CURVES:
        f = we.facts(name)
        assert (f["kind"], f["S"]) == (kind, S) and f["S"] == table[name]["S"], name
        got.add((kind, S))
    built = {("NIST" if t["a"] is None else "GENERAL", t["S"]) for t in table.values()}
    assert got == built == {("NIST", 9), ("NIST", 10), ("NIST", 15), ("NIST", 21),
                            ("GENERAL", 9), ("GENERAL", 10), ("GENERAL", 13), ("GENERAL", 15), ("GENERAL", 21)}
    # the widths that leave the top packed word partly absent, and the Java widths that equal the natural ones
    assert [we.widths(n)["natural"] for n in ("P-192", "prime239v1", "P-521", "brainpoolp512r1")] == [24, 30, 66, 64]
    assert [4 * we.facts(n)["NW"] for n in ("P-192", "prime239v1", "P-521", "brainpoolp512r1")] == [28, 32, 68, 68]
    assert {n for n in we.NAMES if we.widths(n)["java"] == we.widths(n)["natural"]} == {"P-521", "prime239v1"}
    assert we.widths("P-256") == dict(natural=32, java=33, buffer=36, beyond=37)
    assert {n for n in we.NAMES if we.facts(n)["zero_x"]} == B_IS_A_SQUARE


@pytest.mark.parametrize("name,width", CASES)
def test_every_class_is_present_or_explained(name, width):
    f = we.facts(name)
    c, nb = f["c"], we.widths(name)[width]
    rows, absent = we.catalogue(name, nb)
    labels = [r.label for r in rows]
    assert len(set(labels)) == len(labels) and all(len(r.x) == nb == len(r.y) for r in rows)
    assert set(we.LABELS) <= set(labels) | set(absent) and not set(labels) & set(absent)
    assert all(reason for reason in absent.values())
    # what may be absent, and where
    above_words = nb > 4 * f["NW"]
    allowed = set()
    if name not in B_IS_A_SQUARE:
        allowed |= {"x=0+", "x=0-"}
    if not above_words:
        allowed |= {"lead-01-x", "lead-80-x", "lead-01-y", "lead-80-y"}
    if width == "natural":
        allowed |= {"alias-y"}
    assert set(absent) <= allowed, sorted(set(absent) - allowed)
    assert {"alias-x+", "alias-x-"} <= set(labels)                               # x + p fits every width of every curve
    # y + p fits the natural width on P-521, prime239v1 and the six brainpool curves; the Java width carries it elsewhere
    assert ("alias-y" in labels) == (width != "natural" or name in ("P-521", "prime239v1") or name.startswith("brainpool"))
    verdicts = dict(zip(labels, we.decoded(name, nb)))
    for r in rows:
        P, ok = verdicts[r.label]
        assert ok == (r.cls == we.VALID), r.label
        assert (P is None) == (not ok or r.label == "identity"), r.label
        if P is not None:
            assert c.on_curve(P) and r.x + r.y == P[0].to_bytes(nb, "big") + P[1].to_bytes(nb, "big")
        x, y = int.from_bytes(r.x, "big"), int.from_bytes(r.y, "big")
        if r.cls == we.ALIAS:                                                    # one group element, a second encoding
            assert (x >= c.p or y >= c.p) and (x - c.p < c.p and y - c.p < c.p)
            assert c.on_curve((x % c.p, y % c.p)) and r.x + r.y != b"\xff" * (2 * nb)
        if r.cls == we.LEAD:                                                     # a valid point below the packed words' top
            m = (1 << (32 * f["NW"])) - 1
            assert c.on_curve((x & m, y & m)) and (r.x[0] | r.y[0]) in (0x01, 0x80) and (x >> (32 * f["NW"]) or y >> (32 * f["NW"]))
    # the edge points are what they are called
    assert int.from_bytes(rows[labels.index("min-x+")].x, "big") == f["min_x"][0] <= 3
    assert all(we.lift(x, c.p, c.a, c.b) in (None, 0) for x in range(f["min_x"][0]))
    assert all(we.lift(x, c.p, c.a, c.b) in (None, 0) for x in range(f["max_x"][0] + 1, c.p))
    assert c.on_curve(f["min_x"]) and c.on_curve(f["max_x"]) and c.p - f["max_x"][0] <= 6
    for wrong in ("wrong-a", "wrong-b"):
        r = rows[labels.index(wrong)]
        x, y = int.from_bytes(r.x, "big"), int.from_bytes(r.y, "big")
        a2, b2 = ((c.p - 3 if c.a != c.p - 3 else 0), c.b) if wrong == "wrong-a" else (c.a, c.b + 1)
        assert (y * y - (x * x * x + a2 * x + b2)) % c.p == 0 and not c.on_curve((x, y))


def test_java_width_puts_aliases_under_a_leading_byte():
    """Where the aliases do not fit the natural width, the Java width is one byte more and the sum is 2^(8 (nbytes - 1)) or
    more: the alias has a non-zero leading byte, above the packed words wherever the natural width fills them."""
    for name in we.NAMES:
        w = we.widths(name)
        rows, _ = we.catalogue(name, w["java"])
        _, absent = we.catalogue(name, w["natural"])
        assert w["java"] > w["natural"] or not [label for label in absent if label.startswith("alias")]
        for r in rows:
            if r.cls == we.ALIAS and (r.label in absent or r.label == "alias-xy" and "alias-y" in absent):
                assert r.x[0] or r.y[0], (name, r.label)
                assert w["java"] <= 4 * we.facts(name)["NW"] or int.from_bytes(r.x, "big") >> (32 * we.facts(name)["NW"]) \
                    or int.from_bytes(r.y, "big") >> (32 * we.facts(name)["NW"])


@pytest.mark.parametrize("name", we.NAMES)
def test_decode_is_libcryptos_verdict_at_the_natural_width(name):
    """EC_POINT_set_affine_coordinates on BN_bin2bn of the same bytes accepts exactly the rows with ok = True and a finite
    point -- once the range is checked beside it: libcrypto reduces the coordinates it is given (BN_nnmod in
    ossl_ec_GFp_simple_set_Jprojective_coordinates_GFp), so alone it takes every alias row, which is the very defect this
    catalogue is after.  The range comes from libcrypto too (BN_cmp against the p of EC_GROUP_get_curve), and
    EC_POINT_oct2point of 04 || x || y, which checks both itself, is asked as well."""
    lib = nc.libcrypto()
    f = we.facts(name)
    nb = we.widths(name)["natural"]
    rows, _ = we.catalogue(name, nb)
    grp = ctypes.c_void_p(lib.EC_GROUP_new_by_curve_name(lib.OBJ_sn2nid(nc.OPENSSL_SN[name].encode())))
    ctx = ctypes.c_void_p(lib.BN_CTX_new())
    p, a, b = (ctypes.c_void_p(lib.BN_new()) for _ in range(3))
    assert lib.EC_GROUP_get_curve(grp, p, a, b, ctx) == 1
    pt = ctypes.c_void_p(lib.EC_POINT_new(grp))
    taken_alone = []
    for r, (P, ok) in zip(rows, we.decoded(name, nb)):
        x, y = ctypes.c_void_p(lib.BN_bin2bn(r.x, nb, None)), ctypes.c_void_p(lib.BN_bin2bn(r.y, nb, None))
        on_curve = lib.EC_POINT_set_affine_coordinates(grp, pt, x, y, ctx) == 1
        in_range = lib.BN_cmp(x, p) < 0 and lib.BN_cmp(y, p) < 0
        want = ok and P is not None
        assert (on_curve and in_range) == want, r.label
        assert (lib.EC_POINT_oct2point(grp, pt, b"\x04" + r.x + r.y, ctypes.c_size_t(1 + 2 * nb), ctx) == 1) == want, r.label
        if on_curve and not in_range:
            taken_alone.append(r.label)
        lib.BN_free(x)
        lib.BN_free(y)
    lib.ERR_clear_error()
    assert sorted(taken_alone) == sorted(r.label for r in rows if r.cls == we.ALIAS) and taken_alone


# ---- mutants of decode() -------------------------------------------------------------------------------------------------
def caught(name, nb, rows, mutant):
    f = we.facts(name)
    return [r.label for r in rows if we.decode(f["c"], nb, r.x, r.y, mutant, f["NW"]) != we.decode(f["c"], nb, r.x, r.y)]


def distinguishable(name, width, mutant):
    """Can any input at all tell the mutant from decode() on this curve at this width?"""
    f = we.facts(name)
    nb = we.widths(name)[width]
    if mutant == we.GT_FOR_GE:                     # x = p or y = p: (0, y) needs a square b; (x, 0) a point of order 2 (cofactor 1: none)
        return name in B_IS_A_SQUARE
    if mutant == we.LOW_WORDS_ONLY:
        return nb > 4 * f["NW"]
    if mutant == we.NIST_A:
        return f["c"].a != f["c"].p - 3
    if mutant == we.NO_RANGE_Y:                 # y + p has to fit
        return "alias-y" in [r.label for r in we.catalogue(name, nb)[0]]
    return True


@pytest.mark.parametrize("mutant", we.MUTANTS)
@pytest.mark.parametrize("name", we.NAMES)
def test_catalogue_catches_the_mutant(name, mutant):
    somewhere = False
    for width in we.WIDTHS:
        nb = we.widths(name)[width]
        got = caught(name, nb, we.catalogue(name, nb)[0], mutant)
        if distinguishable(name, width, mutant):
            assert got, (width, mutant)
            somewhere = True
        elif mutant != we.NO_RANGE_Y:           # (y + p fits no row of the catalogue: other inputs might still)
            assert not got, (width, got)
    # three of the mutants can be told apart on every curve at some width; > for >= only where (0, y) is a point, and the
    # NIST a only where a is another
    c = we.facts(name)["c"]
    assert somewhere == {we.GT_FOR_GE: name in B_IS_A_SQUARE, we.NIST_A: c.a != c.p - 3}.get(mutant, True)


def test_what_catches_each_mutant():
    """The rows that do the work, by name."""
    nb = we.widths("P-256")["java"]
    rows = we.catalogue("P-256", nb)[0]
    assert caught("P-256", nb, rows, we.NO_RANGE_X) == ["alias-x+", "alias-x-"]
    assert caught("P-256", nb, rows, we.NO_RANGE_Y) == ["alias-y"]           # (alias-xy needs both checks gone)
    assert caught("P-256", nb, rows, we.GT_FOR_GE) == ["alias-x+", "alias-x-"]           # min x = 0 there: x + p = p
    assert caught("P-256", nb, rows, we.LOW_WORDS_ONLY) == ["lead-01-x", "lead-80-x", "lead-01-y", "lead-80-y"]
    assert caught("P-256", nb, rows, we.NIST_A) == []
    nb = we.widths("secp256k1")["natural"]
    got = caught("secp256k1", nb, we.catalogue("secp256k1", nb)[0], we.NIST_A)
    assert "wrong-a" in got and "G" in got


@pytest.mark.parametrize("name", we.NAMES)
def test_random_valid_points_catch_no_mutant_of_the_range_check(name):
    """300 seeded points of the curve, at the natural and the Java width: the four mutants of the range check and of the bytes
    read pass every one of them -- why the catalogue exists.  The fifth mutant is of another kind: with the wrong a every
    point of a general curve is off the curve, so any valid point catches it (the existing tests do); the catalogue's share
    is the converse, the point of the a = -3 curve that the mutant takes."""
    f = we.facts(name)
    for width in ("natural", "java"):
        nb = we.widths(name)[width]
        rows = we.random_valid_rows(name, nb, 300)
        assert len(rows) == 300 and len({r.x for r in rows}) == 300
        assert all(ok and P is not None for P, ok in we.decoded(name, nb, rows))
        for mutant in (we.NO_RANGE_X, we.NO_RANGE_Y, we.GT_FOR_GE, we.LOW_WORDS_ONLY):
            assert caught(name, nb, rows, mutant) == []
        assert len(caught(name, nb, rows, we.NIST_A)) == (300 if f["c"].a != f["c"].p - 3 else 0)


# ---- the framed form -----------------------------------------------------------------------------------------------------
def test_framed_form_and_header_mutants():
    nb = we.widths("P-256")["java"]
    rows = [r for r in we.catalogue("P-256", nb)[0] if r.cls == we.VALID]
    bt = we.framed(rows)
    assert len(bt) == 5 + len(rows) * (15 + 2 * nb) and bt[:5] == b"\x00" + len(rows).to_bytes(4, "big")
    first = bt[5:5 + 15 + 2 * nb]
    assert first == b"\x00\x00\x00\x00\x02" + b"\x01\x00\x00\x00\x21" + rows[0].x + b"\x01\x00\x00\x00\x21" + rows[0].y
    muts = we.header_mutants(rows, nb)
    assert len(muts) == 18 and len({m for _, m in muts}) == 18
    kinds = {label.split("@")[0] for label, _ in muts}
    assert kinds == {"node-tag", "child-count", "x-leaf-tag", "y-leaf-tag", "x-leaf-len+1", "y-leaf-len-1"}
    assert {int(label.split("@")[1]) for label, _ in muts} == {0, len(rows) // 2, len(rows) - 1}
    for label, m in muts:
        diff = [i for i in range(len(bt)) if bt[i] != m[i]]
        pos = int(label.split("@")[1])
        assert len(m) == len(bt) and len(diff) == 1
        assert 5 + pos * (15 + 2 * nb) <= diff[0] < 5 + pos * (15 + 2 * nb) + 15 + nb      # in that element's headers
        off = (diff[0] - 5) % (15 + 2 * nb)
        assert off < 10 or 10 + nb <= off < 15 + nb                                      # never in a coordinate
