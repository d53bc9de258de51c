"""The operand catalogue of tests/ring_edges.py is not vacuous: for every built geometry and every ring modulus it holds
the operands whose carries and borrows run through a whole lane's share, at every share boundary, and the exact sums.
Conditions on the inputs alone, from Python integers (an element = limbs of 28 bits cut into shares of L limbs); the
kernels meet these operands in tests/test_gpu_ring_edges.py."""
import pytest

import ring_edges as re_

CASES = [(geo.id, name) for geo in re_.GEOMETRIES for name in re_.moduli(geo)]
MULTI_LANE = [geo.id for geo in re_.GEOMETRIES if geo.LPE > 1]

# (condition, modulus) -> the geometries in which the condition cannot be met, and why.  A listed case must really be unmet
# (test_skip_list_is_exact), so the list cannot hide a hole of the catalogue.
SKIP = {
    # a full-share carry into share h needs an operand with limbs in share h - 1; below 2^256 everything is in share 0
    # (a share is at least 10 limbs = 280 bits in every multi-lane geometry)
    ("a", "small256"): (MULTI_LANE, "operands below 2^256 have no limb above share 0"),
    # q - a borrows out of limb j only if q[j] - a[j] - borrow < 0; every limb of 2^bits - 1 below the top one is 0xfffffff
    ("d", "ones"): (MULTI_LANE, "no limb of N - a borrows when every limb of N is all ones"),
    ("d", "small256"): (MULTI_LANE, "q - a has no limb above share 0"),
}
# No condition may lose more than one modulus per geometry -- except (d), which is impossible for BOTH of the moduli above,
# each by the one-line argument next to it: that pair is the whole allowance.
MOST_SKIPPED = {"a": 1, "b": 1, "c": 1, "d": 2}


def skipped(cond, geo_id, name):
    geos, _ = SKIP.get((cond, name), ((), ""))
    return geo_id in geos


_cache = {}


def findings(geo_id, name):
    """{condition: True / False} (a, b: per boundary h) for one geometry and modulus, computed once."""
    if (geo_id, name) not in _cache:
        geo = re_.GEOMETRY[geo_id]
        q = re_.modulus(geo, name)
        pairs = re_.catalogue(q, geo.bits)
        hs = range(1, geo.LPE)
        a_left, b_left = set(hs), set(hs)
        for a, b in pairs:
            for h in list(a_left):
                if re_.carry_ripples_through_share(a, b, geo, h):
                    a_left.discard(h)
            for h in list(b_left):
                if re_.borrow_ripples_through_share(a + b, q, geo, h):
                    b_left.discard(h)
            if not a_left and not b_left:
                break
        sums = {a + b for a, b in pairs}
        operands = {v for pair in pairs for v in pair}
        d = any(re_.negation_borrows_across_every_boundary(v, q, geo) for v in operands)
        _cache[(geo_id, name)] = {"a": not a_left, "b": not b_left, "c": {q - 1, q, q + 1, 2 * q - 2} <= sums, "d": d,
                                  "a_left": sorted(a_left), "b_left": sorted(b_left), "pairs": pairs, "q": q}
    return _cache[(geo_id, name)]


@pytest.mark.parametrize("geo_id,name", CASES)
def test_catalogue_is_deterministic_and_in_range(geo_id, name):
    f = findings(geo_id, name)
    geo, q, pairs = re_.GEOMETRY[geo_id], f["q"], f["pairs"]
    assert q % 2 == 1 and q.bit_length() <= geo.bits and q.bit_length() + 2 <= 28 * geo.S
    assert pairs == re_.catalogue(q, geo.bits)
    assert all(0 <= a < q and 0 <= b < q for a, b in pairs) and len(set(pairs)) == len(pairs)
    assert pairs[-1] == (q - 1, q - 1), "an edge value sits last"
    limit = 2000 if geo.bits >= 8192 else 8000
    assert 50 < len(pairs) <= limit, len(pairs)
    # the Montgomery preimages are the pairs again once multiplied by R
    R = 1 << (28 * geo.rows)
    pre = re_.montgomery_preimages(pairs[:50] + pairs[-50:], q, geo.rows)
    assert [(a * R % q, b * R % q) for a, b in pre] == pairs[:50] + pairs[-50:]


@pytest.mark.parametrize("geo_id,name", CASES)
def test_full_share_carry_at_every_boundary(geo_id, name):
    """(a): for every share boundary a pair whose sum carries into share h through a share h - 1 of all-ones sums."""
    if skipped("a", geo_id, name):                          # cannot be met (SKIP gives the reason): and it is not
        assert not findings(geo_id, name)["a"], SKIP[("a", name)][1]
        return
    f = findings(geo_id, name)
    assert f["a"], "no full-share carry into the shares %s" % f["a_left"]


@pytest.mark.parametrize("geo_id,name", CASES)
def test_full_share_borrow_at_every_boundary(geo_id, name):
    """(b): for every share boundary an x = a + b for which x - q borrows into share h through an all-zero difference share."""
    if skipped("b", geo_id, name):                          # cannot be met (SKIP gives the reason): and it is not
        assert not findings(geo_id, name)["b"], SKIP[("b", name)][1]
        return
    f = findings(geo_id, name)
    assert f["b"], "no full-share borrow into the shares %s" % f["b_left"]


@pytest.mark.parametrize("geo_id,name", CASES)
def test_exact_sums(geo_id, name):
    """(c): pairs with a + b = q - 1, q, q + 1 and 2q - 2."""
    assert not skipped("c", geo_id, name)
    assert findings(geo_id, name)["c"]


@pytest.mark.parametrize("geo_id,name", CASES)
def test_negation_borrows_across_every_boundary(geo_id, name):
    """(d): an operand a for which q - a borrows into every share above the lowest."""
    if skipped("d", geo_id, name):                          # cannot be met (SKIP gives the reason): and it is not
        assert not findings(geo_id, name)["d"], SKIP[("d", name)][1]
        return
    assert findings(geo_id, name)["d"]


def test_skip_list_is_exact():
    """A skipped case is one the catalogue really does not meet, names a real geometry and modulus, and no condition loses
    more moduli in a geometry than MOST_SKIPPED allows."""
    for (cond, name), (geos, reason) in SKIP.items():
        assert cond in MOST_SKIPPED and name in re_.MODULI and reason
        for geo_id in geos:
            assert (geo_id, name) in CASES
            assert findings(geo_id, name)[cond] is False, (cond, geo_id, name)
    for geo in re_.GEOMETRIES:
        for cond, most in MOST_SKIPPED.items():
            lost = [name for name in re_.moduli(geo) if skipped(cond, geo.id, name)]
            assert len(lost) <= most, (geo.id, cond, lost)


def test_every_built_geometry_is_listed():
    """The table follows size_for_bits() and the wide forms of csrc/modp_kernels.h: limbs split evenly, R = 2^(28 rows) > 4N."""
    assert [g.bits for g in re_.GEOMETRIES] == [256, 384, 512, 1024, 2048, 2048, 2048, 3072, 3072, 4096, 8192, 16384]
    for g in re_.GEOMETRIES:
        assert g.S % g.LPE == 0 and 28 * g.rows >= g.bits + 2 and g.rows <= g.S
        assert (g.force is None) == (g.bits not in (2048, 3072))
