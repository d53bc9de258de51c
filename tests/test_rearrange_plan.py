"""CPU suite: the plans of verificatum_vmn_amd/rearrange.py -- which component array of which input every component array of
every output is -- on plain integers, and the list operations on a host stand-in for the device arrays.  The expected values are
written down from the reference's definitions (ProtocolElGamalRear.java:72-105, 199-213, 297-375, 387-419, 430-473 and
ProtocolElGamalRearTool.java:88-125), component by component, not computed by the plans.

A list is what proofdir.read_array_nests returns: kappa * omega component arrays per nest, component c = l * kappa + j, the u nest
before the v nest.  Here a component array is a label ("u" / "v" / "m", input, l, j) or a short list of integers."""
import pytest

from fake_backend import FakeG, FakeGroup


@pytest.fixture(scope="module")
def rear(vmn):
    from verificatum_vmn_amd import rearrange
    return rearrange


def plain_list(i, width, kappa):
    return [("m", i, l, j) for l in range(width) for j in range(kappa)]


def ciph_list(i, width, kappa):
    return [(h, i, l, j) for h in "uv" for l in range(width) for j in range(kappa)]


def apply(plan, inputs):
    return [[inputs[i][c] for i, c in out] for out in plan]


# ---- TestProtocolElGamalRear.constructOutputElement (:112-180): its three cases, element for array ---------------------------------
def test_pick_element_one_of_ten(rear):
    inputs = [plain_list(i, 1, 1) for i in range(10)]
    assert apply(rear.plan_shallow([1] * 10, 1, rear.parse_format("(1,0)"), False), inputs) == [[("m", 1, 0, 0)]]      # inputs.get(1) itself


def test_combine_elements_zero_and_two(rear):
    inputs = [plain_list(i, 1, 1) for i in range(10)]
    assert apply(rear.plan_shallow([1] * 10, 1, rear.parse_format("(0,0)x(2,0)"), False), inputs) == [[("m", 0, 0, 0), ("m", 2, 0, 0)]]


def test_pick_components_at_width_five(rear):
    inputs = [plain_list(i, 5, 1) for i in range(10)]
    got = apply(rear.plan_shallow([5] * 10, 1, rear.parse_format("(0,0)x(2,3)"), False), inputs)
    assert got == [[("m", 0, 0, 0), ("m", 2, 3, 0)]]                   # product(inputs[0].project(0), inputs[2].project(3))


# ---- shallow ---------------------------------------------------------------------------------------------------------------------
def test_shallow_ciphertexts_under_keywidth_two(rear):
    widths, kappa = [2, 1, 3], 2
    inputs = [ciph_list(i, w, kappa) for i, w in enumerate(widths)]
    fmt = rear.parse_format("(0,1)x(2,2)x(1,0):(2,0-2)")
    assert fmt == [[(0, 1), (2, 2), (1, 0)], [(2, 0), (2, 1)]]
    got = apply(rear.plan_shallow(widths, kappa, fmt, True), inputs)
    want0 = [(h, i, l, j) for h in "uv" for i, l in ((0, 1), (2, 2), (1, 0)) for j in range(2)]        # width 3 under keywidth 2
    want1 = [(h, 2, l, j) for h in "uv" for l in (0, 1) for j in range(2)]                               # width 2
    assert got == [want0, want1]
    # plaintexts: the same positions, one nest
    got = apply(rear.plan_shallow(widths, kappa, fmt, False), [plain_list(i, w, kappa) for i, w in enumerate(widths)])
    assert got == [[("m",) + t[1:] for t in want0[:6]], [("m",) + t[1:] for t in want1[:4]]]


# ---- deep ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ciphs", [False, True])
def test_deep_joins_keywidths_one_and_two_into_three_and_back(rear, ciphs):
    w, mk = 2, (ciph_list if ciphs else plain_list)
    halves = "uv" if ciphs else "m"
    a, b = mk(0, w, 1), mk(1, w, 2)
    join = rear.plan_deep([1, 2], w, rear.parse_format("(0,0)x(1,0-2)"), ciphs)
    (joint,) = apply(join, [a, b])
    # array (l, m) of the output of keywidth 3: m = 0 the one key of input 0, m = 1, 2 the two keys of input 1
    assert joint == [(h, s, l, j) for h in halves for l in range(w) for s, j in ((0, 0), (1, 0), (1, 1))]
    assert len(joint) == (2 if ciphs else 1) * 3 * w
    back = rear.plan_deep([3], w, rear.parse_format("(0,0):(0,1-3)"), ciphs)
    assert apply(back, [joint]) == [a, b]


def test_deep_at_width_one_is_the_reference_help_text_flow(rear):
    """Two lists under single keys joined into one under the combined key; the part under the first key cut out again."""
    a, b = ciph_list(0, 1, 1), ciph_list(1, 1, 1)
    (joint,) = apply(rear.plan_deep([1, 1], 1, rear.parse_format("(0,0)x(1,0)"), True), [a, b])
    assert joint == [("u", 0, 0, 0), ("u", 1, 0, 0), ("v", 0, 0, 0), ("v", 1, 0, 0)]
    assert apply(rear.plan_deep([2], 1, rear.parse_format("(0,0)"), True), [joint]) == [a]


# ---- public keys -------------------------------------------------------------------------------------------------------------------
def test_pkeys_one_plus_two_into_three_and_into_a_plain_pair(rear):
    k0 = ["g0", "y0"]
    k1 = ["g10", "g11", "y10", "y11"]
    got = apply(rear.plan_pkeys([1, 2], rear.parse_format("(0,0)x(1,0-2)")), [k0, k1])
    assert got == [["g0", "g10", "g11", "y0", "y10", "y11"]]                 # the g rows, then the y rows
    got = apply(rear.plan_pkeys([1, 2], rear.parse_format("(1,1):(0,0)")), [k0, k1])
    assert got == [["g11", "y11"], ["g0", "y0"]]                             # one position: a plain pair, two rows


# ---- [NOT-IN-REF] errors -----------------------------------------------------------------------------------------------------------
def test_a_position_whose_source_or_index_does_not_exist(rear):
    E = rear.RearrangeFormatError
    with pytest.raises(E, match="source 3"):
        rear.plan_shallow([2, 1, 3], 2, [[(3, 0)]], True)
    with pytest.raises(E, match="index 1"):
        rear.plan_shallow([2, 1, 3], 2, [[(0, 0), (1, 1)]], True)
    rear.plan_shallow([2, 1, 3], 2, [[(2, 2)]], True)
    with pytest.raises(E, match="index 3"):
        rear.plan_shallow([2, 1, 3], 2, [[(2, 3)]], False)
    with pytest.raises(E, match="source 2"):
        rear.plan_deep([1, 2], 2, [[(2, 0)]], False)
    with pytest.raises(E, match="index 2"):
        rear.plan_deep([1, 2], 2, [[(1, 2)]], False)
    with pytest.raises(E, match="index 1"):
        rear.plan_pkeys([1, 2], [[(0, 1)]])
    with pytest.raises(E, match="source 2"):
        rear.plan_pkeys([1, 2], [[(2, 0)]])
    with pytest.raises(E):
        rear.plan_shallow([2, 0], 1, [[(0, 0)]], False)


def test_a_count_of_outputs_that_differs_from_the_formats(rear):
    E = rear.RearrangeFormatError
    fmt = rear.parse_format("(0,0):(0,1)")
    assert len(rear.plan_shallow([2], 1, fmt, False, outputs=2)) == 2
    for n in (1, 3):
        with pytest.raises(E, match="do not match"):
            rear.plan_shallow([2], 1, fmt, False, outputs=n)
        with pytest.raises(E, match="do not match"):
            rear.plan_deep([2], 1, fmt, False, outputs=n)
        with pytest.raises(E, match="do not match"):
            rear.plan_pkeys([2], fmt, outputs=n)


def test_inputs_of_different_lengths(rear):
    grp = FakeGroup(23, 11, 2)
    ten, nine = FakeG(grp, range(1, 11)), FakeG(grp, range(1, 10))
    with pytest.raises(rear.RearrangeFormatError, match="differ in length"):
        rear.rearrange_shallow([[ten, ten], [nine]], [2, 1], 1, [[(0, 0), (1, 0)]], False)
    with pytest.raises(rear.RearrangeFormatError, match="differ in length"):
        rear.rearrange_deep([[ten], [nine, nine]], [1, 2], 1, [[(0, 0), (1, 0)]], False)


# ---- sub and cat on a host stand-in --------------------------------------------------------------------------------------------------
class HostGroup:
    def fromSegments(self, arrays, froms, tos):
        assert all(0 <= f <= t <= a.size() for a, f, t in zip(arrays, froms, tos))
        return HostArray(self, [x for a, f, t in zip(arrays, froms, tos) for x in a.v[f:t]])

    def concat(self, arrays):
        return self.fromSegments(arrays, [0] * len(arrays), [a.size() for a in arrays])


class HostArray:
    def __init__(self, group, v):
        self.group, self.v = group, list(v)

    def size(self):
        return len(self.v)

    def free(self):
        self.v = None


def test_sub_and_cat(rear):
    g = HostGroup()
    comps = [HostArray(g, range(100 * c, 100 * c + 10)) for c in range(4)]
    parts = rear.sub_arrays(comps, rear.parse_intervals("0-3:3-10"))
    assert [[a.v for a in part] for part in parts] == [[c.v[0:3] for c in comps], [c.v[3:10] for c in comps]]
    assert [a.v for a in rear.cat_arrays(parts)] == [c.v for c in comps]
    parts = rear.sub_arrays(comps, rear.parse_intervals("2-7:5-9"))                     # intervals may intersect
    assert [[a.v for a in part] for part in parts] == [[c.v[2:7] for c in comps], [c.v[5:9] for c in comps]]
    empty = [HostArray(g, []) for _ in range(4)]
    assert [a.v for a in rear.cat_arrays([empty, comps, empty])] == [c.v for c in comps]   # an empty input is allowed
    with pytest.raises(rear.RearrangeFormatError, match="differ in width"):
        rear.cat_arrays([comps, comps[:2]])


def test_all_intervals_are_checked_before_anything_is_made(rear):
    made = []

    class Counting(HostGroup):
        def fromSegments(self, arrays, froms, tos):
            made.append(1)
            return HostGroup.fromSegments(self, arrays, froms, tos)
    comps = [HostArray(Counting(), range(10))]
    with pytest.raises(rear.RearrangeFormatError) as exc:
        rear.sub_arrays(comps, [(0, 3), (5, 11)])
    assert str(exc.value) == "Interval out of bounds! 5-11. Length of array is 10!" and made == []


def test_shallow_and_deep_copy_the_chosen_arrays(rear):
    g = HostGroup()
    a = [HostArray(g, [10 * c + k for k in range(3)]) for c in range(6)]               # ciphertexts of width 3
    b = [HostArray(g, [100 + 10 * c + k for k in range(3)]) for c in range(2)]         # ciphertexts of width 1
    (out0, out1) = rear.rearrange_shallow([a, b], [3, 1], 1, rear.parse_format("(0,2)x(1,0):(0,0-2)"), True)
    assert [x.v for x in out0] == [a[2].v, b[0].v, a[5].v, b[1].v]
    assert [x.v for x in out1] == [a[0].v, a[1].v, a[3].v, a[4].v]
    assert all(x is not y for x in out0 + out1 for y in a + b)
    (joint,) = rear.rearrange_deep([b, b], [1, 1], 1, rear.parse_format("(0,0)x(1,0)"), True)
    assert [x.v for x in joint] == [b[0].v, b[0].v, b[1].v, b[1].v]
    keys = [HostArray(g, ["g0", "y0"]), HostArray(g, ["g10", "g11", "y10", "y11"])]
    (wide, pair) = rear.rearrange_pkeys(keys, rear.parse_format("(0,0)x(1,0-2):(1,1)"))
    assert wide.v == ["g0", "g10", "g11", "y0", "y10", "y11"] and pair.v == ["g11", "y11"]
