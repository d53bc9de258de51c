"""GPU suite: k_modpow<Cfg<74, 1>> and k_modpow_phased<Cfg<74, 1>> with the 29-bit squaring reading its multiplier limbs from
registers, nothing of it going through LDS (mont28.h mont29_sqr_rows, modp_kernels.h sqr_times) -- bit for bit against Python's
pow, one element per lane forced as in tests/test_gpu_modpow29.py.

The LDS column now keeps whatever the last product left in it across the squarings of a window, so the launches cover every
window width with its own number of squarings between two products (w = 1, 2, 3 and 6), the table of each (no row beyond x,
one pair of rows, three pairs, all 31) and the all-ones exponent, where every window multiplies by the last row.  The bases
carry the edge values: 1, N - 1, 2, 2^2047 and the x for which x R' is congruent to 2^2047 - 1 mod N -- seventy limbs at
2^29 - 1 and the seventy-first at 2^17 - 1 if the entry product leaves that representative; it is only bound to stay below
2N, so the registers may as well hold 2^2047 - 1 + N (the other file has no helper for such a base; here it is
all_ones_image).  The same register is then two inputs of a row's asm statement, as a[i] and as the multiplier."""
import pytest

from oracle import pyref
from test_gpu_modpow29 import MODULI, exponents, groups, one_lane  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

RP = 1 << (29 * 71)
N = 257


def pick_window(ebits):
    """pick_window of csrc/vmnhip.hip, restated (the library has no query for the width it chose): the first w of 1 .. 7 with
    the fewest products, 2^w - 2 for the table and one per window.  If that function changes, change this one with it:
    test_the_exponent_lengths_build_every_shape_of_table only says which widths the lengths below reach under THIS model."""
    return min(range(1, 8), key=lambda w: ((1 << w) - 2 + (ebits + w - 1) // w, w))


def all_ones_image(p):
    return ((1 << 2047) - 1) * pow(RP, -1, p) % p


def edge_bases(name, n):
    p = MODULI[name]
    xs = [1 + v % (p - 1) for v in pyref.stream_ints(b"modpow29/diet/x", n, p)]
    edges = [1, p - 1, 2, 1 << 2047, all_ones_image(p)]
    assert all(0 < x < p for x in edges) and (edges[-1] * RP) % p == (1 << 2047) - 1
    xs[:len(edges)] = edges
    xs[-2:] = [all_ones_image(p), p - 1]                  # and in the ragged last tile
    return xs


_expected = {}


def expected(name, xs, es):
    """[x^e mod p] by pyref (GMP on all host cores in the GPU suite), a few elements checked against pow itself; computed once
    per set of inputs.  (Not the other file's cache: that one is keyed by the exponents alone and these bases differ.)"""
    key = (name, tuple(xs), tuple(es))
    if key not in _expected:
        p = MODULI[name]
        want = pyref.exp_array(xs, es, p)
        for i in (0, 2, 4, len(xs) // 2, len(xs) - 2):
            assert want[i] == pow(xs[i], es[i], p)
        _expected[key] = want
    return _expected[key]


def test_the_exponent_lengths_build_every_shape_of_table():
    # (20 bits build w = 2, like 8 bits: the launch at w = 3 is the one of 30 bits)
    assert [pick_window(b) for b in (3, 8, 20, 30, 2047)] == [1, 2, 2, 3, 6]


@pytest.mark.parametrize("ebits", [3, 8, 20, 30, 2047])
@pytest.mark.parametrize("name", sorted(MODULI))
def test_plain_kernel_at_every_table_size(name, ebits, groups, one_lane):
    G = groups[name]
    qbits = ((MODULI[name] - 1) // 2).bit_length()
    assert qbits == 2047
    xs = edge_bases(name, N)
    es = exponents(name, N, ebits)
    got = G.toElementArray(xs).exp(G.ringArray(es), 0 if ebits == qbits else ebits).toInts()
    assert got == expected(name, xs, es), (name, ebits)


@pytest.mark.parametrize("name", sorted(MODULI))
def test_phased_kernel_equals_the_plain_one(name, groups, one_lane, monkeypatch):
    """n = 600, full-length exponents: three tiles side by side (the plain kernel), then on two workgroup slots (the phased
    one, the table read back by other workgroups than the one that squared it together)."""
    G = groups[name]
    n = 600
    xs = edge_bases(name, n)
    es = exponents(name, n, 2047)
    X, E = G.toElementArray(xs), G.ringArray(es)
    monkeypatch.delenv("VMN_MODPOW_MAX_BLOCKS", raising=False)
    plain = X.exp(E).toInts()
    monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", "2")
    phased = X.exp(E).toInts()
    assert phased == plain
    assert plain == expected(name, xs, es)


@pytest.mark.parametrize("name", sorted(MODULI))
def test_all_ones_exponent_multiplies_by_the_last_row(name, groups, one_lane):
    G = groups[name]
    xs = edge_bases(name, N)
    es = [(1 << 2047) - 1] * N
    assert G.toElementArray(xs).expInts(es, 2047).toInts() == expected(name, xs, es)
