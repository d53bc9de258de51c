"""GPU suite: k_modpow<Cfg<74, 1>, true> and k_modpow_phased<Cfg<74, 1>, true>, the variable-base powers of a modulus
N = -1 mod 2^58 on the SHORT rows of mont28.h (quotient digit = low limb of column 0, reduction by N'' = (N + 1) >> 58), through
the C ABI: every launch once on the short rows and once with VMN_POW29_SHORT=0 on the general rows, the two compared with each
other and with Python's pow.  One element per lane is forced as in tests/test_gpu_modpow29.py.

The moduli are those of tests/test_mont29_short_model.py, the shapes N'' can take (odd suffices for the kernels; the expected
values are pows).  The bases carry 1, N - 1, 2, the top bit alone (2^2047 for the 2048-bit moduli), the base whose image x R' is
all ones below that bit (all_ones_image of tests/test_gpu_modpow29_diet.py) and one whose image has the low limb 0 -- the
first row of its products has the quotient digit 0.  The exponent lengths 3, 8, 30 and 2047 build the tables of the window
widths 1, 2, 3 and 6; each array holds 0, 1, the top bit alone and the all-ones exponent of its length."""
import pytest

from oracle import pyref
from test_gpu_modpow29 import one_lane  # noqa: F401  (fixture)
from test_gpu_modpow29_diet import pick_window
from test_mont29_short_model import MODULI

pytestmark = pytest.mark.gpu

RP = 1 << (29 * 71)
_expected = {}


@pytest.fixture(scope="module")
def groups(vmn, gpu_ctx):
    return {name: vmn.ModPGroup(gpu_ctx, p, (p - 1) // 2, 4) for name, p in MODULI.items()}


def image_base(p, v):
    """x with x R' = v mod p"""
    x = v * pow(RP, -1, p) % p
    assert 0 < x < p and x * RP % p == v
    return x


def edge_bases(name, n):
    p = MODULI[name]
    xs = [1 + v % (p - 1) for v in pyref.stream_ints(b"modpow29/short/x", n, p)]
    low0 = (xs[0] >> 29 << 29) % p
    assert low0 and low0 % (1 << 29) == 0
    edges = [image_base(p, (1 << (p.bit_length() - 1)) - 1), 1, p - 1, 2, 1 << (p.bit_length() - 1), image_base(p, low0)]
    xs[:len(edges)] = edges[:n]
    if n > len(edges) + 2:
        xs[-2:] = [edges[0], p - 1]                               # and in the ragged last tile
    return xs


def exponents(n, ebits):
    top = (1 << ebits) - 1
    es = [e % (top + 1) for e in pyref.stream_ints(b"modpow29/short/e%d" % ebits, n, 1 << ebits)]
    es[0] = top
    for i, e in enumerate((0, 1, 1 << (ebits - 1), top)):
        if 1 + i < n:
            es[1 + i] = e
    return es


def exp_array_any(xs, es, p):
    """pyref.exp_array, also where an exponent is not below p (the 2000-bit modulus under 2047-bit exponents), which the GMP
    oracle behind it does not take: x^e = (x^(e >> 1024))^(2^1024) x^(e mod 2^1024), every exponent below p."""
    if all(e < p for e in es):
        return pyref.exp_array(xs, es, p)
    half = 1024
    assert p >> half and all(e >> half < p for e in es)
    hi = pyref.exp_array(pyref.exp_array(xs, [e >> half for e in es], p), [1 << half] * len(xs), p)
    lo = pyref.exp_array(xs, [e & ((1 << half) - 1) for e in es], p)
    return [h * l % p for h, l in zip(hi, lo)]


def expected(name, xs, es):
    """[x^e mod p] by pyref (GMP on all host cores in the GPU suite), a few elements checked against pow itself; once per input."""
    key = (name, tuple(xs), tuple(es))
    if key not in _expected:
        p = MODULI[name]
        want = exp_array_any(xs, es, p)
        for i in {0, len(xs) // 2, len(xs) - 1}:
            assert want[i] == pow(xs[i], es[i], p)
        _expected[key] = want
    return _expected[key]


def both_rows(X, es, ebits, monkeypatch):
    """X^es on the short rows, then on the general ones"""
    monkeypatch.delenv("VMN_POW29_SHORT", raising=False)
    short = X.expInts(es, ebits).toInts()
    monkeypatch.setenv("VMN_POW29_SHORT", "0")
    general = X.expInts(es, ebits).toInts()
    monkeypatch.delenv("VMN_POW29_SHORT")
    return short, general


def test_the_exponent_lengths_build_every_shape_of_table():
    assert [pick_window(b) for b in (3, 8, 30, 2047)] == [1, 2, 3, 6]


@pytest.mark.parametrize("name", sorted(MODULI))
def test_the_short_rows_are_taken_and_can_be_turned_off(name, groups, gpu_ctx, one_lane, monkeypatch):
    """The multiply-adds the library books for a launch: S (S - 2) per reduction on the short rows, S^2 on the general ones."""
    n, ebits = 1, 8
    X = groups[name].toElementArray(edge_bases(name, n))
    es = exponents(n, ebits)
    booked = []
    gpu_ctx.timing_enable(True)
    try:
        for env in (None, "1", "0"):
            if env is None:
                monkeypatch.delenv("VMN_POW29_SHORT", raising=False)
            else:
                monkeypatch.setenv("VMN_POW29_SHORT", env)
            gpu_ctx.timing_reset()
            X.expInts(es, ebits)
            booked.append(gpu_ctx.timing_report()["modpow"][2])
    finally:
        gpu_ctx.timing_enable(False)
    w, S = 2, 71
    products, squarings = (ebits // w - 1) + (1 << w) - 2 + 2, (ebits // w - 1) * w
    assert booked[2] - booked[0] == 2 * S * (products + squarings)
    assert booked[1] == booked[0]


@pytest.mark.parametrize("ebits", [3, 8, 30, 2047])
@pytest.mark.parametrize("name", sorted(MODULI))
def test_plain_kernel_at_every_table_size(name, ebits, groups, one_lane, monkeypatch):
    n = 257
    xs = edge_bases(name, n)
    es = exponents(n, ebits)
    short, general = both_rows(groups[name].toElementArray(xs), es, ebits, monkeypatch)
    assert short == general, (name, ebits)
    assert short == expected(name, xs, es), (name, ebits)


@pytest.mark.parametrize("name", sorted(MODULI))
def test_plain_kernel_on_one_element(name, groups, one_lane, monkeypatch):
    """The all-ones base to the all-ones exponent, alone in its tile."""
    xs = edge_bases(name, 1)
    es = [(1 << 2047) - 1]
    short, general = both_rows(groups[name].toElementArray(xs), es, 2047, monkeypatch)
    assert short == general
    assert short == [pow(xs[0], es[0], MODULI[name])]


@pytest.mark.parametrize("name", sorted(MODULI))
def test_phased_kernel_three_tiles_on_two_slots(name, groups, one_lane, monkeypatch):
    """n = 600 on a "device" of two workgroup slots: the phased kernel, whose last phase alone reads N itself (to leave the
    domain canonical) while every phase reduces by N''."""
    monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", "2")
    n = 600
    xs = edge_bases(name, n)
    X = groups[name].toElementArray(xs)
    for ebits in (2047, 30):
        es = exponents(n, ebits)
        short, general = both_rows(X, es, ebits, monkeypatch)
        assert short == general, (name, ebits)
        assert short == expected(name, xs, es), (name, ebits)
