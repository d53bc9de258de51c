"""GPU suite: k_modpow<Cfg<74, 1>> and k_modpow_phased<Cfg<74, 1>>, which work on 71 limbs of 29 bits inside and on M28 rows
outside (modp_kernels.h, Cfg29), through the C ABI against Python's pow.

The suite's other power tests reach these two kernels only at sizes where one element per lane is the geometry of the size;
here every launch is forced into it (the small- and tiny-array thresholds at 0), at the sizes around a tile of 256 elements
for the plain kernel and over three tiles on two workgroup slots for the phased one.  tests/test_mont29_model.py checks the
same schedule on the CPU."""
import os

import pytest

from oracle import pyref

pytestmark = pytest.mark.gpu

DEFAULT_WIDE = int(os.environ.get("VMN_WIDE_MAX", 40960))
DEFAULT_WIDE8 = int(os.environ.get("VMN_WIDE8_MAX", 6144))


def generic_modulus():
    """An odd 2048-bit modulus whose low limbs are not all ones (group 14 has -1/N = 1 mod 2^29, which hides a wrong quotient
    digit).  Not a prime: the kernels need an odd modulus, and the expected values are Python pows."""
    return pyref.stream_ints(b"mont29/modulus", 1, 1 << 2048)[0] | (1 << 2047) | 1


MODULI = {"group14": pyref.RFC3526_14_P, "generic": generic_modulus()}
_expected = {}


@pytest.fixture
def one_lane(gpu_ctx):
    gpu_ctx.set_small_array_threshold(0)
    gpu_ctx.set_tiny_array_threshold(0)
    yield
    gpu_ctx.set_small_array_threshold(DEFAULT_WIDE)
    gpu_ctx.set_tiny_array_threshold(DEFAULT_WIDE8)


@pytest.fixture(scope="module")
def groups(vmn, gpu_ctx):
    return {name: vmn.ModPGroup(gpu_ctx, p, (p - 1) // 2, 4) for name, p in MODULI.items()}


def bases(name, n):
    """random ones, with 1 and p - 1 among them"""
    p = MODULI[name]
    xs = [1 + v % (p - 1) for v in pyref.stream_ints(b"modpow29/x", n, p)]
    xs[0] = p - 1
    if n > 2:
        xs[1], xs[-1] = 1, p - 1
    return xs


def exponents(name, n, ebits):
    """random ones of ebits bits with 0, 1, the largest (full length: q - 1) and a one-digit top window's extremes among them"""
    q = (MODULI[name] - 1) // 2
    full = ebits == q.bit_length()
    top = q - 1 if full else (1 << ebits) - 1
    es = [e % (top + 1) for e in pyref.stream_ints(b"modpow29/e%d" % ebits, n, 1 << ebits)]
    es[0] = top
    for i, e in enumerate((0, 1, 1 << (ebits - 1), top)):
        if 1 + i < n:
            es[1 + i] = e
    return es


def expected(name, xs, es):
    """[x^e mod p]; es: one exponent per element, or the one shared exponent.  pyref's array powers are Python's pow -- in the
    GPU suite computed by GMP on all host cores (tests/fast_pyref.py; a few elements are checked against pow itself, the
    generic modulus being no prime)."""
    key = (name, len(xs), tuple(es))
    if key not in _expected:
        p = MODULI[name]
        want = pyref.exp_array(xs, es, p) if len(es) == len(xs) else pyref.exp_scalar(xs, es[0], p)
        for i in {0, len(xs) // 2, len(xs) - 1}:
            assert want[i] == pow(xs[i], es[i % len(es)], p)
        _expected[key] = want
    return _expected[key]


@pytest.mark.parametrize("n", [1, 255, 256, 257])
@pytest.mark.parametrize("name", sorted(MODULI))
def test_plain_kernel_around_a_tile(name, n, groups, one_lane):
    G = groups[name]
    xs = bases(name, n)
    X = G.toElementArray(xs)
    qbits = ((MODULI[name] - 1) // 2).bit_length()
    for ebits in (qbits, 256, 37):                  # 342, 43 and 8 windows (w = 6, 6, 5); the top one holds 1, 4 and 2 bits
        es = exponents(name, n, ebits)
        got = X.exp(G.ringArray(es), 0 if ebits == qbits else ebits).toInts()
        assert got == expected(name, xs, es), (name, n, ebits)


@pytest.mark.parametrize("name", sorted(MODULI))
def test_all_ones_exponent_of_full_length(name, groups, one_lane):
    """2^2047 - 1 is above q: plain integers as exponents (expInts), every window digit at its largest."""
    G = groups[name]
    n = 257
    xs = bases(name, n)
    qbits = ((MODULI[name] - 1) // 2).bit_length()
    es = [(1 << qbits) - 1] * n
    es[2] = (1 << qbits) - 2
    assert G.toElementArray(xs).expInts(es, qbits).toInts() == expected(name, xs, es)


@pytest.mark.parametrize("name", sorted(MODULI))
def test_phased_kernel_three_tiles_on_two_slots(name, groups, one_lane, monkeypatch):
    """n = 600 on a "device" of two workgroup slots: k_modpow_phased, a tile's running value and table handed from workgroup
    to workgroup in the 29-bit form; only the first phase enters it and only the last one leaves it."""
    monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", "2")
    G = groups[name]
    n = 600
    xs = bases(name, n)
    X = G.toElementArray(xs)
    qbits = ((MODULI[name] - 1) // 2).bit_length()
    for ebits in (qbits, 256, 37):
        es = exponents(name, n, ebits)
        got = X.exp(G.ringArray(es), 0 if ebits == qbits else ebits).toInts()
        assert got == expected(name, xs, es), (name, ebits)


@pytest.mark.parametrize("phased", [False, True])
@pytest.mark.parametrize("name", sorted(MODULI))
def test_shared_exponent(name, phased, groups, one_lane, monkeypatch):
    """One exponent for all elements (stride 0) in the fixed-window kernels: VMN_SLIDING_WINDOW=0 keeps the full-length one
    out of the sliding-window kernel; exponents of up to 32 bits take this path anyway."""
    monkeypatch.setenv("VMN_SLIDING_WINDOW", "0")
    if phased:
        monkeypatch.setenv("VMN_MODPOW_MAX_BLOCKS", "2")
    G = groups[name]
    n = 600 if phased else 257
    xs = bases(name, n)
    X = G.toElementArray(xs)
    q = (MODULI[name] - 1) // 2
    for e in (q - 1, 0xfffffffb, 1, 0):
        assert X.exp(e).toInts() == expected(name, xs, [e]), (name, n, hex(e)[:18])
