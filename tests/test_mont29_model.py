"""CPU suite: the radix-2^29 schedule of the 2048-bit power kernels (k_modpow / k_modpow_phased of Cfg<74, 1>), executed on
Python integers before it ever runs on a GPU.

tools/gen_mont_asm.py keeps the schedule of one product -- the rows in order, the reliefs of the columns in front of the rows
RELIEF29 -- as a list that it renders to csrc/gen/mont29_rows.inc AND can execute (run29): every instruction of every row on
integers, 64-bit registers wrapping like the hardware's.  Here that model is checked for what the kernels rely on:

  * a product and a squaring of operands below 2N give a b / R' mod N as a value below 2N (R' = 2^(29*71));
  * no 64-bit column wraps: the largest value any register held is below 2^64, and below the generator's static bound;
  * in (x R -> x R' by c_in), a fixed-window power as the kernels run it, out (by c_out, canonical) is Python's pow;
  * the committed .inc is what the generator emits.

Two moduli: RFC 3526 group 14, whose low limbs are all ones (-1/N = 1 mod 2^29: a wrong quotient digit can hide there), and an
odd 2048-bit modulus with generic low limbs."""
import importlib.util
import os

import pytest

from conftest import ROOT
from oracle import pyref

spec = importlib.util.spec_from_file_location("gen_mont_asm", os.path.join(ROOT, "tools", "gen_mont_asm.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

S, BITS = 71, 29
MASK = (1 << BITS) - 1
RP = 1 << (BITS * S)                 # R'
R28 = 1 << (28 * 74)                 # R of the stored form


def limbs(x):
    assert 0 <= x < RP
    return [(x >> (BITS * j)) & MASK for j in range(S)]


def value(cols):
    return sum(c << (BITS * j) for j, c in enumerate(cols))


class Modulus:
    def __init__(self, n):
        assert n % 2 == 1 and n.bit_length() == 2048
        self.n = n
        self.limbs = limbs(n)
        self.n0inv = (-pow(n, -1, 1 << BITS)) % (1 << BITS)
        self.largest = 0             # over every product of this modulus

    def mont(self, a, b=None):
        """a b / R' mod N through the schedule (b None: the squaring schedule); operands and result below 2N."""
        sqr = b is None
        bb = a if sqr else b
        assert a < 2 * self.n and bb < 2 * self.n
        cols, big = gen.run29(S, sqr, limbs(a), limbs(bb), self.limbs, self.n0inv)
        self.largest = max(self.largest, big)
        assert big < 1 << 64, "a column wrapped"
        r = value(cols)                                  # what normalize() resolves: the same value in 71 limbs
        assert r < 2 * self.n and r < RP, "the lazy bound"
        assert r % self.n == a * bb * pow(RP, -1, self.n) % self.n
        return r


def generic_modulus():
    n = pyref.stream_ints(b"mont29/modulus", 1, 1 << 2048)[0] | (1 << 2047) | 1
    assert limbs(n)[0] != MASK and limbs(n)[1] != MASK
    return n


MODULI = {"group14": pyref.RFC3526_14_P, "generic": generic_modulus()}


@pytest.fixture(scope="module", params=sorted(MODULI))
def mod(request):
    return Modulus(MODULI[request.param])


def operands(mod):
    r1, r2 = (v % (2 * mod.n) for v in pyref.stream_ints(b"mont29/ops", 2, 1 << 2050))
    return {"r1": r1, "r2": r2, "0": 0, "1": 1, "N-1": mod.n - 1, "all ones, clipped": min(RP - 1, 2 * mod.n - 1)}


def test_the_generic_modulus_does_not_hide_the_quotient_digit():
    assert Modulus(MODULI["group14"]).n0inv == 1
    assert Modulus(MODULI["generic"]).n0inv not in (1, MASK)


def test_products_and_squarings(mod):
    ops = operands(mod)
    for name, a in ops.items():
        mod.mont(a)
    top = ops["all ones, clipped"]
    for a, b in [("r1", "r2"), ("r2", "r1"), ("r1", "0"), ("1", "r2"), ("r1", "1"), ("N-1", "N-1"), ("N-1", "r1")]:
        mod.mont(ops[a], ops[b])
    for b in ops.values():
        mod.mont(top, b)
        mod.mont(b, top)
    assert mod.largest < 1 << 64


@pytest.mark.parametrize("sqr", [False, True])
def test_columns_stay_below_the_static_bound(sqr):
    """Every limb of both operands and of the "modulus" at 2^29-1 (no valid operands: the columns' worst case)."""
    bound = gen.static_bound29(S, sqr)
    assert bound < 1 << 64
    top = [MASK] * S
    largest = 0
    for n0inv in (1, MASK, 0x0f0f0f0f & MASK):
        cols, big = gen.run29(S, sqr, top, top, top, n0inv)
        largest = max(largest, big)
    assert largest <= bound
    assert largest > 1 << 63, "the reliefs are needed: without a bound this close the schedule would carry spare ones"
    for m in (Modulus(n) for n in MODULI.values()):       # real operands stay below it too
        t = min(RP - 1, 2 * m.n - 1)
        m.mont(t, None if sqr else t)
        assert m.largest <= bound


def test_one_relief_less_wraps():
    """The generator refuses a schedule whose bound reaches 2^64."""
    keep = gen.RELIEF29
    try:
        gen.RELIEF29 = keep[:1]
        assert gen.static_bound29(S, False) >= 1 << 64
        with pytest.raises(SystemExit):
            gen.gen29(S)
    finally:
        gen.RELIEF29 = keep


@pytest.mark.parametrize("x_of,e", [(lambda n: pyref.stream_ints(b"mont29/x", 1, n)[0], 0xb5c0fd), (lambda n: n - 1, 0x3fffff),
                                    (lambda n: 1, 0x800001), (lambda n: pyref.stream_ints(b"mont29/y", 1, n)[0], 0)])
def test_in_power_out_is_pow(mod, x_of, e):
    """The kernels' own sequence: the stored x R enters with c_in, a table of 2^w rows from R' mod N, the top window read from
    the table, w squarings and a product per further window, out with c_out, canonical."""
    n, w, ebits = mod.n, 3, 24
    x = x_of(n)
    c_in, c_out, one = RP * RP * pow(R28, -1, n) % n, R28 % n, RP % n
    a = mod.mont(x * R28 % n, c_in)
    assert a % n == x * RP % n
    tab = [one, a]
    for k in range(2, 1 << w):
        tab.append(mod.mont(a, tab[-1]))
    nwin = (ebits + w - 1) // w
    digit = lambda wi: (e >> (wi * w)) & ((1 << w) - 1)
    acc = tab[digit(nwin - 1)]
    for wi in range(nwin - 2, -1, -1):
        for _ in range(w):
            acc = mod.mont(acc)
        acc = mod.mont(acc, tab[digit(wi)])
    y = mod.mont(acc, c_out)
    y -= n if y >= n else 0
    assert y == pow(x, e, n) * R28 % n


def test_committed_rows_are_the_generated_ones():
    with open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "gen", "mont29_rows.inc")) as f:
        assert f.read() == gen.render29([S])
