"""CPU suite: the SHORT radix-2^29 rows of the 2048-bit power kernels (k_modpow / k_modpow_phased of Cfg<74, 1> for a modulus
N = -1 mod 2^58), executed on Python integers.

tools/gen_mont_asm.py emits a second family of rows for such a modulus (_row, short): the quotient digit is the low limb of
column 0, and the reduction adds m * N'' * 2^58 - m with N'' = (N + 1) >> 58 -- nothing but a carry for columns 0 and 1, 69
multiply-adds for the columns above.  The generator's model (run29) executes the emitted text, so what is checked here is the
text the GPU gets:

  * a product and a squaring of operands below 2N give a b / R' mod N as a value below 2N;
  * the columns, normalised to 71 limbs, are those of the GENERAL rows on the same operands, limb for limb;
  * no 64-bit column wraps, on these operands and under the static bound (every limb and quotient digit at 2^29 - 1);
  * the detector: 58 trailing one bits make a modulus short, 57 do not.

The moduli are the shapes N'' can take: RFC 3526 group 14 (64 trailing ones), exactly 58 trailing ones, 87 and more (the low limb
of N'' is zero), 2^2048 - 1 (N + 1 carries out of 2048 bits, N'' = 2^1990) and a 2000-bit modulus (the top limbs of N'' are zero).
They need not be prime: the rows only need an odd modulus."""
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
ONES = 2 * BITS                      # trailing ones the short rows need


def limbs(x, count=S):
    assert 0 <= x < 1 << (BITS * count)
    return [(x >> (BITS * j)) & MASK for j in range(count)]


def value(cols):
    return sum(c << (BITS * j) for j, c in enumerate(cols))


def trailing_ones(n):
    return ((n + 1) & -(n + 1)).bit_length() - 1


def with_trailing_ones(seed, bits, ones):
    """An odd number of `bits` bits with exactly `ones` trailing one bits and random bits above them."""
    r = pyref.stream_ints(seed, 1, 1 << bits)[0] | (1 << (bits - 1))
    n = (r >> (ones + 1) << (ones + 1)) | ((1 << ones) - 1)
    assert n.bit_length() == bits and trailing_ones(n) == ones
    return n


MODULI = {
    "group14": pyref.RFC3526_14_P,
    "58 ones": with_trailing_ones(b"mont29s/58", 2048, 58),
    "87 ones": with_trailing_ones(b"mont29s/87", 2048, 87),
    "2^2048-1": (1 << 2048) - 1,
    "2000 bits": with_trailing_ones(b"mont29s/2000", 2000, 58),
}


def test_the_moduli_are_the_shapes_they_are_named_for():
    assert trailing_ones(MODULI["group14"]) == 64
    assert not (MODULI["58 ones"] >> 58) & 1
    for name, n in MODULI.items():
        assert gen.short29_modulus(n), name
        ns = (n + 1) >> ONES
        assert ns < 1 << (BITS * (S - 2)), name                   # N'' fits the 69 operands of a row
    assert limbs((MODULI["87 ones"] + 1) >> ONES, S - 2)[0] == 0
    assert limbs((MODULI["2^2048-1"] + 1) >> ONES, S - 2) == [0] * 68 + [1 << 18]
    assert limbs((MODULI["2000 bits"] + 1) >> ONES, S - 2)[-2:] == [0, 0]


def test_the_detector_needs_58_trailing_ones():
    assert gen.SHORT29_ONES == ONES
    for bits in (2048, 2000):
        assert not gen.short29_modulus(with_trailing_ones(b"mont29s/edge", bits, 57))
        assert gen.short29_modulus(with_trailing_ones(b"mont29s/edge", bits, 58))
        assert gen.short29_modulus(with_trailing_ones(b"mont29s/edge", bits, 59))
    assert not gen.short29_modulus(pyref.stream_ints(b"mont29/modulus", 1, 1 << 2048)[0] | (1 << 2047) | 1)


@pytest.mark.parametrize("sqr", [False, True])
def test_static_bound_of_the_short_schedule(sqr):
    """Every limb, every limb of N'' and every quotient digit at 2^29 - 1, nothing wrapping: no register reaches 2^64, and none
    exceeds the general schedule's (fewer terms land in every column)."""
    bound = gen.static_bound29(S, sqr, short=True)
    assert bound < 1 << 64
    assert bound <= gen.static_bound29(S, sqr)


def normalised(cols):
    v = value(cols)
    assert v < RP
    return limbs(v)


class Modulus:
    def __init__(self, n):
        self.n = n
        self.limbs = limbs(n)
        self.ns = limbs((n + 1) >> ONES, S - 2)
        self.n0inv = (-pow(n, -1, 1 << BITS)) % (1 << BITS)
        assert self.n0inv == 1

    def check(self, a, b=None):
        """a b / R' mod N through the short schedule (b None: the squaring schedule) against the definition and against the
        general schedule."""
        sqr = b is None
        bb = a if sqr else b
        assert a < 2 * self.n and bb < 2 * self.n
        cols, big = gen.run29(S, sqr, limbs(a), limbs(bb), self.ns, 0, short=True)
        assert big < 1 << 64, "a column wrapped"
        r = value(cols)
        assert r < 2 * self.n and r < RP, "the lazy bound"
        assert r % self.n == a * bb * pow(RP, -1, self.n) % self.n
        general, big = gen.run29(S, sqr, limbs(a), limbs(bb), self.limbs, self.n0inv)
        assert big < 1 << 64
        assert normalised(cols) == normalised(general)
        return cols


@pytest.fixture(scope="module", params=sorted(MODULI))
def mod(request):
    return Modulus(MODULI[request.param])


def operands(n):
    """0, 1, N - 1, 2N - 1 (the largest operand a row may see), the largest 2^k - 1 below 2N (its limbs all at 2^29 - 1
    up to the top one), two random ones, and the operands that steer the FIRST row's quotient digit m = a[0] b[0] mod 2^29: a low limb of 0 (m = 0) and the pair of low
    limbs 1 and 2^29 - 1 (m = 2^29 - 1; no squaring has it, -1 is not a square mod 2^29)."""
    r1, r2 = (v % (2 * n) for v in pyref.stream_ints(b"mont29s/ops", 2, 1 << 2050))
    return {"0": 0, "1": 1, "N-1": n - 1, "2N-1": 2 * n - 1, "all ones": (1 << ((2 * n).bit_length() - 1)) - 1,
            "r1": r1, "r2": r2, "low limb 0": (r1 >> BITS << BITS) % (2 * n), "low limb 1": (r2 >> BITS << BITS | 1) % (2 * n),
            "low limb ones": (r1 | MASK) % (2 * n)}


def test_squarings(mod):
    for name, a in operands(mod.n).items():
        mod.check(a)


def test_products(mod):
    ops = operands(mod.n)
    names = sorted(ops)
    for i, x in enumerate(names):                                 # every operand with a partner, both ways round
        y = names[(i + 3) % len(names)]
        mod.check(ops[x], ops[y])
        mod.check(ops[y], ops[x])


def test_first_row_quotient_digits(mod):
    """m = 0 and m = 2^29 - 1 in the first row of a product, m = 0 in the first row of a squaring: read back from the model."""
    ops = operands(mod.n)
    a0, a1, am = ops["low limb 0"], ops["low limb 1"], ops["low limb ones"]
    assert limbs(a0)[0] == 0 and limbs(a1)[0] == 1 and limbs(am)[0] == MASK
    assert (limbs(a0)[0] * limbs(am)[0]) & MASK == 0 and (limbs(a1)[0] * limbs(am)[0]) & MASK == MASK
    mod.check(a0, am)
    mod.check(am, a0)
    mod.check(a1, am)
    mod.check(am, a1)
    mod.check(a0)


def test_short_rows_count():
    """What the rows are for: 69 multiply-adds and three other instructions in the reduction half, no v_mul_lo_u32."""
    for sqr in (False, True):
        for step in gen.schedule29(S, sqr, short=True):
            if step[0] != "row" or step[2] == "any":
                continue
            ops = [line.split()[0] for line in step[3]]
            assert ops.count("v_mad_u64_u32") == S + S - 2 and "v_mul_lo_u32" not in ops
            assert len(ops) == 2 * S - 2 + 3


def test_committed_rows_are_the_generator_s():
    path = os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "gen", "mont29_rows.inc")
    assert open(path).read() == gen.render29([S])
