"""GPU suite: the Jacobi membership kernels (csrc/modp_kernels.h: k_jacobi_member, k_jacobi_member_lanes) on the limbs they
really see, against the textbook symbol on Python integers (jacobi_edges.jacobi).  An element is a member when its symbol
is 1.

An array lives on the device in Montgomery form, so a plain 1 << 28 reaches the kernel as a random-looking row.  The rows
come from tests/jacobi_edges.py and are fed as their preimages v / R mod N: the kernel then finds v itself in its registers.
What that reaches, per kernel, that random rows and plain special values do not (tests/test_jacobi_edge_catalogue.py counts
each on an integer model of the kernels' steps, for the very rows used here):

  k_jacobi_member (256 to 2048 bits, one lane per element)
    - the whole-limb shift `if (low == 0)`: runs of 1 to S - 1 zero limbs, at the first step and -- N - 2^(28 j) -- after a swap;
    - ctz = 26 and 27 (random rows stop at about 25);
    - the symbol 0: composite moduli (2^bits - 1 and two seeded ones), rows that share a factor with them: m does not end at 1;
    - a modulus that is 3 mod 8, composite and prime, so that (2 / m) = -1 holds for the modulus the kernel starts from.
  k_jacobi_member_lanes (3072 to 16384 bits, 2 / 4 / 8 / 16 lanes per element)
    - all of the above, runs of up to (bits - 1) // 28 zero limbs;
    - `a[L - 1] = up`: a non-zero limb crosses every share boundary in a limb shift (from_above in all three DPP forms);
    - `& ln.nottopmask` in the limb shift: the top lane holds a non-zero low limb while the element shifts, so its own
      (two and four lanes) or the next element's (eight and sixteen) low limb would enter above the element without the mask;
    - elements on the limb-shift path next to ordinary ones in one wave, the cross-lane moves inside the divergent loop.

Moduli that are 1 and 5 mod 8 do NOT reach these kernels as the starting modulus: the dispatch asks for 2q = N - 1 and the
group for an odd q, so N = 3 mod 4.  `hi` and `rnd5` of jacobi_edges are therefore refused when the group is made (asserted
below); m takes those residues after the swaps only, which the integer model covers on the CPU under all four moduli.

Zero: k_import_be reports a zero row (flag 2) without replacing it -- only values >= N become 1 -- so a zero can enter a
group array, in range; the kernels call it a non-member (zero_in)."""
import random

import pytest

import jacobi_edges as je
from conftest import load_golden
from test_gpu_schedules import launches, witness

pytestmark = pytest.mark.gpu

CASES = [(geo.id, name) for geo in je.GEOMETRIES for name, N in je.moduli(geo).items() if N % 4 == 3]
REFUSED = [(geo.id, name) for geo in je.GEOMETRIES for name in je.MODULI if je.modulus(geo, name) % 4 == 1]
PRIMES = ["256-3mod8", "512-3mod8", "1024-golden"]


class Case:
    """One geometry and modulus N (q = (N - 1) / 2): the group, the catalogue's rows v, the values x = v / R whose device
    row is v, and the textbook symbols (v / N) = (x / N)."""

    def __init__(self, vmn, gpu_ctx, geo, N):
        self.ctx, self.geo, self.N = gpu_ctx, geo, N
        self.nb = geo.bits // 8
        self.rows = je.catalogue(N, geo)
        self.pre = je.preimages(self.rows, N, geo)
        self.sym = [je.jacobi(v, N) for v in self.rows]
        self.G = vmn.ModPGroup(gpu_ctx, N, (N - 1) // 2, 3, nbytes=self.nb)
        self.members = [x for x, s in zip(self.pre, self.sym) if s == 1]
        self.others = [(x, s) for x, s in zip(self.pre, self.sym) if s != 1]
        # a member whose row starts with a zero limb: it takes the limb shift at its first step
        self.shifter = next(x for x, v, s in zip(self.pre, self.rows, self.sym) if s == 1 and v & je.LIMB_MASK == 0)
        self.epb = 256 // geo.LPE                           # C::EPB: elements per workgroup

    def enc(self, values):
        return b"".join(x.to_bytes(self.nb, "big") for x in values)

    def verdict(self, values):
        """isMember() of the array of `values` (ints, or their big-endian block)."""
        arr = self.G.toElementArray(values if isinstance(values, bytes) else self.enc(values))
        try:
            return arr.isMember()
        finally:
            arr.free()

    def close(self):
        self.G.close()


def make_case(request, vmn, gpu_ctx, geo, N):
    c = Case(vmn, gpu_ctx, geo, N)
    request.addfinalizer(c.close)
    return c


@pytest.fixture(scope="module", params=CASES, ids=["%s-%s" % c for c in CASES])
def case(request, vmn, gpu_ctx):
    geo = je.GEOMETRY[request.param[0]]
    return make_case(request, vmn, gpu_ctx, geo, je.modulus(geo, request.param[1]))


@pytest.fixture(scope="module", params=PRIMES)
def prime_case(request, vmn, gpu_ctx):
    bits = int(request.param.split("-")[0])
    p = load_golden(bits)[0]["p"] if request.param.endswith("golden") else je.SAFE_PRIMES_3_MOD_8[bits]
    assert p.bit_length() == bits
    return make_case(request, vmn, gpu_ctx, je.GEOMETRY[str(bits)], p)


# ---- every row alone ----------------------------------------------------------------------------------------------------
def alone(case, values):
    """Each value in an array of its own: the verdict is (v / N) = 1.  Witness: one launch of the Jacobi kernel per
    verdict, none of the power."""
    with launches(case.ctx) as got:
        assert case.verdict([values[0]]) is (case.sym[0] == 1)
    witness(got, {"member": 1, "modpow": 0}, "the Jacobi symbol")
    with launches(case.ctx) as got:
        for v, x, s in zip(case.rows, values, case.sym):
            assert case.verdict([x]) is (s == 1), (hex(v), s)
    witness(got, {"member": len(case.rows), "modpow": 0}, "the Jacobi symbol")


def test_every_catalogue_row_alone(case):
    """The preimage x = v / R of every row v: the kernel finds v itself."""
    assert {-1, 1} <= set(case.sym) and (0 in case.sym or not je.small_factors(case.N))
    alone(case, case.pre)


def test_every_catalogue_value_alone(case):
    """v itself as a value: the kernel finds v R mod N, and (v R / N) = (v / N), R being a square."""
    alone(case, case.rows)


# ---- mixed waves --------------------------------------------------------------------------------------------------------
def test_members_and_one_non_member_in_one_array(case):
    """All members in catalogue order: rows on the limb-shift path and ordinary rows share their waves.  Then each
    non-member (symbol -1 and symbol 0) inserted first, in the middle, last."""
    members = case.members
    assert len(members) >= 10 and case.shifter in members
    assert case.verdict(members) is True
    others = case.others
    if case.geo.bits >= je.LARGE:                           # a seeded sample of 12, one of symbol 0 where there is one
        zeros = [o for o in others if o[1] == 0]
        sample = random.Random(case.geo.bits).sample(others, 12)
        if zeros and not any(s == 0 for _, s in sample):
            sample[0] = zeros[0]
        others = sample
        assert len(others) == 12 and (not zeros or any(s == 0 for _, s in others))
    blocks = [x.to_bytes(case.nb, "big") for x in members]
    for i, (x, s) in enumerate(others):
        pos = (0, len(members) // 2, len(members))[i % 3]
        blk = b"".join(blocks[:pos]) + x.to_bytes(case.nb, "big") + b"".join(blocks[pos:])
        assert case.verdict(blk) is False, (hex(x), s, pos)


# ---- array lengths around a workgroup -----------------------------------------------------------------------------------
def test_array_lengths_around_a_workgroup(case):
    """E = 256 / LPE elements per workgroup.  Members at lengths E - 1, E, E + 1; one non-member last (at E + 1 alone in the
    next workgroup, at E - 1 recomputed by the dead lanes); the non-member first and a limb-shift member last."""
    E = case.epb
    bad = case.others[0][0]
    assert case.others[0][1] == -1 or je.small_factors(case.N)
    for n in (E - 1, E, E + 1):
        ms = (case.members * (n // len(case.members) + 1))[:n]
        assert len(ms) == n
        assert case.verdict(ms) is True, n
        assert case.verdict(ms[:-1] + [bad]) is False, n
        assert case.verdict([bad] + ms[1:-1] + [case.shifter]) is False, n
        assert case.verdict(ms[:-1] + [case.shifter]) is True, n


def test_zero_is_in_range_and_no_member(case):
    arr = case.G.toElementArray([0], checked=False)
    assert arr.all_in_range is True and arr.toInts() == [0]
    assert arr.isMember() is False
    arr.free()
    assert case.verdict(case.members[:5] + [0]) is False
    assert case.verdict([0] + case.members[:5]) is False


# ---- what cannot reach the kernels --------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo_id,name", REFUSED, ids=["%s-%s" % c for c in REFUSED])
def test_moduli_that_are_1_mod_4_have_no_group(geo_id, name, vmn, gpu_ctx):
    """N = 1, 5 mod 8: q = (N - 1) / 2 is even, and an even order is refused (Montgomery arithmetic mod q)."""
    geo = je.GEOMETRY[geo_id]
    N = je.modulus(geo, name)
    assert N % 8 in (1, 5) and ((N - 1) // 2) % 2 == 0
    with pytest.raises(vmn.VmnError):
        vmn.ModPGroup(gpu_ctx, N, (N - 1) // 2, 3, nbytes=geo.bits // 8)


# ---- safe primes: the symbol against x^q = 1, the Jacobi kernels against the power kernels --------------------------------
def test_safe_primes_by_symbol_and_by_power(prime_case, monkeypatch):
    """Two safe primes that are 3 mod 8 and the golden 1024-bit one (7 mod 8): the catalogue's preimages one by one, by
    the Jacobi kernel and by x^q = 1 on the device (VMN_MEMBER_BY_POWER=1), both equal to pow(x, q, p) == 1."""
    c = prime_case
    p, q = c.N, (c.N - 1) // 2
    want = [pow(x, q, p) == 1 for x in c.pre]
    assert want == [s == 1 for s in c.sym] and set(want) == {True, False}
    monkeypatch.delenv("VMN_MEMBER_BY_POWER", raising=False)
    with launches(c.ctx) as got:
        by_symbol = [c.verdict([x]) for x in c.pre]
    witness(got, {"member": len(c.pre), "modpow": 0}, "the Jacobi symbol")
    monkeypatch.setenv("VMN_MEMBER_BY_POWER", "1")
    with launches(c.ctx) as got:
        by_power = [c.verdict([x]) for x in c.pre]
    witness(got, {"member": 0}, "VMN_MEMBER_BY_POWER")
    assert got.get("modpow", 0) >= len(c.pre)
    monkeypatch.delenv("VMN_MEMBER_BY_POWER", raising=False)
    assert by_symbol == want
    assert by_power == want
    if p % 8 == 3:                                          # (2 / p) = -1
        assert c.verdict([2]) is False and c.verdict([4]) is True
        assert c.verdict([4, 2]) is False
    assert c.verdict(c.members) is True
    assert c.verdict(c.members + [c.others[0][0]]) is False
