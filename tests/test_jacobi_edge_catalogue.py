"""The rows of tests/jacobi_edges.py are not vacuous: in every geometry the Jacobi kernels run in and under every modulus,
an integer model of the kernels' steps (jacobi_edges.model) takes the whole-limb shift, the longest possible run of them,
ctz = 27, both the subtraction and the swap and -- with several lanes per element -- a non-zero limb across every share
boundary; the model is the textbook symbol on every row; and two mutants of the model (never of a kernel) that random rows
cannot tell from it are caught.  No GPU: the kernels meet these rows in tests/test_gpu_jacobi_edges.py."""
import pytest

import jacobi_edges as je
from conftest import load_golden
from oracle import pyref

CASES = [(geo.id, name) for geo in je.GEOMETRIES for name in je.moduli(geo)]
MULTI_LANE = [geo.id for geo in je.GEOMETRIES if geo.LPE > 1]
RANDOM_UP_TO = 4096                                     # the mutants against 300 random rows: every size up to here

_cache = {}


def findings(geo_id, name):
    """The catalogue of one geometry and modulus with its textbook symbols and the model's results, computed once."""
    if (geo_id, name) not in _cache:
        geo = je.GEOMETRY[geo_id]
        N = je.modulus(geo, name)
        rows = je.catalogue(N, geo)
        _cache[(geo_id, name)] = (geo, N, rows, [je.jacobi(v, N) for v in rows], [je.model(v, N, geo) for v in rows])
    return _cache[(geo_id, name)]


def miller_rabin(n):
    """n is prime: trial division by and Miller-Rabin to 24 prime bases (a composite passes one base in four at most), on
    Python's pow."""
    bases = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89)
    if n < 2:
        return False
    for b in bases:
        if n % b == 0:
            return n == b
    d, s = n - 1, 0
    while d % 2 == 0:
        d //= 2
        s += 1
    for b in bases:
        x = pow(b, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def test_geometries_and_moduli():
    """One geometry per size, the group's own (vmn_garray_is_member: with_cfg on the group's modulus); every modulus is odd,
    of exactly `bits` bits, and the four of them are 7, 1, 3 and 5 mod 8."""
    assert [(g.bits, g.S, g.LPE) for g in je.GEOMETRIES] == [(256, 10, 1), (384, 14, 1), (512, 19, 1), (1024, 37, 1), (2048, 74, 1),
                                                            (3072, 110, 2), (4096, 148, 4), (8192, 296, 8), (16384, 592, 16)]
    for geo in je.GEOMETRIES:
        assert geo.rows == geo.S and geo.S % geo.LPE == 0
        ms = je.moduli(geo)
        assert set(ms) == (set(je.MODULI) if geo.bits < 16384 else {"ones", "rnd3", "rnd5"})
        for name, N in ms.items():
            assert N.bit_length() == geo.bits and N % 8 == {"ones": 7, "hi": 1, "rnd3": 3, "rnd5": 5}[name]


@pytest.mark.parametrize("geo_id,name", CASES)
def test_catalogue_rows_and_their_preimages(geo_id, name):
    geo, N, rows, _, _ = findings(geo_id, name)
    assert rows == je.catalogue(N, geo) and len(set(rows)) == len(rows)
    assert all(0 < v < N for v in rows)
    assert 50 <= len(rows) <= je.LARGE_LIMIT.get(geo.bits, 1200), len(rows)
    R = 1 << (je.LIMB * geo.rows)
    pre = je.preimages(rows, N, geo)
    assert all(0 < x < N for x in pre) and [x * R % N for x in pre] == rows
    need = {1, 2, N - 1, (N - 1) // 2, 1 << 27, 1 << (je.LIMB * je.top_limb(geo.bits))}
    if geo.bits < je.LARGE:
        need |= {3, 4, N - 2, N - 4, (N + 1) // 2} | {1 << k for k in range(1, 29)} | {N - (1 << k) for k in (1, 27, 28, 56)}
        need |= {1 << (je.LIMB * j) for j in range(1, je.top_limb(geo.bits) + 1)}
        need |= {N - (1 << (je.LIMB * j)) for j in range(1, je.top_limb(geo.bits) + 1)}
    for _, (below, at, above) in je.boundary_positions(geo):
        need.add(1 << (je.LIMB * at))
        assert any(v % (1 << (je.LIMB * below)) == 0 and (v >> (je.LIMB * below)) & 1 for v in rows), below
        assert N - (1 << (je.LIMB * above)) in rows
    assert need <= set(rows)
    for f in je.small_factors(N):
        assert f in rows
        assert geo.bits >= je.LARGE or {f << je.LIMB, N // f} <= set(rows)


@pytest.mark.parametrize("geo_id,name", CASES)
def test_model_is_the_textbook_symbol(geo_id, name):
    geo, N, rows, ref, got = findings(geo_id, name)
    wrong = [hex(v) for v, r, (s, _) in zip(rows, ref, got) if s != r]
    assert not wrong, wrong[:3]
    if name in ("rnd3", "rnd5"):
        assert {-1, 1} <= set(ref)
    if je.small_factors(N):
        assert set(ref) == {-1, 0, 1}
    assert name != "ones" or je.small_factors(N), "2^bits - 1 has the factor 3"


@pytest.mark.parametrize("geo_id,name", CASES)
def test_catalogue_reaches_every_branch(geo_id, name):
    geo, N, rows, _, got = findings(geo_id, name)
    counts = [c for _, c in got]
    L = je.limbs_per_lane(geo)
    assert sum(c.limb_shifts for c in counts) >= 1
    longest = max(c.longest_run for c in counts)
    # a row below N < 2^bits has at most (bits - 1) // 28 zero limbs under its lowest set bit: S - 1 of them wherever
    # 28 (S - 1) < bits, which is every size but 4096 bits (28 * 147 = 4116) and the two above it
    most = min(geo.S - 1, je.top_limb(geo.bits))
    assert most == geo.S - 1 or geo.bits >= 4096
    assert longest == most and (geo.LPE == 1 or most >= L)
    assert max(c.max_ctz for c in counts) == 27
    assert sum(c.subtractions for c in counts) >= 1 and sum(c.swaps for c in counts) >= 1
    for h in range(1, geo.LPE):
        assert sum(c.crossings[h] for c in counts) >= 1, "no non-zero limb crosses the share boundary %d" % h
    if geo.LPE > 1:                                     # and the top lane holds a live limb while the element shifts
        assert sum(c.top_share_live for c in counts) >= 1


def first_caught(geo, N, rows, ref, mutant):
    return next((v for v, r in zip(rows, ref) if je.model(v, N, geo, mutant)[0] != r), None)


@pytest.mark.parametrize("geo_id,name", [c for c in CASES if c[0] in MULTI_LANE])
def test_catalogue_catches_a_lost_limb_from_the_share_above(geo_id, name):
    """Mutant (a) of the MODEL: the limb shift drops the limb that arrives from the share above."""
    geo, N, rows, ref, _ = findings(geo_id, name)
    assert first_caught(geo, N, rows, ref, je.DROP_FROM_ABOVE) is not None


@pytest.mark.parametrize("geo_id", [g.id for g in je.GEOMETRIES])
@pytest.mark.parametrize("name", ["rnd3", "rnd5"])
def test_catalogue_catches_a_sign_flip_on_the_limb_shift(geo_id, name):
    """Mutant (b) of the MODEL: the limb shift flips the sign when m mod 8 is 3 or 5 (28 twos are an even count: it must not)."""
    geo, N, rows, ref, _ = findings(geo_id, name)
    assert first_caught(geo, N, rows, ref, je.FLIP_ON_LIMB_SHIFT) is not None


@pytest.mark.parametrize("geo_id", [g.id for g in je.GEOMETRIES if g.bits <= RANDOM_UP_TO])
def test_random_rows_catch_neither_mutant(geo_id):
    """300 seeded random rows take no limb shift, so both mutants pass them: why the catalogue exists."""
    geo = je.GEOMETRY[geo_id]
    for name in ("rnd3", "rnd5"):
        N = je.modulus(geo, name)
        rows = je.random_rows(N, geo, 300, name.encode())
        ref = [je.jacobi(v, N) for v in rows]
        assert len(rows) >= 299 and {-1, 1} <= set(ref)
        assert first_caught(geo, N, rows, ref, je.FLIP_ON_LIMB_SHIFT) is None
        if geo.LPE > 1 and name == "rnd3":
            assert first_caught(geo, N, rows, ref, je.DROP_FROM_ABOVE) is None


def test_random_2048_bit_rows_never_shift_a_whole_limb():
    """3000 seeded random rows under the golden 2048-bit prime: no limb shift at all, and no ctz of 27."""
    geo = je.GEOMETRY["2048"]
    p = load_golden(2048)[0]["p"]
    rows = je.random_rows(p, geo, 3000, b"golden")
    counts = [je.model(v, p, geo)[1] for v in rows]
    assert len(rows) == 3000
    assert sum(c.limb_shifts for c in counts) == 0
    assert max(c.max_ctz for c in counts) < 27
    assert sum(c.subtractions for c in counts) > 0 and sum(c.swaps for c in counts) > 0


# ---- prime moduli: the second reference x^q = 1 --------------------------------------------------------------------------
@pytest.mark.parametrize("bits", sorted(je.SAFE_PRIMES_3_MOD_8))
def test_safe_primes_that_are_3_mod_8(bits):
    p = je.SAFE_PRIMES_3_MOD_8[bits]
    q = (p - 1) // 2
    assert p.bit_length() == bits and p % 8 == 3 and 2 * q + 1 == p
    assert miller_rabin(p) and miller_rabin(q)
    assert not miller_rabin(p * q) and not miller_rabin((1 << bits) - 1)      # (and the test does reject composites)
    geo = je.GEOMETRY[str(bits)]
    rows = je.catalogue(p, geo)
    pre = je.preimages(rows, p, geo)
    verdicts = set()
    for v, x in zip(rows, pre):
        sym, _ = je.model(v, p, geo)
        assert sym == je.jacobi(v, p) == je.jacobi(x, p) and sym != 0
        assert (sym == 1) == (pow(x, q, p) == 1) == (pow(v, q, p) == 1)
        verdicts.add(sym)
    assert verdicts == {-1, 1}
    assert je.jacobi(2, p) == -1 and je.jacobi(4, p) == 1   # (2 / p) = -1 for p = 3 mod 8


@pytest.mark.parametrize("bits", [512, 1024, 2048, 3072, 4096, 6144, 8192])
def test_known_primes_are_7_mod_8_and_agree_with_the_power(bits):
    """The golden groups and the RFC 3526 groups: all 7 mod 8, and symbol 1 <=> x^q = 1 on catalogue rows."""
    p = load_golden(bits)[0]["p"] if bits <= 4096 else pyref.modp_group(bits)[0]
    q = (p - 1) // 2
    assert p % 8 == 7
    geo = next(g for g in je.GEOMETRIES if p.bit_length() <= g.bits)
    rows = je.catalogue(p, geo)[:40 if bits <= 2048 else 6 if bits <= 4096 else 2]
    for v in rows:
        sym = je.jacobi(v, p)
        assert je.model(v, p, geo)[0] == sym
        assert (sym == 1) == (pow(v, q, p) == 1)
