"""Rows for the Jacobi membership kernels (csrc/modp_kernels.h: k_jacobi_member, k_jacobi_member_lanes): the limbs at which
the binary algorithm leaves its common path -- a whole zero limb (the limb shift), ctz up to 27, the limb pulled from the
share above -- under moduli that are 1, 3, 5 and 7 mod 8, composite ones among them (symbol 0).  Shared by
tests/test_jacobi_edge_catalogue.py (the catalogue reaches every branch of an integer model of the kernels' steps, and that
model is the textbook symbol; no GPU) and tests/test_gpu_jacobi_edges.py (the kernels against the textbook symbol).

The kernels see x R mod N (R = 2^(28 rows)), not x: catalogue() gives DEVICE ROWS v, preimages() the values x = v / R mod N
to feed so that the kernel finds v's limbs in its registers.  (R / N) = 1 -- R is an even power of two -- so the symbol of
the row is the symbol of x."""
from collections import namedtuple

from oracle import pyref
from ring_edges import GEOMETRIES as RING_GEOMETRIES, LIMB, LIMB_MASK, limbs_per_lane, seeded_odd

# The geometry vmn_garray_is_member runs in is the group's own (with_cfg on the group's modulus: no choice by size), one per
# size: k_jacobi_member for LPE = 1, k_jacobi_member_lanes above.
GEOMETRIES = [g._replace(id=str(g.bits)) for g in RING_GEOMETRIES if g.S == g.rows]
GEOMETRY = {g.id: g for g in GEOMETRIES}
MODULI = ("ones", "hi", "rnd3", "rnd5")
FACTORS = (3, 5, 7, (1 << 32) - 1)
LARGE = 8192                                            # from here on the catalogue is cut: LARGE_LIMIT values per modulus
LARGE_LIMIT = {8192: 100, 16384: 60}

# Safe primes p = 2q + 1 with p = 3 mod 8 (every golden and RFC 3526 modulus is 7 mod 8), found once by a sieve and
# Miller-Rabin; tests/test_jacobi_edge_catalogue.py proves p and q prime.
SAFE_PRIMES_3_MOD_8 = {
    256: 0xe2c0b5b6805ab69005f66bf0f2bfa2b8973a75baaa90128deff3607478ba5623,
    512: 0xdfbb628c73824a6cebac8180cb13637efc28c73d640276cb5597e89625f68e7dedbd31a7e56a32fc2da96aa16ff10d2f9d5e420bff448fc30dff3aa3acfa848b,
}


def jacobi(a, n):
    """The textbook Jacobi symbol (a / n), n odd and positive, by division with remainder (Euclid's steps, no limbs):
    1, -1, or 0 when gcd(a, n) > 1."""
    a %= n
    t = 1
    while a:
        twos = (a & -a).bit_length() - 1                # (2 / n) = -1 iff n = 3, 5 mod 8, once per factor of two
        a >>= twos
        if twos % 2 and n % 8 in (3, 5):
            t = -t
        a, n = n, a
        if a % 4 == 3 and n % 4 == 3:
            t = -t
        a %= n
    return t if n == 1 else 0


def modulus(geo, name):
    """An odd N of exactly geo.bits bits: all ones (7 mod 8, small factors), the top bit and one (1 mod 8), and two seeded
    values that end in 011 and 101."""
    bits = geo.bits
    if name == "ones":
        return (1 << bits) - 1
    if name == "hi":
        return (1 << (bits - 1)) + 1
    if name == "rnd3":
        return seeded_odd(b"jacobi-edges/N3/%d" % bits, bits) & ~7 | 3
    if name == "rnd5":
        return seeded_odd(b"jacobi-edges/N5/%d" % bits, bits) & ~7 | 5
    raise KeyError(name)


def moduli(geo):
    """{name: N}.  At 16384 bits the textbook symbol costs ~45 ms a value: all ones, and one each of 3 and 5 mod 8."""
    names = ("ones", "rnd3", "rnd5") if geo.bits >= 16384 else MODULI
    return {name: modulus(geo, name) for name in names}


def top_limb(bits):
    """The largest j with 2^(28 j) below every modulus of `bits` bits: no row has more zero limbs under its lowest set bit."""
    return (bits - 1) // LIMB


def boundary_positions(geo):
    """[(h, (hL - 1, hL, hL + 1))] for every share boundary h."""
    L = limbs_per_lane(geo)
    return [(h, (h * L - 1, h * L, h * L + 1)) for h in range(1, geo.LPE)]


def small_factors(N):
    return [f for f in FACTORS if N % f == 0 and f < N]


def catalogue(N, geo):
    """Device rows v, 0 < v < N, in a fixed order, each once.  Below 8192 bits every limb position; from there on the
    share boundaries first, then what the branch conditions need, then the rest, cut at LARGE_LIMIT."""
    bits = geo.bits
    jtop = top_limb(bits)
    rnd = iter(pyref.stream_ints(b"jacobi-edges/v/%d/%x" % (bits, N & 0xffffffff), geo.S + 64 if bits < LARGE else 96, N))

    def odd_multiple(shift):                            # an odd value with random high limbs, `shift` zero bits below it
        return ((next(rnd) >> shift) | 1) << shift

    def at_limb(j):
        b = 1 << (LIMB * j)
        return [b, 3 * b, b - 1, b + 1, N - b, odd_multiple(LIMB * j)]

    def at_bit(k):
        return [1 << k, N - (1 << k), odd_multiple(k)]

    base = [1, 2, 3, 4, N - 1, N - 2, N - 4, (N - 1) // 2, (N + 1) // 2]
    fs = small_factors(N)
    ks = list(range(1, 29)) + [55, 56, 57]
    if bits < LARGE:
        vs = list(base)
        for j in range(1, geo.S):
            vs += at_limb(j)
        for k in ks:
            vs += at_bit(k)
        for f in fs:
            vs += [f, f << LIMB, N // f]
        vs += [next(rnd) for _ in range(16)]
        limit = None
    else:
        first, second = [], []
        for _, (below, at, above) in boundary_positions(geo):
            first += [odd_multiple(LIMB * below), 1 << (LIMB * at), N - (1 << (LIMB * above))]
            second += [1 << (LIMB * below), N - (1 << (LIMB * at)), 3 << (LIMB * at), (1 << (LIMB * above)) + 1]
        need = [1 << 27, 1 << (LIMB * jtop), 1, 2, N - 1, (N - 1) // 2, odd_multiple(27)] + fs + [next(rnd), next(rnd)]
        rest = base + [v for j in (1, 2, 3, jtop) for v in at_limb(j)] + [v for k in (1, 28, 55, 56, 57) for v in at_bit(k)]
        rest += [v for f in fs for v in (f << LIMB, N // f)] + [next(rnd) for _ in range(14)]
        vs = first + need + second + rest
        limit = LARGE_LIMIT[bits]
    seen, out = set(), []
    for v in vs:
        if 0 < v < N and v not in seen:
            seen.add(v)
            out.append(v)
    return out[:limit]


def preimages(rows, N, geo):
    """v / R mod N, R = 2^(28 rows): the values whose device (Montgomery) form is exactly v (N is odd: R has an
    inverse)."""
    rinv = pow(1 << (LIMB * geo.rows), -1, N)
    return [v * rinv % N for v in rows]


def random_rows(N, geo, count, tag=b""):
    """`count` seeded random rows below N: what the device finds for arbitrary inputs."""
    return [v for v in pyref.stream_ints(b"jacobi-edges/random/%d/%s" % (geo.bits, tag), count, N) if v]


# ---- the integer model of the kernels' steps ----------------------------------------------------------------------------
Counts = namedtuple("Counts", "limb_shifts crossings longest_run max_ctz subtractions swaps top_share_live")
DROP_FROM_ABOVE = "drop-from-above"                     # mutant (a): the limb shift loses the limb that comes from the share above
FLIP_ON_LIMB_SHIFT = "flip-on-limb-shift"               # mutant (b): the limb shift flips the sign when m is 3 or 5 mod 8


def model(v, N, geo, mutant=None):
    """(symbol, Counts) of the row v under N by the steps of k_jacobi_member / k_jacobi_member_lanes on Python integers:
    a zero low limb shifts the element down by one limb (each share's top limb comes from the share above), else the twos
    of the low limb go (ctz <= 27, sign by m mod 8), then a >= m subtracts and a < m swaps to (m - a, a) by reciprocity.
    crossings[h] = limb shifts that carry a non-zero limb from share h into share h - 1.  top_share_live = limb shifts with
    a non-zero low limb in the top share (the lane whose own or neighbour's limb nottopmask keeps out).  The loop is
    bounded at 8 * bits steps: symbol None if it does not end (a mutant may not)."""
    L, LPE = limbs_per_lane(geo), geo.LPE
    keep = ~sum(LIMB_MASK << (LIMB * (h * L - 1)) for h in range(1, LPE))
    a, m, t = v, N, 0
    limb_shifts = longest = run = max_ctz = subs = swaps = top_live = 0
    crossings = {h: 0 for h in range(1, LPE)}
    steps, bound = 0, 8 * geo.bits
    assert 0 <= v < N and N & 1
    while a:
        steps += 1
        if steps > bound:
            return None, Counts(limb_shifts, crossings, longest, max_ctz, subs, swaps, top_live)
        low = a & LIMB_MASK
        if low == 0:
            limb_shifts += 1
            run += 1
            longest = max(longest, run)
            for h in range(1, LPE):
                if (a >> (LIMB * h * L)) & LIMB_MASK:
                    crossings[h] += 1
            if LPE > 1 and (a >> (LIMB * (LPE - 1) * L)) & LIMB_MASK:
                top_live += 1
            a >>= LIMB
            if mutant == DROP_FROM_ABOVE:
                a &= keep
            if mutant == FLIP_ON_LIMB_SHIFT and m & 7 in (3, 5):
                t ^= 1
            continue
        run = 0
        k = (low & -low).bit_length() - 1
        if k:
            max_ctz = max(max_ctz, k)
            if k & 1 and m & 7 in (3, 5):
                t ^= 1
            a >>= k
        if a >= m:
            subs += 1
            a -= m
        else:
            swaps += 1
            if a & 3 == 3 and m & 3 == 3:
                t ^= 1
            a, m = m - a, a
    symbol = 0 if (v == 0 or m != 1) else (-1 if t else 1)
    return symbol, Counts(limb_shifts, crossings, longest, max_ctz, subs, swaps, top_live)
