"""The catalogue of scalars for the curve powers under ONE scalar (csrc/ec_shared_schedule.h, k_ec_mulshared in
csrc/ec_kernels.h), shared by the host test of the schedule (tests/test_ec_shared_schedule_host.py) and the GPU test
(tests/test_gpu_ec_shared.py).  Over a group order q: the values at which the reduction modulo q, the recoding into signed odd
digits with its carry, and the schedule's first and last steps take another path."""
import random

WINDOWS = range(2, 7)
EC_DBL, EC_ADD = 6.9, 15.4                  # the prices the library books a doubling and an addition with (csrc/vmnhip.hip)


def extreme_digits(w):
    """A value whose width-w recoding holds the digits +(2^(w-1) - 1) and -(2^(w-1) - 1): D 2^k - D with D = 2^(w-1) - 1 and
    k = 2w + 3.  Modulo 2^w it is 2^w - D >= 2^(w-1), hence the digit -D and a carry; what remains is D 2^k."""
    D = (1 << (w - 1)) - 1
    return (D << (2 * w + 3)) - D


def catalogue(q):
    """[(name, scalar)] over the order q; the names are unique."""
    bits = q.bit_length()
    rnd = random.Random(bits * 1000003 + q % 1000003)
    out = [("0", 0), ("q", q), ("1", 1), ("2", 2), ("3", 3),
           ("q-1", q - 1), ("q+1", q + 1), ("q-2", q - 2), ("(q-1)/2", (q - 1) // 2), ("(q+1)/2", (q + 1) // 2)]
    for k in sorted({1, 200} | {w + d for w in WINDOWS for d in (-1, 0, 1)}):
        out += [("2^%d" % k, 1 << k), ("2^%d-1" % k, (1 << k) - 1)]
    out.append(("ones", (1 << (bits - 1)) - 1))                         # the carry runs to the top
    out += [("0x55", int("55" * 80, 16) % (1 << (bits - 1))), ("0xaa", int("aa" * 80, 16) % (1 << (bits - 1)))]
    out += [("extreme%d" % w, extreme_digits(w)) for w in WINDOWS]
    out.append(("320 bits", (1 << 319) | rnd.getrandbits(319)) if bits < 319 else ("wide", (q << 60) | rnd.getrandbits(60) | (1 << 59)))
    out += [("full%d" % i, rnd.randrange(1 << (bits - 1), q)) for i in range(4)]
    assert len({name for name, _ in out}) == len(out)
    return out


def cost(w, adds, dbls):
    """What a point costs under a schedule of `adds` additions and `dbls` doublings behind its first step, table included."""
    return EC_DBL * dbls + EC_ADD * (adds + (1 << (w - 2)) - 1) + (EC_DBL if w > 2 else 0)
