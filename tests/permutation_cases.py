"""The rule of a prover's secret permutation (csrc/permutation_layout.h, [NOT-IN-REF: VCR Permutation.random; unpinned]) restated on
Python integers, and the catalogue the CPU harness and the GPU tests share.

    kb = rbitlen + 2 ceil(log2(max(n, 2))),  key_bytes = ceil(kb / 8)
    key_i = the i-th key_bytes bytes of PRG(seed), big-endian, superfluous leading bits cleared (oracle.pyref_prg.random_integers)
    pi = the indices in the order (key_i, i);  inv[pi[j]] = j
"""
import hashlib

from oracle import pyref_prg

HASH_OF_SEEDLEN = {32: "sha256", 48: "sha384", 64: "sha512"}

# the sort's tile (csrc/permutation_kernels.h: SORT_TILE) and a wave's piece of it
TILE, WAVE_PIECE = 4096, 1024

SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65537, 300001)
RBITLENS = (0, 100, 256)
KEY_BYTES = (1, 4, 5, 8, 9, 18, 32, 64)


def ceil_log2(m: int) -> int:
    return (m - 1).bit_length()


def key_bits(n: int, rbitlen: int) -> int:
    return rbitlen + 2 * ceil_log2(max(n, 2))


def key_bytes(n: int, rbitlen: int) -> int:
    return (key_bits(n, rbitlen) + 7) // 8


def seed_of(tag: bytes, seedlen: int = 32) -> bytes:
    return hashlib.sha512(b"permutation/" + tag).digest()[:seedlen]


def keys_of(seed: bytes, n: int, rbitlen: int, hashname: str = "sha256"):
    """The n keys as integers."""
    kb = key_bits(n, rbitlen)
    if hashname == "sha256":
        return pyref_prg.random_integers(seed, n, kb)
    vb = (kb + 7) // 8                                  # the same convention over the other two hashes
    stream = pyref_prg.prg_bytes(seed, n * vb, hashname)
    return [int.from_bytes(stream[i * vb:(i + 1) * vb], "big") & ((1 << kb) - 1) for i in range(n)]


def key_rows(seed: bytes, n: int, rbitlen: int, hashname: str = "sha256"):
    """The n keys as a numpy array (n, key_bytes) of bytes, big-endian (no per-element Python work: the large cases)."""
    import numpy as np
    kb, vb = key_bits(n, rbitlen), key_bytes(n, rbitlen)
    rows = np.frombuffer(pyref_prg.prg_bytes(seed, n * vb, hashname), dtype=np.uint8).reshape(n, vb).copy()
    if kb % 8 and n:
        rows[:, 0] &= (1 << (kb % 8)) - 1
    return rows


def lexsort_rows(rows):
    """The order (key, index) of big-endian key rows, by numpy: (pi, inv) as uint32."""
    import numpy as np
    n, vb = rows.shape
    # lexsort sorts by the LAST key first: index is the least significant, byte 0 the most
    pi = np.lexsort([np.arange(n)] + [rows[:, k] for k in range(vb - 1, -1, -1)]).astype(np.uint32) if n else np.empty(0, dtype=np.uint32)
    inv = np.empty(n, dtype=np.uint32)
    inv[pi] = np.arange(n, dtype=np.uint32)
    return pi, inv


def restate(seed: bytes, n: int, rbitlen: int, hashname: str = "sha256"):
    """pi as a list, the rule word for word."""
    keys = keys_of(seed, n, rbitlen, hashname)
    return sorted(range(n), key=lambda i: (keys[i], i))


def restate_large(seed: bytes, n: int, rbitlen: int, hashname: str = "sha256"):
    """(pi, inv) as numpy arrays: lexsort on the key bytes plus the index."""
    return lexsort_rows(key_rows(seed, n, rbitlen, hashname))


def by_insertion(keys):
    """A second, independent statement: insertion by comparison (i goes in front of the first j with a larger key, or an
    equal key and a larger index)."""
    order = []
    for i, k in enumerate(keys):
        at = len(order)
        for pos, j in enumerate(order):
            if keys[j] > k or (keys[j] == k and j > i):
                at = pos
                break
        order.insert(at, i)
    return order


# ---- crafted keys for vmn_permutation_from_keys: name -> f(n, key_bytes) -> numpy (n, key_bytes) of bytes -------------------------
def _np():
    import numpy as np
    return np


def crafted_all_equal(n, vb):
    return _np().full((n, vb), 0xA7, dtype=_np().uint8)


def crafted_two_values(n, vb):
    rows = _np().full((n, vb), 0x11, dtype=_np().uint8)
    rows[::2] = 0xEE                                   # the larger value first: every second key moves behind the others
    return rows


def crafted_last_byte(n, vb):
    rows = _np().full((n, vb), 0x5C, dtype=_np().uint8)
    rows[:, vb - 1] = (_np().arange(n) * 37 + 11) % 251
    return rows


def crafted_first_byte(n, vb):
    rows = _np().full((n, vb), 0x5C, dtype=_np().uint8)
    rows[:, 0] = (_np().arange(n) * 91 + 5) % 253
    return rows


def _counter_rows(values, vb):
    """values (uint64) as big-endian rows of vb bytes (the low min(vb, 8) bytes of each value, the rest zero)."""
    np = _np()
    rows = np.zeros((len(values), vb), dtype=np.uint8)
    for k in range(min(vb, 8)):
        rows[:, vb - 1 - k] = (values >> np.uint64(8 * k)) & np.uint64(0xFF)
    return rows


def crafted_sorted(n, vb):
    """Non-decreasing keys: i itself on two bytes and more (n < 2^16), floor(256 i / n) on one byte (ties in runs)."""
    np = _np()
    assert n < 1 << 16
    i = np.arange(n, dtype=np.uint64)
    return _counter_rows(i if vb > 1 else i * np.uint64(256) // np.uint64(max(n, 1)), vb)


def crafted_reversed(n, vb):
    return crafted_sorted(n, vb)[::-1].copy()


def crafted_runs(n, vb):
    """Runs of equal keys whose ends straddle the boundaries of a wave's piece and of a tile: run r covers the positions
    [cuts[r], cuts[r + 1]) and holds the value (r * 5) % 7, so that equal values also meet again in later tiles."""
    np = _np()
    cuts = sorted({0, n} | {c for b in (WAVE_PIECE, TILE, 2 * TILE, 3 * TILE - WAVE_PIECE) for c in (b - 3, b + 2) if 0 < c < n}
                  | {c for c in (61, 67, 700) if c < n})
    rows = np.zeros((n, vb), dtype=np.uint8)
    for r in range(len(cuts) - 1):
        rows[cuts[r]:cuts[r + 1], vb - 1] = (r * 5) % 7
    return rows


def crafted_seven_values(n, vb):
    np = _np()
    pick = np.frombuffer(pyref_prg.prg_bytes(seed_of(b"seven"), n), dtype=np.uint8) % 7
    table = np.frombuffer(pyref_prg.prg_bytes(seed_of(b"seven-values"), 7 * vb), dtype=np.uint8).reshape(7, vb).copy()
    table[:, vb - 1] = np.arange(7) * 37 + 3            # seven different values at every width
    return table[pick].copy()


# (name, n): all of them at every key width of KEY_BYTES
CRAFTED = (("all_equal", crafted_all_equal, 5000), ("two_values", crafted_two_values, 5001), ("last_byte", crafted_last_byte, 4500),
           ("first_byte", crafted_first_byte, 4500), ("sorted", crafted_sorted, 4200), ("reversed", crafted_reversed, 4200),
           ("runs", crafted_runs, 3 * TILE + 100), ("seven_values", crafted_seven_values, 70001))
