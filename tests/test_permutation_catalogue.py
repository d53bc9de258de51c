"""CPU suite: the catalogue of tests/permutation_cases.py checks what it claims -- the key-width rule at its edges, that the
rule reaches every order of four elements, and that the restatement agrees with a second, independent statement of the order."""
import hashlib
import itertools

import permutation_cases as pc


def test_the_key_width_rule():
    log2 = {0: 1, 1: 1, 2: 1, 3: 2, 4: 2, 5: 3, 1 << 16: 16, (1 << 16) + 1: 17, (1 << 32) - 1: 32}
    for n, lg in log2.items():
        assert pc.ceil_log2(max(n, 2)) == lg, n
        assert 1 << lg >= max(n, 2) and (lg == 1 or 1 << (lg - 1) < n), n        # the definition of ceil(log2)
        for rbitlen in (0, 100, 256):
            kb = pc.key_bits(n, rbitlen)
            assert kb == rbitlen + 2 * lg
            assert pc.key_bytes(n, rbitlen) == (kb + 7) // 8 <= 40
            # some tie occurs with probability at most n^2 / 2^(kb + 1) <= 2^-(rbitlen + 1)
            assert n * n << (rbitlen + 1) <= 1 << (kb + 1)
    assert pc.key_bytes((1 << 32) - 1, 256) == 40 and pc.key_bytes(0, 0) == 1 and pc.key_bytes(10 ** 6, 100) == 18


def test_all_24_orders_of_four_elements_occur():
    seen = set()
    for i in range(2400):
        seed = hashlib.sha256(i.to_bytes(4, "big")).digest()
        seen.add(tuple(pc.restate(seed, 4, 100)))
    assert seen == set(itertools.permutations(range(4)))


def test_restate_agrees_with_insertion_by_comparison():
    for n in list(range(0, 12)) + [31, 50]:
        for rbitlen in (0, 100):
            for hashname in ("sha256", "sha384", "sha512"):
                seed = pc.seed_of(b"insert/%d/%d" % (n, rbitlen), {"sha256": 32, "sha384": 48, "sha512": 64}[hashname])
                keys = pc.keys_of(seed, n, rbitlen, hashname)
                assert pc.restate(seed, n, rbitlen, hashname) == pc.by_insertion(keys), (n, rbitlen, hashname)
    # with ties: rbitlen 0 at n = 50 has 12-bit keys; a few bits make them certain
    keys = [k & 7 for k in pc.keys_of(pc.seed_of(b"ties"), 50, 0)]
    assert len(set(keys)) < 50
    assert sorted(range(50), key=lambda i: (keys[i], i)) == pc.by_insertion(keys)


def test_the_numpy_statement_agrees_with_the_integers():
    import numpy as np
    for n, rbitlen, seedlen in ((0, 100, 32), (1, 0, 32), (257, 100, 32), (300, 0, 48), (1025, 256, 64)):
        seed = pc.seed_of(b"numpy/%d" % n, seedlen)
        h = pc.HASH_OF_SEEDLEN[seedlen]
        pi, inv = pc.restate_large(seed, n, rbitlen, h)
        assert pi.tolist() == pc.restate(seed, n, rbitlen, h)
        assert (inv[pi] == np.arange(n)).all()
        rows = pc.key_rows(seed, n, rbitlen, h)
        assert [int.from_bytes(bytes(r), "big") for r in rows] == pc.keys_of(seed, n, rbitlen, h)


def test_the_crafted_keys_are_what_their_names_say():
    import numpy as np
    for name, make, n in pc.CRAFTED:
        for vb in pc.KEY_BYTES:
            rows = make(n, vb)
            assert rows.shape == (n, vb) and rows.dtype == np.uint8, (name, vb)
            pi, _ = pc.lexsort_rows(rows)
            distinct = len({bytes(r) for r in rows})
            if name == "all_equal":
                assert distinct == 1 and (pi == np.arange(n)).all()
            elif name == "two_values":
                assert distinct == 2 and pi[0] == 1 and pi[-1] == n - 1
            elif name == "sorted":
                assert (pi == np.arange(n)).all() and distinct == (n if vb > 1 else 256)
            elif name == "reversed":
                assert distinct == (n if vb > 1 else 256) and (vb == 1 or (pi == np.arange(n)[::-1]).all())
            elif name == "seven_values":
                assert distinct == 7
            elif name == "runs":
                assert distinct == 7 and n > 3 * pc.TILE
                ends = np.flatnonzero(rows[1:, vb - 1] != rows[:-1, vb - 1]) + 1
                assert {pc.WAVE_PIECE - 3, pc.WAVE_PIECE + 2, pc.TILE - 3, pc.TILE + 2, 2 * pc.TILE - 3, 2 * pc.TILE + 2} <= set(ends.tolist())
            else:
                assert distinct >= 250, (name, vb)          # last_byte / first_byte: one byte tells the keys apart


def test_the_tile_is_the_kernels_tile():
    import os
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "verificatum-vmn_amd", "csrc", "permutation_kernels.h")).read()
    block = int(re.search(r"SORT_BLOCK = (\d+);", src).group(1))
    items = int(re.search(r"SORT_ITEMS = (\d+);", src).group(1))
    assert (pc.TILE, pc.WAVE_PIECE) == (block * items, 64 * items)
    assert {pc.TILE - 1, pc.TILE, pc.TILE + 1} <= set(pc.SIZES)
