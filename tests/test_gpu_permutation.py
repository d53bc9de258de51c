"""GPU suite: a prover's secret permutation drawn on the device (include/vmnhip.h: vmn_permutation_key_bytes, vmn_permutation_from_prg,
vmn_permutation_from_keys; include/vmnproofs.h: vmn_permutation_random; csrc/permutation_kernels.h; randomsource.SecureRandomSource
with a context) against tests/permutation_cases.py, the rule restated on Python integers, by exact equality of the tables.

from_prg: n in {0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 65 537, 300 001} (4096 is the sort's tile,
1024 a wave's piece of it), rbitlen 0 / 100 / 256, the three seed lengths.  from_keys: crafted keys at 1, 4, 5, 8, 9, 18, 32 and
64 bytes against numpy.lexsort.  One property case at n = 2^20 + 3.  The sort has one path for every size, so the determinism
test is the same seed twice, on the suite's context and on a fresh one."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from oracle import pyref

import permutation_cases as pc

pytestmark = pytest.mark.gpu

VMN_ERR_ARG, VMN_ERR_UNSUPPORTED = -1, -5
U32P = C.POINTER(C.c_uint32)


def check_tables(pi, inv, want_pi):
    n = len(want_pi)
    assert pi.dtype == np.uint32 and inv.dtype == np.uint32 and pi.shape == inv.shape == (n,)
    assert np.array_equal(pi, np.asarray(want_pi, dtype=np.uint32))
    assert np.array_equal(inv[pi], np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("rbitlen", pc.RBITLENS)
@pytest.mark.parametrize("n", pc.SIZES)
def test_from_prg_is_the_restatement(vmn, gpu_ctx, n, rbitlen):
    assert vmn.permutation_key_bytes(n, rbitlen) == pc.key_bytes(n, rbitlen)
    seed = pc.seed_of(b"gpu/%d/%d" % (n, rbitlen))
    want = pc.restate(seed, n, rbitlen) if n <= 4097 else pc.restate_large(seed, n, rbitlen)[0]
    pi, inv = vmn.permutation_from_prg(gpu_ctx, seed, n, rbitlen)
    check_tables(pi, inv, want)


@pytest.mark.parametrize("seedlen,n", [(32, 257), (48, 1025), (64, 4097)])
def test_from_prg_under_the_three_hashes(vmn, gpu_ctx, seedlen, n):
    seed = pc.seed_of(b"gpu/hash/%d" % seedlen, seedlen)
    pi, inv = vmn.permutation_from_prg(gpu_ctx, seed, n, 100)
    check_tables(pi, inv, pc.restate(seed, n, 100, pc.HASH_OF_SEEDLEN[seedlen]))


@pytest.mark.parametrize("key_bytes", pc.KEY_BYTES)
@pytest.mark.parametrize("name,make,n", pc.CRAFTED, ids=[c[0] for c in pc.CRAFTED])
def test_from_keys_on_crafted_keys(vmn, gpu_ctx, name, make, n, key_bytes):
    rows = make(n, key_bytes)
    want_pi, want_inv = pc.lexsort_rows(rows)
    pi, inv = vmn.permutation_from_keys(gpu_ctx, rows, key_bytes)
    check_tables(pi, inv, want_pi)
    assert np.array_equal(inv, want_inv)
    if name == "all_equal":
        assert np.array_equal(pi, np.arange(n, dtype=np.uint32))
    # one table alone: the other pointer NULL
    only = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    blk = np.ascontiguousarray(rows)
    assert vmn.lib().vmn_permutation_from_keys(gpu_ctx._h, C.c_void_p(blk.ctypes.data), C.c_size_t(key_bytes), C.c_size_t(n), None,
                                               only.ctypes.data_as(U32P)) == 0
    assert np.array_equal(only, want_inv)


def test_from_keys_bytes_and_the_empty_table(vmn, gpu_ctx):
    pi, inv = vmn.permutation_from_keys(gpu_ctx, b"\x02\x01\x02\x00", 1)
    assert pi.tolist() == [3, 1, 0, 2] and inv.tolist() == [2, 1, 3, 0]
    pi, inv = vmn.permutation_from_keys(gpu_ctx, b"", 18)
    assert pi.shape == inv.shape == (0,)


def test_a_million_entries_are_a_permutation_in_key_order(vmn, gpu_ctx):
    n, rbitlen = (1 << 20) + 3, 100
    seed = pc.seed_of(b"gpu/property")
    pi, inv = vmn.permutation_from_prg(gpu_ctx, seed, n, rbitlen)
    assert np.array_equal(np.bincount(pi, minlength=n), np.ones(n, dtype=np.int64))
    assert np.array_equal(inv[pi], np.arange(n, dtype=np.uint32))
    rows = pc.key_rows(seed, n, rbitlen)[pi]                 # the keys read through pi: non-decreasing, equal ones by index
    differ = rows[1:] != rows[:-1]
    first = differ.argmax(axis=1)
    at = np.arange(n - 1)
    distinct = differ.any(axis=1)
    assert (rows[1:][at, first] >= rows[:-1][at, first]).all()
    assert (pi[1:][~distinct] > pi[:-1][~distinct]).all()


def test_the_same_seed_gives_the_same_bytes(vmn, gpu_ctx):
    seed = pc.seed_of(b"gpu/twice")
    first = vmn.permutation_from_prg(gpu_ctx, seed, 70001, 100)
    again = vmn.permutation_from_prg(gpu_ctx, seed, 70001, 100)
    other = vmn.Context(0)
    fresh = vmn.permutation_from_prg(other, seed, 70001, 100)
    other.close()
    for a, b in ((first, again), (first, fresh)):
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert first[0].tobytes() != vmn.permutation_from_prg(gpu_ctx, pc.seed_of(b"gpu/another"), 70001, 100)[0].tobytes()


class CountingSource:
    def __init__(self, seeds):
        self.seeds, self.calls = list(seeds), 0

    def array_seed(self):
        self.calls += 1
        return self.seeds[self.calls - 1]


class RowsOnlySource:
    """A source without array_seed: every other draw is forbidden too."""

    def ring_array(self, n):
        raise AssertionError("the source must not be called")

    ring_element = int_array = ring_array


@pytest.fixture(scope="module")
def native(entry):
    import mirror
    return mirror.load(entry, ("native",))["native"]


@pytest.mark.parametrize("n", (0, 1, 300, 5000))
def test_random_permutation_takes_one_seed_of_the_source(vmn, gpu_ctx, native, n):
    seeds = [pc.seed_of(b"source/a"), pc.seed_of(b"source/b")]
    src = CountingSource(seeds)
    pi, inv = native.random_permutation(gpu_ctx, src, n, 100)
    assert src.calls == 1
    want = vmn.permutation_from_prg(gpu_ctx, seeds[0], n, 100)
    assert np.array_equal(pi, want[0]) and np.array_equal(inv, want[1])
    check_tables(pi, inv, pc.restate(seeds[0], n, 100))


def test_random_permutation_without_array_seed_is_unsupported(vmn, gpu_ctx, native):
    with pytest.raises(vmn.VmnError) as err:
        native.random_permutation(gpu_ctx, RowsOnlySource(), 100, 100)
    assert err.value.status == VMN_ERR_UNSUPPORTED and "array_seed" in str(err.value)


def test_the_secure_source_draws_its_permutation_on_the_device(entry, vmn, gpu_ctx, tmp_path):
    import mirror
    mods = mirror.load(entry, ("proofdir", "randomsource"))
    pd, rs = mods["proofdir"], mods["randomsource"]
    grpd, _ = load_golden(512)
    p, q, g = grpd["p"], grpd["q"], grpd["g"]
    src = rs.SecureRandomSource(q, ctx=gpu_ctx)
    for n in (0, 1, 40, 5000):
        pi = src.permutation(n)
        assert isinstance(pi, np.ndarray) and pi.dtype == np.uint32 and sorted(pi.tolist()) == list(range(n))
    assert src.permutation(5000).tobytes() != src.permutation(5000).tobytes()          # fresh seeds
    assert sorted(rs.SecureRandomSource(q).permutation(40)) == list(range(40))          # without a context: the host's shuffle
    # a shuffle written with that source verifies
    n = 40
    G = vmn.ModPGroup(gpu_ctx, p, q, g)
    params = {"version": "3.1.0", "sid": "SessionID", "auxsid": "default", "rbitlen": 100, "vbitlenro": 256, "ebitlenro": 256,
              "prg": "SHA-256", "rohash": "SHA-256", "rohash_name": "SHA-256", "width": 1, "pgroup": "ModPGroup(512)",
              "group": {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(g, "x")}}
    tape = rs.InsecureShaRandomSource(b"permutation-shuffle", q)
    y = pow(g, tape.ring_element(), p)
    t_enc, msgs = tape.ring_array(n), tape.ring_array(n)
    w = [pyref.exp_fixed(g, t_enc, p), pyref.mul(pyref.exp_fixed(g, msgs, p), pyref.exp_fixed(y, t_enc, p), p)]
    W = [G.toElementArray(c) for c in w]
    nizkp = str(tmp_path / "nizkp")
    pd.write_inputs(nizkp, G, params, [g, y], W)
    pd.write_shuffle(nizkp, 1, G, params, [g, y], W, src)
    assert pd.verify_shuffle(nizkp, 1, G, params, [g, y])


def raw_calls(vmn, ctx):
    """(name, call(pi, inv) -> status) of every misuse; pi / inv are ctypes pointers or None."""
    lib = vmn.lib()
    seed = pc.seed_of(b"misuse")
    keys = bytes(range(64)) * 4
    sz = C.c_size_t

    def prg(seedlen=32, n=4, rbitlen=100):
        return lambda pi, inv: lib.vmn_permutation_from_prg(ctx._h, seed + seed, sz(seedlen), sz(n), C.c_int(rbitlen), pi, inv)

    def from_keys(key_bytes):
        return lambda pi, inv: lib.vmn_permutation_from_keys(ctx._h, keys, sz(key_bytes), sz(4), pi, inv)
    return [("key_bytes 0", from_keys(0)), ("key_bytes 65", from_keys(65)), ("rbitlen -1", prg(rbitlen=-1)), ("rbitlen 257", prg(rbitlen=257)),
            ("seedlen 31", prg(seedlen=31)), ("n = 2^32", prg(n=1 << 32))]


def test_misuse_is_refused_and_nothing_is_written(vmn, gpu_ctx):
    lib = vmn.lib()
    for name, call in raw_calls(vmn, gpu_ctx):
        pi = np.full(8, 0xA5A5A5A5, dtype=np.uint32)
        inv = np.full(8, 0x5A5A5A5A, dtype=np.uint32)
        assert call(pi.ctypes.data_as(U32P), inv.ctypes.data_as(U32P)) == VMN_ERR_ARG, name
        assert lib.vmn_last_error(), name
        assert (pi == 0xA5A5A5A5).all() and (inv == 0x5A5A5A5A).all(), name
    # both tables NULL
    seed = pc.seed_of(b"misuse")
    assert lib.vmn_permutation_from_prg(gpu_ctx._h, seed, C.c_size_t(32), C.c_size_t(4), C.c_int(100), None, None) == VMN_ERR_ARG
    assert lib.vmn_permutation_from_keys(gpu_ctx._h, b"abcd", C.c_size_t(1), C.c_size_t(4), None, None) == VMN_ERR_ARG
    assert b"table" in lib.vmn_last_error()
    # the width of a key: 0 out of range
    for n, rbitlen in ((1 << 32, 100), (4, -1), (4, 257)):
        assert vmn.permutation_key_bytes(n, rbitlen) == 0
    # the context still serves
    pi, _ = vmn.permutation_from_prg(gpu_ctx, seed, 4, 100)
    assert pi.tolist() == pc.restate(seed, 4, 100)
