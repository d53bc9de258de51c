#!/usr/bin/env python3
"""permutation_rate.py — a prover's secret permutation drawn on the GPU from one seed against the host draws, in one process.

  python tools/permutation_rate.py [--sizes 10000 100000 1000000 4194304] [--passes 5] [--rbitlen 100]
                                   [--out profiles/permutation_rate.txt] [--bench-ms PARENT THIS]

Per size N, after one untimed draw:
  (a) device draw:  permutation_from_prg(ctx, os.urandom(32), N, rbitlen) -- seed to the two HOST tables (pi, inv), host clock
                    around the call (keys, sort, inverse and the two downloads inside); median of --passes;
  (b) its kernel time: vmn_ctx_timing_get("permutation") (the sort's kernels) and ("prg") (the keys) of one more draw;
  (c) host draw of the parent commit: SecureRandomSource(q).permutation(N) without a context (random.SystemRandom().shuffle);
      --passes draws up to N = 10^5, ONE draw above (it takes seconds);
  (d) for scale: numpy.argsort (stable) of N random 64-bit keys, median of --passes.
The pass count of the sort (one per key byte) and the bytes it moves per pass are stated beside the kernel time, so that it can
be set against the memory bandwidth.  --bench-ms records the two ms_per_step of bench.py (parent commit, this commit)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BYTES_PER_PASS = 14          # per element: histogram 4 + 1 read, 1 written; scatter 4 + 1 read, 4 written (csrc/permutation_kernels.h)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def fmt(xs):
    return "median %9.3f ms  (min %9.3f  max %9.3f)  samples %s" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3,
                                                                   " ".join("%.3f" % (x * 1e3) for x in xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[10 ** 4, 10 ** 5, 10 ** 6, 4194304])
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--rbitlen", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "permutation_rate.txt"))
    ap.add_argument("--bench-ms", type=float, nargs=2, metavar=("PARENT", "THIS"))
    args = ap.parse_args()
    import numpy as np
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import randomsource
    ctx = vmn.Context(0)
    host = randomsource.SecureRandomSource((1 << 255) - 19)
    rng = np.random.Generator(np.random.PCG64(1))
    out = ["== a prover's secret permutation: device draw against host draws ==",
           "(tools/permutation_rate.py --sizes %s --passes %d --rbitlen %d, one MI355X, one process; wall time around the calls)"
           % (" ".join(str(n) for n in args.sizes), args.passes, args.rbitlen), ""]
    for n in args.sizes:
        kbytes = vmn.permutation_key_bytes(n, args.rbitlen)

        def device():
            return vmn.permutation_from_prg(ctx, os.urandom(32), n, args.rbitlen)

        pi, inv = device()                                              # warm-up: the pool's blocks, the pinned buffers
        assert np.array_equal(inv[pi], np.arange(n, dtype=np.uint32))
        dev_t = [timed(device)[0] for _ in range(args.passes)]
        ctx.timing_enable(True)
        ctx.timing_reset()
        device()
        ctx.synchronize()
        launches, sort_ms = ctx.timing_get("permutation")
        _, prg_ms = ctx.timing_get("prg")
        ctx.timing_enable(False)
        host_t = [timed(lambda: host.permutation(n))[0] for _ in range(args.passes if n <= 10 ** 5 else 1)]
        keys = rng.integers(0, 1 << 63, size=n, dtype=np.int64)
        sort_t = [timed(lambda: np.argsort(keys, kind="stable"))[0] for _ in range(args.passes)]
        moved = n * kbytes * BYTES_PER_PASS
        ratio = statistics.median(host_t) / statistics.median(dev_t)
        out += ["N = %d, rbitlen %d: keys of %d bytes, %d radix passes" % (n, args.rbitlen, kbytes, kbytes),
                "  (a) device draw, seed -> host tables pi, inv     " + fmt(dev_t),
                "  (b) kernel time: sort %.3f ms in %d launches, keys (prg) %.3f ms; the passes move %d x %d x N = %.1f MB: %.0f GB/s"
                % (sort_ms, launches, prg_ms, kbytes, BYTES_PER_PASS, moved / 1e6, moved / 1e9 / (sort_ms / 1e3) if sort_ms else 0.0),
                "  (c) host draw, SecureRandomSource.permutation    " + fmt(host_t),
                "  (d) numpy.argsort of 64-bit keys (stable)        " + fmt(sort_t),
                "  host draw / device draw = %.1f" % ratio, ""]
    if args.bench_ms:
        out += ["bench.py --gpus 1 (the headline, which calls none of this): ms_per_step %.3f on the parent commit, %.3f on this one"
                % tuple(args.bench_ms), ""]
    print("\n".join(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
