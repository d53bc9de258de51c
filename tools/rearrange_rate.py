#!/usr/bin/env python3
"""rearrange_rate.py — `vre -cat` and `vre -sub` file to file at the size of an election, in one process.

  python tools/rearrange_rate.py [--lists 4] [--n 250000] [--bits 2048] [--passes 3] [--dir DIR]
                                 [--out profiles/rearrange_rate.txt] [--bench-ms PARENT THIS]

--lists raw lists of --n ciphertexts each (width 1, the RFC 3526 group of --bits bits; members: g^r drawn on the device) are
written to DIR.  Then, --passes times alternating, after one untimed pass of each:
  (a) -cat: rearrange.cat_files of the lists into one file -- read, import, membership, ONE "segments" launch per component
      array, export, write -- host clock around the call;
  (b) -sub: rearrange.sub_files of that file back into --lists files of --n.
Beside each: the time of the kernels of the family "segments" (k_rows_segments) of one more pass with the context's timing on,
and the bytes they move (read + written).  The last -sub pass is compared with the input files byte for byte.
--bench-ms records the two ms_per_step of bench.py (parent commit, this commit)."""
import argparse
import hashlib
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def fmt(xs):
    return "median %9.1f ms  (min %9.1f  max %9.1f)  samples %s" % (statistics.median(xs) * 1e3, min(xs) * 1e3, max(xs) * 1e3,
                                                                   " ".join("%.1f" % (x * 1e3) for x in xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lists", type=int, default=4)
    ap.add_argument("--n", type=int, default=250000)
    ap.add_argument("--bits", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--dir")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rearrange_rate.txt"))
    ap.add_argument("--bench-ms", type=float, nargs=2, metavar=("PARENT", "THIS"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import proofdir, rearrange, stdgroups
    ctx = vmn.Context(0)
    p, q, g = stdgroups.modp_group(args.bits)
    grp = vmn.ModPGroup(ctx, p, q, g)
    work = tempfile.mkdtemp(prefix="rearrange_rate_", dir=args.dir)
    try:
        ins = [os.path.join(work, "in%d.bt" % k) for k in range(args.lists)]
        outs = [os.path.join(work, "out%d.bt" % k) for k in range(args.lists)]
        joined = os.path.join(work, "joined.bt")
        for k, path in enumerate(ins):
            comps = []
            for c in range(2):
                e = grp.ringArrayFromPRG(hashlib.sha256(b"rearrange_rate/%d/%d" % (k, c)).digest(), args.n, q.bit_length() - 1)
                comps.append(grp.exp(g, e))
                e.free()
            proofdir.write_ciphertexts(path, comps)
            for a in comps:
                a.free()
        intervals = [(k * args.n, (k + 1) * args.n) for k in range(args.lists)]
        cat = lambda: rearrange.cat_files(grp, ins, joined, 1, 1, True)
        sub = lambda: rearrange.sub_files(grp, joined, outs, intervals, 1, 1, True)
        cat()                                                            # warm-up: the pool's blocks, the pinned buffers, the page cache
        sub()
        cat_t, sub_t = [], []
        for _ in range(args.passes):
            cat_t.append(timed(cat))
            sub_t.append(timed(sub))
        for a, b in zip(ins, outs):
            with open(a, "rb") as fa, open(b, "rb") as fb:
                assert fa.read() == fb.read(), "-sub of -cat is not the input again: " + a
        kernel = {}
        ctx.timing_enable(True)
        for name, fn in (("cat", cat), ("sub", sub)):
            ctx.timing_reset()
            fn()
            ctx.synchronize()
            kernel[name] = (ctx.timing_get("segments"), {k: v[:2] for k, v in ctx.timing_report().items() if v[0]})
        ctx.timing_enable(False)
        file_bytes = os.path.getsize(joined)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    total = args.lists * args.n
    row = 4 * ((-(-args.bits // 28) + 3) // 4 * 4)                        # bytes of a device row: a 32-bit word per 28-bit limb, padded to 4 words
    moved = 2 * 2 * total * row                                          # two component arrays, read + written
    out = ["== vre -cat and -sub, file to file ==",
           "(tools/rearrange_rate.py --lists %d --n %d --bits %d --passes %d, one MI355X, one process; wall time around the calls, files on local disk)"
           % (args.lists, args.n, args.bits, args.passes), "",
           "%d raw lists of %d ciphertexts, width 1, %d-bit group: the joined file has %.1f MB" % (args.lists, args.n, args.bits, file_bytes / 1e6), ""]
    for name, ts in (("cat", cat_t), ("sub", sub_t)):
        (launches, ms), families = kernel[name]
        out += ["  -%s, files -> file%s   %s" % (name, "" if name == "cat" else "s", fmt(ts)),
                "        \"segments\" kernels: %d launches, %.3f ms; %d rows of %d bytes read and written = %.1f MB: %.0f GB/s; %.2f %% of the median pass"
                % (launches, ms, 2 * total, row, moved / 1e6, moved / 1e9 / (ms / 1e3) if ms else 0.0, 100 * ms / 1e3 / statistics.median(ts)),
                "        all kernel families of one pass (launches, ms): " + ", ".join("%s %d %.2f" % (k, v[0], v[1]) for k, v in sorted(families.items())),
                "        the rest of the pass is the host: file read, upload, download, file write", ""]
    if args.bench_ms:
        out += ["bench.py --gpus 1 (the headline, which calls none of this): ms_per_step %.3f on the parent commit, %.3f on this one"
                % tuple(args.bench_ms), ""]
    print("\n".join(out), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
