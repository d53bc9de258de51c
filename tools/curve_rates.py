#!/usr/bin/env python3
"""Rates of the curve array operations over named curves, in one process (GPU box): exp_fixed (fixed-base powers of the
generator, the table built before timing), exp_array (variable-base, one scalar per point) and expProd (one
multi-exponentiation) at N = 10^5 and 10^6, for P-256 (the NIST kernels) and brainpoolp256r1, secp256k1, brainpoolp384r1
(the general-a kernels).  Wall time around each call with the device synchronised, the median of three after one untimed
pass; points per second, and each curve's rate relative to P-256's at the same N.

    python3 tools/curve_rates.py [--curves P-256,brainpoolp256r1,...] [--sizes 100000,1000000] [--out FILE]
"""
import argparse
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--curves", default="P-256,brainpoolp256r1,secp256k1,brainpoolp384r1")
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    vmn = entry.load_package()
    spec = importlib.util.spec_from_file_location("rs", os.path.join(entry.PKG_DIR, "randomsource.py"))
    rs = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rs)
    ctx = vmn.Context(0)
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn):
        fn()
        ctx.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            r = fn()
            ctx.synchronize()
            ts.append(time.perf_counter() - t0)
            if hasattr(r, "free"):
                r.free()
        return statistics.median(ts)

    rates = {}
    emit("%-16s %8s %14s %14s %14s   (points / s; median of %d)" % ("curve", "N", "exp_fixed", "exp_array", "expProd", args.reps))
    for name in args.curves.split(","):
        G = vmn.ECqPGroup(ctx, name)
        for n in (int(s) for s in args.sizes.split(",")):
            rnd = rs.InsecureBulkRandomSource(7, G.q, G.exp_bytes)
            E = G.ringArray(rnd.ring_array(n))
            X = G.exp(G.g, G.ringArray(rnd.ring_array(n)))
            ctx.synchronize()
            t = dict(exp_fixed=timed(lambda: G.exp(G.g, E)), exp_array=timed(lambda: X.exp(E)), expProd=timed(lambda: X.expProd(E)))
            rates[name, n] = {k: n / v for k, v in t.items()}
            emit("%-16s %8d %14.0f %14.0f %14.0f" % (name, n, rates[name, n]["exp_fixed"], rates[name, n]["exp_array"], rates[name, n]["expProd"]))
            X.free()
            E.free()
    base = args.curves.split(",")[0]
    emit("relative to %s:" % base)
    for (name, n), r in rates.items():
        if (base, n) in rates and name != base:
            b = rates[base, n]
            emit("%-16s %8d %14.2f %14.2f %14.2f" % (name, n, r["exp_fixed"] / b["exp_fixed"], r["exp_array"] / b["exp_array"], r["expProd"] / b["expProd"]))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
