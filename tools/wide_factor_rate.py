#!/usr/bin/env python3
"""What one launch for the omega component arrays of a party's decryption factors is worth: vmn_garray_exp_scalar_multi over a
2048-bit group with a full-length exponent, omega = 3, fused (the default) against VMN_EXP_MULTI_FUSED=0 (one launch per
array), same build, same process, the two arms alternating.  With --keywidth kappa > 1 the factors are those under a key of
width kappa: kappa * omega arrays, array c under exponent c mod kappa of kappa full-length exponents
(vmn_garray_exp_scalars_multi: one launch per eight arrays, each array under its own schedule).
With --curve NAME the group is ECqPGroup over that curve and the arms are the signed windows in one launch (k_ec_mulshared, the
default) against VMN_EC_SHARED=0 (the parent's path: k_ec_mulvar, fixed unsigned windows, one launch per array).

    python3 tools/wide_factor_rate.py [--curve P-256] [--keywidth 2] [--sizes 10000,100000,1000000] [--passes 7]
                                      [--out profiles/wide_factor_rates.txt [--append]]

A pass times one call of each arm: host clock around the call and a device synchronise, results freed outside the window.
Two warm-up passes per size (code objects, scratch and pool blocks of the size exist afterwards).  Reported per size and arm:
median, minimum and maximum over the passes, and the run-to-run spread (max - min) / median of each arm; "fused / separate" is
the ratio of the medians.  A difference below the spread of the separate runs is no difference."""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry          # noqa: E402
from oracle import pyref                 # noqa: E402

WIDTH = 3


KNOB = "VMN_EXP_MULTI_FUSED"             # the environment variable whose value 0 selects the second arm (main() may change it)


def timed(ctx, vmn, arrays, e, fused):
    if fused:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = "0"
    ctx.synchronize()
    t0 = time.perf_counter()
    out = vmn.PGroupElementArray.expMultiEach(arrays, e) if isinstance(e, list) else vmn.PGroupElementArray.expMulti(arrays, e)
    ctx.synchronize()
    dt = time.perf_counter() - t0
    os.environ.pop(KNOB, None)
    return dt, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--keywidth", type=int, default=1)
    ap.add_argument("--curve", default=None, help="a curve name: the signed-window launch against VMN_EC_SHARED=0")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    args = ap.parse_args()
    vmn = entry.load_package()
    ctx = vmn.Context(0)
    global KNOB
    if args.curve:
        G = vmn.ECqPGroup(ctx, args.curve)
        q, g = G.q, G.g
        KNOB, arms, group = "VMN_EC_SHARED", {True: "shared", False: "parent"}, f"{args.curve},"
    else:
        p, q, g = pyref.modp_group(2048)
        G = vmn.ModPGroup(ctx, p, q, g)
        arms, group = {True: "fused", False: "separate"}, "2048-bit group,"
    kw = max(1, args.keywidth)
    narrays = kw * WIDTH
    es = [v | (1 << (q.bit_length() - 2)) for v in pyref.stream_ints(b"wide_factor_rate/e", kw, q)]
    e = es[0] if kw == 1 else [es[c % kw] for c in range(narrays)]
    what = "vmn_garray_exp_scalar_multi" if kw == 1 else f"vmn_garray_exp_scalars_multi, key width {kw},"
    lines = [f"# {what} {group} {es[0].bit_length()}-bit exponent{'s' if kw > 1 else ''}, omega = {WIDTH}; {args.passes} alternating passes after 2 warm-up passes",
             f"# times in ms per call (all {narrays} arrays); spread = (max - min) / median of the arm",
             f"# {'N':>8} {'arm':>9} {'median':>9} {'min':>9} {'max':>9} {'spread':>7} {'modexp/s':>10}  {arms[True]}/{arms[False]}"]
    for n in [int(s) for s in args.sizes.split(",")]:
        arrays = [G.exp(g, G.ringArrayFromPRG(hashlib.sha256(b"wide_factor_rate/%d/%d" % (n, c)).digest(), n, q.bit_length() - 1)) for c in range(narrays)]
        first = {}
        for fused in (True, False):                                   # warm-up, and: the two arms give the same arrays
            for _ in range(2):
                _, out = timed(ctx, vmn, arrays, e, fused)
                first[fused] = [o.toBytes() for o in out] if n <= 100000 else None
                for o in out:
                    o.free()
        assert first[True] == first[False], "the two arms' results differ"
        t = {True: [], False: []}
        for i in range(args.passes):
            for fused in ((True, False) if i % 2 == 0 else (False, True)):
                dt, out = timed(ctx, vmn, arrays, e, fused)
                t[fused].append(dt * 1e3)
                for o in out:
                    o.free()
        med = {f: statistics.median(t[f]) for f in t}
        for fused in (True, False):
            ts = t[fused]
            ratio = f"  {med[True] / med[False]:.3f}" if fused else ""
            lines.append(f"  {n:>8} {arms[fused]:>9} {med[fused]:9.3f} {min(ts):9.3f} {max(ts):9.3f} {(max(ts) - min(ts)) / med[fused]:7.3f} "
                         f"{narrays * n / med[fused] * 1e3:10.4g}{ratio}")
        for a in arrays:
            a.free()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a" if args.append else "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
