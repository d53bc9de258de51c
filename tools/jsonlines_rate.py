#!/usr/bin/env python3
"""jsonlines_rate.py — reading and writing a ciphertext list in the json interface (one {"alpha":"A","beta":"B"} line of decimal
strings per ciphertext), on the GPU against the obvious host conversion, in one process.

  python tools/jsonlines_rate.py [-n 1000000] [--passes 3] [--out profiles/jsonlines_rate.txt] [--bench-ms PARENT THIS]

One list: N lines over the 2048-bit safe-prime group at width 1 (up to 1257 bytes a line).  After one untimed pass of each,
--passes alternating passes of
  (a) read, device:   interface.parse_json(text)  (vmn_garrays_from_jsonlines + membership), host clock around the call, which
                      ends in a synchronisation: the upload of the text is inside;
  (b) read, host:     int() per number, to_bytes and a transposition into the raw tree, proofdir.parse_ciphertexts (+ the same
                      membership calls);
  (c) write, device:  interface.format_json(arrays), the download of the text inside;
  (d) write, host:    toBytes per array, int.from_bytes and str() per value, one join.
Every time, the medians and the spreads (max - min) are written to --out, with the share of the kernels of
csrc/decimal_kernels.h (the timing family "jsonlines") in the GPU time of one more reading and one more writing pass under
vmn_ctx_timing_report.  By the rule of profiles/README.md the device path is called faster only if the gap of the medians
exceeds five times the larger spread.  --bench-ms records the two ms_per_step of bench.py (parent commit, this commit) that
were measured beside this run."""
import argparse
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hdr(tag, count):
    return bytes([tag]) + count.to_bytes(4, "big")


def host_json_to_raw(text, vb):
    """The obvious host conversion at width 1: the raw list tree (proofdir's file format) of a json text."""
    leaf = hdr(1, vb)
    us, vs = [], []
    for line in text.split(b"\n"):
        if not line:
            continue
        # {"alpha":"A","beta":"B"}: the writer's own form, cut at its quotes
        parts = line.split(b'"')
        us.append(leaf + int(parts[3]).to_bytes(vb, "big"))
        vs.append(leaf + int(parts[7]).to_bytes(vb, "big"))
    n = len(us)
    return hdr(0, 2) + hdr(0, n) + b"".join(us) + hdr(0, n) + b"".join(vs)


def host_arrays_to_json(comps, vb):
    ub, vbts = comps[0].toBytes(), comps[1].toBytes()
    n = len(ub) // vb
    return b"".join(b'{"alpha":"%d","beta":"%d"}\n' % (int.from_bytes(ub[i * vb:(i + 1) * vb], "big"), int.from_bytes(vbts[i * vb:(i + 1) * vb], "big"))
                    for i in range(n))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def line(label, xs):
    return "%-46s median %8.3f s  (min %8.3f  max %8.3f  spread %6.3f)  samples %s" % (
        label, statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), " ".join("%.3f" % x for x in xs))


def verdict(dev, host):
    gap = statistics.median(host) - statistics.median(dev)
    spread = max(max(dev) - min(dev), max(host) - min(host))
    return "gap of the medians host - device: %.3f s; five times the larger spread: %.3f s -> %s" % (
        gap, 5 * spread, "the device path is faster" if gap > 5 * spread else "the host path is faster" if -gap > 5 * spread else "no claim either way")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jsonlines_rate.txt"))
    ap.add_argument("--bench-ms", nargs=2, type=float, metavar=("PARENT", "THIS"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import interface, proofdir, stdgroups
    ctx = vmn.Context(0)
    p, q, g = stdgroups.modp_group(2048)
    grp = vmn.ModPGroup(ctx, p, q, g, nbytes=256)
    vb, w = grp.nbytes, 1
    seeds = [hashlib.sha256(b"jsonlines-rate/%d" % c).digest() for c in range(2)]
    comps = [grp.exp(grp.g, grp.ringArrayFromPRG(seed, args.n, grp.q.bit_length() - 1)) for seed in seeds]
    text = interface.format_json(comps)

    def read_device():
        got = interface.parse_json(grp, text, w)
        assert got is not None
        return got

    def read_host():
        got = proofdir.parse_ciphertexts(grp, host_json_to_raw(text, vb), w)
        assert got is not None and all(a.isMember() for a in got)
        return got

    a = read_device()
    b = read_host()
    assert all(x.equals(y) and x.equals(z) for x, y, z in zip(a, b, comps)), "the two readers disagree"
    for arr in a + b:
        arr.free()
    assert host_arrays_to_json(comps, vb) == text, "the two writers disagree"
    rd, rh, wd, wh = [], [], [], []
    for _ in range(args.passes):
        dt, got = timed(read_device)
        rd.append(dt)
        for arr in got:
            arr.free()
        dt, got = timed(read_host)
        rh.append(dt)
        for arr in got:
            arr.free()
        wd.append(timed(lambda: interface.format_json(comps))[0])
        wh.append(timed(lambda: host_arrays_to_json(comps, vb))[0])
    # the share of the new kernels in the GPU time of one reading and one writing pass
    shares = []
    for label, fn in (("reading", read_device), ("writing", lambda: interface.format_json(comps))):
        ctx.timing_enable(True)
        ctx.timing_reset()
        got = fn()
        rep = ctx.timing_report()
        ctx.timing_enable(False)
        if isinstance(got, list):
            for arr in got:
                arr.free()
        total = sum(v[1] for v in rep.values())
        mine = rep.get("jsonlines", (0, 0.0))[1]
        shares.append("    GPU time of one %s pass by kernel family: %s; jsonlines = %.1f %% of %.2f ms"
                      % (label, ", ".join("%s %.2f ms (%d launches)" % (k, v[1], v[0]) for k, v in sorted(rep.items())), 100 * mine / max(total, 1e-9), total))
    out = ["== a ciphertext list in the json interface: device against host conversion ==",
           "(tools/jsonlines_rate.py -n %d --passes %d, one MI355X, one process, the passes alternating; wall time around the calls)" % (args.n, args.passes),
           "",
           "2048-bit safe-prime group, 256-byte leaves, width 1, N = %d: %.1f MB of text, %.1f bytes a line on average" % (args.n, len(text) / 1e6, len(text) / args.n),
           line("(a) read, device (parse_json)", rd),
           line("(b) read, host (int(), to_bytes, raw parse)", rh),
           "    " + verdict(rd, rh),
           line("(c) write, device (format_json)", wd),
           line("(d) write, host (toBytes, from_bytes, str(), join)", wh),
           "    " + verdict(wd, wh)] + shares + [
           "",
           "Kernel shapes: one was built for each kernel -- k_jsonlines_scan walks a line with one lane (eight digits a step inside a",
           "number), k_dec_to_rows and k_rows_to_dec give a wave to a value and a column of the table product to a lane.  The scan",
           "with several lanes per line on ballot masks was not built, so there is no second number to set beside these.", ""]
    if args.bench_ms:
        out += ["bench.py --gpus 1, ms_per_step: parent commit %.1f, this commit %.1f (one run each; the headline kernels are untouched)" % tuple(args.bench_ms), ""]
    print("\n".join(out), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))
    for arr in comps:
        arr.free()
    grp.close()


if __name__ == "__main__":
    main()
