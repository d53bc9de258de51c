#!/usr/bin/env python3
"""hexlines_rate.py — reading and writing a ciphertext list in the native interface (one hex line per ciphertext), on the GPU
against the obvious host conversion, in one process.

  python tools/hexlines_rate.py [-n 1000000] [--passes 3] [--out profiles/hexlines_rate.txt]

Two lists: N lines over the 2048-bit safe-prime group at width 1 (527 bytes = 1054 digits a line at 256-byte leaves) and N
lines over P-256 at width 3 (501 bytes at 33-byte coordinates).  Per list, after one untimed pass of each, --passes alternating
passes of
  (a) read, device:  interface.parse_native(text)            (vmn_garrays_from_hexlines + membership), host clock around the
                     call, which ends in a synchronisation: the upload of the text is inside;
  (b) read, host:    bytes.fromhex per line, a transposition into the raw tree with numpy, proofdir.parse_ciphertexts
                     (+ the same membership calls);
and, outside the alternation, --passes each of
  (c) write, device: interface.format_native(arrays);
  (d) the floor:     the host-to-device copy of the text's bytes alone: hipMemcpy of the same pageable buffer into a device
                     buffer, through ctypes on the HIP runtime the library has loaded.
Every time, the medians and the spreads (max - min) are written to --out.  The parent has no native reader: (b) is the
comparison.  By the rule of profiles/README.md the device path is called faster only if the gap of the medians exceeds five
times the larger spread."""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def hdr(tag, count):
    return bytes([tag]) + count.to_bytes(4, "big")


def host_native_to_raw(text, curve, vb, w):
    """The obvious host conversion: the raw list tree (proofdir's file format) of a native text, with numpy for the transposition."""
    import numpy as np
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    n = len(lines)
    E = 15 + 2 * vb if curve else 5 + vb
    B = 5 + (10 if w > 1 else 0) + 2 * w * E
    rec = np.frombuffer(b"".join(bytes.fromhex(l.decode("ascii")) for l in lines), dtype=np.uint8).reshape(n, B)
    head = 5 + (5 if w > 1 else 0)
    offs = [head + c * E for c in range(w)] + [head + w * E + (5 if w > 1 else 0) + c * E for c in range(w)]
    out = [hdr(0, 2)]
    for half in range(2):
        if w > 1:
            out.append(hdr(0, w))
        for c in range(w):
            off = offs[half * w + c]
            out.append(hdr(0, n) + np.ascontiguousarray(rec[:, off:off + E]).tobytes())
    return b"".join(out)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def line(label, xs):
    return "%-42s median %8.3f s  (min %8.3f  max %8.3f  spread %6.3f)  samples %s" % (
        label, statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), " ".join("%.3f" % x for x in xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hexlines_rate.txt"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import interface, proofdir, stdgroups
    ctx = vmn.Context(0)
    hip = C.CDLL("libamdhip64.so")
    out = ["== a ciphertext list in the native interface: device against host conversion ==",
           "(tools/hexlines_rate.py -n %d --passes %d, one MI355X, one process; wall time around the calls)" % (args.n, args.passes), ""]
    p, q, g = stdgroups.modp_group(2048)
    lists = [("2048-bit safe-prime group, 256-byte leaves, width 1", vmn.ModPGroup(ctx, p, q, g, nbytes=256), 1),
             ("P-256, 33-byte coordinates, width 3", vmn.ECqPGroup(ctx, "P-256", java_widths=True), 3)]
    for title, grp, w in lists:
        curve = grp.coord_bytes is not None
        vb = grp.coord_bytes if curve else grp.nbytes
        seeds = [hashlib.sha256(b"hexlines-rate/%d" % c).digest() for c in range(2 * w)]
        comps = [grp.exp(grp.g, grp.ringArrayFromPRG(seed, args.n, grp.q.bit_length() - 1)) for seed in seeds]
        text = interface.format_native(comps)
        B = interface.ciphertext_line_bytes(grp, w)
        assert len(text) == args.n * (2 * B + 1)

        def read_device():
            got = interface.parse_native(grp, text, w)
            assert got is not None
            return got

        def read_host():
            got = proofdir.parse_ciphertexts(grp, host_native_to_raw(text, curve, vb, w), w)
            assert got is not None and all(a.isMember() for a in got)
            return got

        def copy_alone():
            dev = C.c_void_p()
            assert hip.hipMalloc(C.byref(dev), C.c_size_t(len(text))) == 0
            t0 = time.perf_counter()
            assert hip.hipMemcpy(dev, text, C.c_size_t(len(text)), C.c_int(1)) == 0 and hip.hipDeviceSynchronize() == 0
            dt = time.perf_counter() - t0
            hip.hipFree(dev)
            return dt

        a = read_device()
        b = read_host()
        assert all(x.equals(y) and x.equals(z) for x, y, z in zip(a, b, comps)), "the two conversions disagree"
        for arr in a + b:
            arr.free()
        assert interface.format_native(comps) == text
        copy_alone()
        dev_t, host_t, write_t, copy_t = [], [], [], []
        for _ in range(args.passes):
            dt, got = timed(read_device)
            dev_t.append(dt)
            for arr in got:
                arr.free()
            dt, got = timed(read_host)
            host_t.append(dt)
            for arr in got:
                arr.free()
        for _ in range(args.passes):
            write_t.append(timed(lambda: interface.format_native(comps))[0])
            copy_t.append(copy_alone())
        gap = statistics.median(host_t) - statistics.median(dev_t)
        spread = max(max(dev_t) - min(dev_t), max(host_t) - min(host_t))
        out += ["%s, N = %d: %d bytes a line, %.1f MB of text" % (title, args.n, B, len(text) / 1e6),
                line("(a) read, device (parse_native)", dev_t),
                line("(b) read, host (fromhex, numpy, raw parse)", host_t),
                line("(c) write, device (format_native)", write_t),
                line("(d) hipMemcpy of the text alone", copy_t),
                "    gap of the read medians (b) - (a): %.3f s; five times the larger spread: %.3f s -> %s"
                % (gap, 5 * spread, "the device path is faster" if gap > 5 * spread else
                   "the host path is faster" if -gap > 5 * spread else "no claim either way"),
                "    (a) reads %.2f GB/s of text, the copy alone moves %.2f GB/s"
                % (len(text) / statistics.median(dev_t) / 1e9, len(text) / statistics.median(copy_t) / 1e9), ""]
        print("\n".join(out[-7:]), flush=True)
        for arr in comps:
            arr.free()
        grp.close()
    with open(args.out, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
