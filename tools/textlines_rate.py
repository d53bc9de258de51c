#!/usr/bin/env python3
"""textlines_rate.py — plaintexts as text (messages encoded as group elements and decoded again), on the GPU against the obvious
host conversion, in one process.

  python tools/textlines_rate.py [-n 1000000] [--passes 3] [--host-sample 2000] [--out profiles/textlines_rate.txt]
                                 [--bench-ms PARENT THIS]

N messages of L = 251 bytes (the full encode length) over the 2048-bit safe-prime group at width 1, 256-byte leaves.  After one
untimed pass of each, --passes alternating passes of
  (a) encode, device:  interface.encode_texts(text)    (vmn_garrays_from_textlines: lines, records, import, one Jacobi symbol per
                       element), host clock around the call, which ends in a synchronisation: the upload of the text is inside;
  (b) decode, device:  interface.decode_texts(arrays)  (vmn_garrays_to_textlines: export, fold, UTF-8 verdict, compaction,
                       download);
  (c) the obvious host conversion with Python integers, both ways, on the first --host-sample messages and SCALED to N (it is
      too slow to run in full: the sample and the factor are stated): int.from_bytes of the framed message, pow(v, q, p) for the
      residue test, p - v, to_bytes of the wire width; and back min(e, p - e), to_bytes, the length word, bytes.decode, replace;
and, outside the alternation, --passes of
  (d) the floor:       the host-to-device copy of the text's bytes alone (hipMemcpy of the same pageable buffer).
Every time, the medians and the spreads (max - min) are written to --out, with the share of the kernel families in the GPU time
of one more encode pass under vmn_ctx_timing (the residue kernel is the family "encode_residue", the byte-level kernels
"textlines").  By the rule of profiles/README.md a path is called faster only if the gap of the medians exceeds five times the
larger spread.  --bench-ms records the two ms_per_step of bench.py (parent commit, this commit), measured apart."""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def line(label, xs):
    return "%-46s median %8.3f s  (min %8.3f  max %8.3f  spread %6.3f)  samples %s" % (
        label, statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), " ".join("%.3f" % x for x in xs))


def host_encode(lines, p, q, L, vb):
    out = []
    for m in lines:
        T = bytearray(len(m).to_bytes(4, "big") + m + bytes(L - len(m)))
        if not m:
            T[4] = 1
        v = int.from_bytes(T, "big")
        out.append((v if pow(v, q, p) == 1 else p - v).to_bytes(vb, "big"))
    return b"".join(out)


def host_decode(block, p, q, L, vb):
    out = []
    for i in range(0, len(block), vb):
        e = int.from_bytes(block[i:i + vb], "big")
        T = (e if e <= q else p - e).to_bytes(L + 4, "big")
        s = T[4:4 + int.from_bytes(T[:4], "big")].decode("utf-8", "replace")
        out.append(s.replace("\n", "").replace("\r", ""))
    return ("\n".join(out) + "\n").encode()


def message(i, L):
    """L bytes of text without line terminators: the line's number, then letters drawn from a hash."""
    body = hashlib.sha256(b"textlines-rate/%d" % i).hexdigest()
    return (("%09d " % i) + body * (L // len(body) + 1)).encode()[:L]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "textlines_rate.txt"))
    ap.add_argument("--bench-ms", type=float, nargs=2, metavar=("PARENT", "THIS"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import interface, stdgroups
    ctx = vmn.Context(0)
    hip = C.CDLL("libamdhip64.so")
    p, q, g = stdgroups.modp_group(2048)
    grp = vmn.ModPGroup(ctx, p, q, g, nbytes=256)
    L, vb, n = interface.encode_length(grp), grp.nbytes, args.n
    lines = [message(i, L) for i in range(n)]
    text = b"".join(m + b"\n" for m in lines)
    sample = min(args.host_sample, n)

    def encode_device():
        got = interface.encode_texts(grp, text)
        assert got is not None
        ctx.synchronize()
        return got

    def copy_alone():
        dev = C.c_void_p()
        assert hip.hipMalloc(C.byref(dev), C.c_size_t(len(text))) == 0
        t0 = time.perf_counter()
        assert hip.hipMemcpy(dev, text, C.c_size_t(len(text)), C.c_int(1)) == 0 and hip.hipDeviceSynchronize() == 0
        dt = time.perf_counter() - t0
        hip.hipFree(dev)
        return dt

    # the two conversions agree (on the sample), and the device inverts itself on the whole list
    arrays = encode_device()
    head = interface.encode_texts(grp, b"".join(m + b"\n" for m in lines[:sample]))
    block = host_encode(lines[:sample], p, q, L, vb)
    assert head[0].toBytes() == block, "the two encodings disagree"
    assert interface.decode_texts(arrays) == text and host_decode(block, p, q, L, vb) == text[:sample * (L + 1)]
    head[0].free()
    copy_alone()
    enc_t, dec_t, host_enc_t, host_dec_t, copy_t = [], [], [], [], []
    for _ in range(args.passes):
        dt, got = timed(encode_device)
        enc_t.append(dt)
        for a in got:
            a.free()
        dec_t.append(timed(lambda: interface.decode_texts(arrays))[0])
        host_enc_t.append(timed(lambda: host_encode(lines[:sample], p, q, L, vb))[0] * n / sample)
        host_dec_t.append(timed(lambda: host_decode(block, p, q, L, vb))[0] * n / sample)
    for _ in range(args.passes):
        copy_t.append(copy_alone())
    ctx.timing_enable(True)
    ctx.timing_reset()
    for a in encode_device():
        a.free()
    rep = ctx.timing_report()
    ctx.timing_enable(False)
    total = sum(v[1] for v in rep.values()) or 1.0
    shares = ", ".join("%s %.2f ms" % (k, v[1]) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1]))
    residue = rep.get("encode_residue", (0, 0.0))[1]

    def verdict(host, dev):
        gap = statistics.median(host) - statistics.median(dev)
        spread = max(max(dev) - min(dev), max(host) - min(host))
        return "gap of the medians %.3f s; five times the larger spread: %.3f s -> %s" % (
            gap, 5 * spread, "the device path is faster" if gap > 5 * spread else "the host path is faster" if -gap > 5 * spread
            else "no claim either way")

    out = ["== plaintexts as text: device against host conversion ==",
           "(tools/textlines_rate.py -n %d --passes %d --host-sample %d, one MI355X, one process, the passes alternating; wall time "
           "around the calls)" % (n, args.passes, sample), "",
           "2048-bit safe-prime group, 256-byte leaves, width 1, N = %d messages of L = %d bytes: %.1f MB of text" % (n, L, len(text) / 1e6),
           line("(a) encode, device (encode_texts)", enc_t),
           line("(b) decode, device (decode_texts)", dec_t),
           line("(c) encode, host, %d messages x %.0f" % (sample, n / sample), host_enc_t),
           line("(c) decode, host, %d messages x %.0f" % (sample, n / sample), host_dec_t),
           line("(d) hipMemcpy of the text alone", copy_t),
           "    encode: " + verdict(host_enc_t, enc_t),
           "    decode: " + verdict(host_dec_t, dec_t),
           "    (a) takes %.2f GB/s of text, (b) writes %.2f GB/s, the copy alone moves %.2f GB/s"
           % (len(text) / statistics.median(enc_t) / 1e9, len(text) / statistics.median(dec_t) / 1e9, len(text) / statistics.median(copy_t) / 1e9),
           "    GPU time of one encode pass by kernel family: %s; the residue kernel (encode_residue) = %.1f %% of %.2f ms"
           % (shares, 100 * residue / total, total), ""]
    if args.bench_ms:
        out += ["bench.py --gpus 1 (the headline, which calls none of this): ms_per_step %.3f on the parent commit, %.3f on this one"
                % tuple(args.bench_ms), ""]
    print("\n".join(out), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
