#!/usr/bin/env python3
"""point_texts_rate.py — plaintexts as text over a curve group (messages encoded as points and decoded again), on the GPU against
the host conversion by the restatement, in one process.

  python tools/point_texts_rate.py [-n 1000000] [--passes 3] [--host-sample 10000] [--curve P-256]
                                   [--out profiles/point_texts_rate.txt] [--bench-ms PARENT THIS]

N lines of ncomp L bytes (the full encode length: L = 26 over P-256) at ncomp = 1 and ncomp = 3, 32-byte coordinates.  Per ncomp,
after one untimed pass of each, --passes alternating passes of
  (a) encode, device:  interface.encode_point_texts(text)   (vmn_ec_arrays_from_textlines: lines, records, the counter search,
                       one square root per point), host clock around the call, which ends in a synchronisation: the upload of
                       the text is inside;
  (b) decode, device:  interface.decode_point_texts(arrays) (vmn_ec_arrays_to_textlines: export, fold, UTF-8 verdict, compaction,
                       download);
  (c) the host conversion by the restatement (tests/point_encode_cases.py, Python integers), both ways, on the first
      --host-sample lines and SCALED to N (it is too slow to run in full: the sample and the factor are stated);
and, outside the alternation, --passes of
  (d) the floor:       the host-to-device copy of the text's bytes alone (hipMemcpy of the same pageable buffer).
Every time, the medians and the spreads (max - min) are written to --out, with the GPU time of one more encode pass by kernel
family under vmn_ctx_timing ("encode_search", "encode_root", and "textlines" for the line finder and the records) and the
divergence of the search: the counters tried per record (accepted counter + 1, read from the x coordinates the device produced)
against the counters a wave of 64 consecutive records runs (its unluckiest lane's).  By the rule of profiles/README.md a path is
called faster only if the gap of the medians exceeds five times the larger spread.  --bench-ms records the two ms_per_step of
bench.py (parent commit, this commit), measured apart."""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return time.perf_counter() - t0, r


def line(label, xs):
    return "%-46s median %8.3f s  (min %8.3f  max %8.3f  spread %6.3f)  samples %s" % (
        label, statistics.median(xs), min(xs), max(xs), max(xs) - min(xs), " ".join("%.3f" % x for x in xs))


def message(i, nbytes):
    """nbytes of text without line terminators: the line's number, then letters drawn from a hash."""
    body = hashlib.sha256(b"point-texts-rate/%d" % i).hexdigest()
    return (("%09d " % i) + body * (nbytes // len(body) + 1)).encode()[:nbytes]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=1000000)
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=10000)
    ap.add_argument("--curve", default="P-256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_texts_rate.txt"))
    ap.add_argument("--bench-ms", type=float, nargs=2, metavar=("PARENT", "THIS"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import interface
    import point_encode_cases as pe
    ctx = vmn.Context(0)
    hip = C.CDLL("libamdhip64.so")
    grp = vmn.ECqPGroup(ctx, args.curve)
    name, L, vb, n = args.curve, interface.point_encode_length(grp), grp.nbytes, args.n
    sample = min(args.host_sample, n)
    out = ["== plaintexts as text over a curve group: device against host conversion ==",
           "(tools/point_texts_rate.py -n %d --passes %d --host-sample %d --curve %s, one MI355X, one process, the passes alternating; "
           "wall time around the calls)" % (n, args.passes, sample, name), ""]

    for ncomp in (1, 3):
        lines = [message(i, ncomp * L) for i in range(n)]
        text = b"".join(m + b"\n" for m in lines)
        head_text = text[:sample * (ncomp * L + 1)]

        def encode_device():
            got = interface.encode_point_texts(grp, text, ncomp)
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

        def host_encode():
            cols, _ = pe.encode_text(head_text, name, ncomp)
            return [pe.block(col, vb) for col in cols]

        def host_decode(blocks):
            cols = [[(int.from_bytes(b[i:i + vb], "big"), int.from_bytes(b[i + vb:i + 2 * vb], "big")) for i in range(0, len(b), 2 * vb)]
                    for b in blocks]
            return pe.decode_text(cols, name)[0]

        # the two conversions agree (on the sample), and the device inverts itself on the whole list
        arrays = encode_device()
        head = interface.encode_point_texts(grp, head_text, ncomp)
        blocks = host_encode()
        assert [a.toBytes() for a in head] == blocks, "the two encodings disagree"
        assert interface.decode_point_texts(arrays) == text and host_decode(blocks) == head_text
        for a in head:
            a.free()
        # the divergence of the search, from the counters in the x coordinates of the first component
        raw = arrays[0].toBytes()
        tried = [raw[i * 2 * vb + vb - 1] + 1 for i in range(n)]
        waves = [max(tried[i:i + 64]) for i in range(0, n, 64)]
        copy_alone()
        enc_t, dec_t, host_enc_t, host_dec_t, copy_t = [], [], [], [], []
        for _ in range(args.passes):
            dt, got = timed(encode_device)
            enc_t.append(dt)
            for a in got:
                a.free()
            dec_t.append(timed(lambda: interface.decode_point_texts(arrays))[0])
            pe.encode_piece.cache_clear()
            host_enc_t.append(timed(host_encode)[0] * n / sample)
            host_dec_t.append(timed(lambda: host_decode(blocks))[0] * n / sample)
        for _ in range(args.passes):
            copy_t.append(copy_alone())
        ctx.timing_enable(True)
        ctx.timing_reset()
        for a in encode_device():
            a.free()
        rep = ctx.timing_report()
        ctx.timing_enable(False)
        for a in arrays:
            a.free()
        total = sum(v[1] for v in rep.values()) or 1.0
        shares = ", ".join("%s %.2f ms" % (k, v[1]) for k, v in sorted(rep.items(), key=lambda kv: -kv[1][1]))

        def verdict(host, dev):
            gap = statistics.median(host) - statistics.median(dev)
            spread = max(max(dev) - min(dev), max(host) - min(host))
            return "gap of the medians %.3f s; five times the larger spread: %.3f s -> %s" % (
                gap, 5 * spread, "the device path is faster" if gap > 5 * spread else "the host path is faster" if -gap > 5 * spread
                else "no claim either way")

        out += ["%s, %d-byte coordinates, ncomp = %d, N = %d lines of %d bytes (%d points): %.1f MB of text"
                % (name, vb, ncomp, n, ncomp * L, ncomp * n, len(text) / 1e6),
                line("(a) encode, device (encode_point_texts)", enc_t),
                line("(b) decode, device (decode_point_texts)", dec_t),
                line("(c) encode, host, %d lines x %.0f (SCALED)" % (sample, n / sample), host_enc_t),
                line("(c) decode, host, %d lines x %.0f (SCALED)" % (sample, n / sample), host_dec_t),
                line("(d) hipMemcpy of the text alone", copy_t),
                "    encode: " + verdict(host_enc_t, enc_t),
                "    decode: " + verdict(host_dec_t, dec_t),
                "    (a) encodes %.2f x 10^6 points/s, (b) decodes %.2f x 10^6 points/s"
                % (ncomp * n / statistics.median(enc_t) / 1e6, ncomp * n / statistics.median(dec_t) / 1e6),
                "    GPU time of one encode pass by kernel family: %s; total %.2f ms" % (shares, total),
                "    counters tried per record (component 0): mean %.3f (the rule implies 2), max %d; per wave of 64 records: mean %.3f"
                % (statistics.mean(tried), max(tried), statistics.mean(waves)), ""]
    if args.bench_ms:
        out += ["bench.py --gpus 1 (the headline, which calls none of this): ms_per_step %.3f on the parent commit, %.3f on this one"
                % tuple(args.bench_ms), ""]
    print("\n".join(out), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out))


if __name__ == "__main__":
    main()
