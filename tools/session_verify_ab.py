#!/usr/bin/env python3
"""session_verify_ab.py — proofdir.verify_session against the sequence of single-link calls it replaces, in one process.

  python tools/session_verify_ab.py [-n 100000] [--bits 2048] [--passes 5]

Writes a mixing session (k = 3 parties, threshold 2, both active, width 1) over the --bits safe-prime group with
proofdir.write_session, then alternates --passes times between
  (a) verify_session(directory), and
  (b) what a caller had before it: verify_shuffle for l = 1, 2, then verify_decryption of proofs/Ciphertexts02.bt,
wall-clock around the calls, after one untimed pass of each; then the same with VMN_SESSION_HASH_AHEAD=0.  Both sides check the
same proofs on the same files; (b) derives the generators, exports their tree and imports the previous list once per party.

Output: profiles/session_verify_ab.txt."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K, THR = 3, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-n", type=int, default=100000)
    ap.add_argument("--bits", type=int, default=2048)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_verify_ab.txt"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import proofdir, randomsource, stdgroups
    ctx = vmn.Context(0)
    p, q, g = stdgroups.modp_group(args.bits)
    grp = vmn.ModPGroup(ctx, p, q, g)
    params = {"version": "3.1.0", "sid": "SessionAB", "auxsid": "default", "rbitlen": 100, "vbitlenro": 256, "ebitlenro": 256,
              "prg": "SHA-256", "rohash": "SHA-256", "rohash_name": "SHA-256",
              "pgroup": f"ModPGroup(safe-prime modulus=2*order+1. order bit-length = {args.bits - 1})"}
    rnd = randomsource.InsecureShaRandomSource(b"session-ab", q)
    coeffs = rnd.ring_array(THR)
    shares = [None] + [sum(c * pow(l, d, q) for d, c in enumerate(coeffs)) % q for l in range(1, K + 1)]
    poly = [grp.k_exp(g, c) for c in coeffs]
    y = poly[0]
    T = grp.ringArray(rnd.ring_array(args.n))
    M = grp.exp(g, grp.ringArray(rnd.ring_array(args.n)))
    W = [grp.exp(g, T), M.mul(grp.exp(y, T))]
    nizkp = tempfile.mkdtemp(prefix="session_ab_")
    try:
        t0 = time.perf_counter()
        params, _ = proofdir.write_session(nizkp, grp, params, proofdir.MIX_TYPE, W, y, randomsource.SecureRandomSource(q, ctx=ctx), K, THR,
                                           poly=poly, shares=shares)
        print(f"wrote the session in {time.perf_counter() - t0:.1f} s", flush=True)
        pkey = [g, y]

        def session():
            v = proofdir.verify_session(nizkp, grp, params)
            assert v.accepted and v.verdicts == [True, True], v

        def links():
            assert proofdir.verify_shuffle(nizkp, 1, grp, params, pkey)
            assert proofdir.verify_shuffle(nizkp, 2, grp, params, pkey)
            assert proofdir.verify_decryption(nizkp, grp, params, pkey, proofdir.l_file(nizkp, 2))

        def timed(fn):
            t = time.perf_counter()
            fn()
            ctx.synchronize()
            return time.perf_counter() - t
        rows = []
        for mode in ("1", "0"):
            os.environ["VMN_SESSION_HASH_AHEAD"] = mode
            session()
            links()
            a, b = [], []
            for _ in range(args.passes):
                a.append(timed(session))
                b.append(timed(links))
                print(f"hash ahead {mode}: session {a[-1]:.3f} s, links {b[-1]:.3f} s", flush=True)
            rows.append((mode, a, b))
    finally:
        shutil.rmtree(nizkp, ignore_errors=True)
    fmt = lambda xs: f"median {statistics.median(xs):8.3f} s  (min {min(xs):8.3f}  max {max(xs):8.3f})  samples " + " ".join(f"{x:.3f}" for x in xs)
    lines = [f"== verify_session against verify_shuffle x 2 + verify_decryption on the same directory ==",
             f"(tools/session_verify_ab.py -n {args.n} --bits {args.bits} --passes {args.passes}, one MI355X, one process)",
             "",
             f"a mixing session over the {args.bits}-bit safe-prime group, k = {K}, threshold {THR}, both parties active, width 1, N = {args.n};",
             f"{args.passes} alternating passes after one untimed pass of each, wall time around the calls up to a device synchronisation"]
    for mode, a, b in rows:
        lines += ["", f"VMN_SESSION_HASH_AHEAD={mode}" + ("  (the default: seeds of later parties hashed on worker threads)" if mode == "1" else "  (every seed hashed where it is needed)"),
                  "(a) verify_session                        " + fmt(a),
                  "(b) verify_shuffle x 2, verify_decryption " + fmt(b),
                  f"    (a) / (b) at the medians: {statistics.median(a) / statistics.median(b):.3f};  spread of (b): {max(b) - min(b):.3f} s"]
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
