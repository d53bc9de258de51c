#!/usr/bin/env python3
"""record_proofdir_sessions.py — the bytes of whole proof directories, pinned as digests.

  python tools/record_proofdir_sessions.py [--out tests/golden/proofdir_sessions.json]

Writes small sessions (K = 3 parties, threshold 2, N = 12 ciphertexts, N_0 = 16) with proofdir.write_session from
InsecureShaRandomSource tapes with fixed tags, verifies each with proofdir.verify_session, and records for every case the SHA-256
of every file of the directory, the SHA-256 of json.dumps(vectors, sort_keys=True) and the verdicts.  The writers draw all their
randomness from the tapes and the arithmetic is exact: two runs give the same file, before and after any change that is meant
to leave the directory byte for byte what it was.  Only the public names of proofdir are used.

Cases: the 512-bit golden group and P-256; (kappa, omega) in {(1,1), (1,2), (2,1), (2,2)}; mixing plain, mixing committed,
shuffling committed, decryption alone.  Over the 512-bit group at (2,2) also: a mixing session of three active parties whose
party 2 fails, plain and committed, and a decryption whose party 2 publishes a wrong reply (write_decryption's per-party branch).

tests/test_gpu_proofdir_recorded.py writes every case again and compares."""
import argparse
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

K, THR, N, N0 = 3, 2, 12, 16
SHAPES = [(1, 1), (1, 2), (2, 1), (2, 2)]
TYPES = {"mix": ("mixing", 0), "mixc": ("mixing", N0), "shufc": ("shuffling", N0), "dec": ("decryption", 0)}


def cases():
    """[(case id, group, kappa, omega, session type, N_0, active, failing, tampered reply)]"""
    out = []
    for group in ("modp512", "p256"):
        for kw, w in SHAPES:
            for name, (session_type, n0) in TYPES.items():
                out.append(("%s-k%dw%d-%s" % (group, kw, w, name), group, kw, w, session_type, n0, THR, (), False))
    out.append(("modp512-k2w2-mix-failing2", "modp512", 2, 2, "mixing", 0, 3, (2,), False))
    out.append(("modp512-k2w2-mixc-failing2", "modp512", 2, 2, "mixing", N0, 3, (2,), False))
    out.append(("modp512-k2w2-dec-reply2", "modp512", 2, 2, "decryption", 0, THR, (), True))
    return out


def groups(vmn, ctx):
    """{name: (group, params without the session's own entries)}"""
    with open(os.path.join(ROOT, "tests", "golden", "modp512.json")) as f:
        rec = json.load(f)["group"]
    p, q, g = (int(rec[name], 16) for name in ("p", "q", "g"))
    base = {"version": "3.1.0", "sid": "SessionID", "auxsid": "default", "rbitlen": 100, "vbitlenro": 256, "ebitlenro": 256,
            "prg": "SHA-256", "rohash": "SHA-256", "rohash_name": "SHA-256"}
    return {"modp512": (vmn.ModPGroup(ctx, p, q, g),
                        dict(base, pgroup="ModPGroup(512)", group={"kind": "modp", "p": rec["p"], "q": rec["q"], "g": rec["g"]})),
            "p256": (vmn.ECqPGroup(ctx, "P-256", java_widths=True),
                     dict(base, pgroup="ECqPGroup(P-256)", group={"kind": "ec", "curve": "P-256"}))}


def sha(data: bytes) -> str:
    return hashlib.sha256(data).hexdigest()


def digests(nizkp):
    out = {}
    for base, _, names in os.walk(nizkp):
        for name in names:
            path = os.path.join(base, name)
            with open(path, "rb") as f:
                out[os.path.relpath(path, nizkp).replace(os.sep, "/")] = sha(f.read())
    return dict(sorted(out.items()))


def record(pd, rs, group, case, nizkp):
    """Write the session of `case` into nizkp, verify it, and return its record."""
    name, _, kw, w, session_type, n0, active, failing, tampered = case
    G, params = group
    q, g = G.q, G.g
    tag = name.encode()
    tape = rs.InsecureShaRandomSource(tag + b"-tape", q)
    coeffs = [tape.ring_array(THR) for _ in range(kw)]
    share = lambda j, l: sum(c * pow(l, d, q) for d, c in enumerate(coeffs[j])) % q
    rows = (lambda x: tuple(x)) if kw > 1 else (lambda x: x[0])                  # at key width 1 the interface takes the scalars
    shares = [None] + [rows([share(j, l) for j in range(kw)]) for l in range(1, K + 1)]
    poly = [rows([G.k_exp(g, coeffs[j][d]) for j in range(kw)]) for d in range(THR)]
    y = [G.k_exp(g, coeffs[j][0]) for j in range(kw)]
    T = [G.ringArray(tape.ring_array(N)) for _ in range(kw * w)]
    M = [G.exp(g, G.ringArray(tape.ring_array(N))) for _ in range(kw * w)]
    W = [G.exp(g, t) for t in T] + [m.mul(G.exp(y[c % kw], t)) for c, (m, t) in enumerate(zip(M, T))]
    written, _ = pd.write_session(nizkp, G, params, session_type, W, rows(y), rs.InsecureShaRandomSource(tag + b"-prover", q), K, THR,
                                  active=active, n0=n0, failing=failing, poly=poly, shares=shares, keywidth=kw)
    if tampered:
        wrong = lambda l, kx: kx if l != 2 else (kx[0], (kx[1] + 1) % q) if kw > 1 else (kx + 1) % q
        pkey = [g] * (kw * w) + y * w
        pd.write_decryption(nizkp, G, written, pkey, W, poly, shares, rs.InsecureShaRandomSource(tag + b"-again", q), K, THR,
                            keywidth=kw, tamper_reply=wrong)
    tv = {}
    v = pd.verify_session(nizkp, G, written, vectors=tv)
    return {"files": digests(nizkp), "vectors": sha(json.dumps(tv, sort_keys=True).encode()),
            "accepted": v.accepted, "verdicts": v.verdicts, "replaced": sorted(v.replaced), "valid_proofs": v.valid_proofs,
            "decryption": v.decryption, "correct": v.correct}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "proofdir_sessions.json"))
    args = ap.parse_args()
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import proofdir, randomsource
    grps = groups(vmn, vmn.Context(0))
    out = {}
    for case in cases():
        t0 = time.perf_counter()
        with tempfile.TemporaryDirectory(prefix="record_") as nizkp:
            out[case[0]] = record(proofdir, randomsource, grps[case[1]], case, os.path.join(nizkp, "nizkp"))
        print("%-32s %6.2f s  %2d files  accepted %s" % (case[0], time.perf_counter() - t0, len(out[case[0]]["files"]), out[case[0]]["accepted"]),
              flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
