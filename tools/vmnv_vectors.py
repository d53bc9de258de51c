#!/usr/bin/env python3
"""vmnv_vectors.py — verify the shuffle of party l in a proof directory on the GPU and print the test vectors the reference's
standalone verifier prints under `vmnv -t` (mixnet/MixNetElGamalVerifyFiatShamirSession.java:843-937; names and descriptions:
MixNetElGamalVerifyFiatShamirTool.java:82-223; output format `\\nTEST VECTOR\\n<name> - <description>\\n<value>`,
MixNetElGamalVerifyFiatShamir.java:382-388).

    python tools/vmnv_vectors.py <nizkp dir> [-l PARTY] [-t der.rho,PoS] [--arrays]
    python tools/vmnv_vectors.py --demo <new dir> [-n 100]      write a directory with the C++ prover first (synthetic list)
    python tools/vmnv_vectors.py <nizkp dir> -decrypt [--list FILE]      the decryption branch (:1545-1667): Dec.s, Dec.v
    python tools/vmnv_vectors.py --demo <new dir> -decrypt [--width 3] [--parties 3] [--threshold 2]
    python tools/vmnv_vectors.py --demo <new dir> --curve P-256 [--precomputed N_0 | -decrypt]     the same over a named curve
    python tools/vmnv_vectors.py <nizkp dir> -session [-mix | -shuffle | -decrypt] [-auxsid SID] [-width W] [-nopos | -noposc | -noccpos]
                                 [-nodec] [-t par,der,bas,PoS] [--arrays]        the WHOLE directory, as `vmnv` verifies it
    python tools/vmnv_vectors.py --demo <new dir> -session [-mix | -shuffle | -decrypt] [--parties 3] [--threshold 2] [--active 2]
                                 [--width 1] [--keywidth 1] [--precomputed N_0] [--curve NAME]

-session is MixNetElGamalVerifyFiatShamirSession.verify (:1318-1670) through proofdir.verify_session; the options have the meaning of
MixNetElGamalVerifyFiatShamirTool.java:562-640, 1015-1044 (expected auxsid "default", expected width 0 = the width of params.json,
unless given; without -mix / -shuffle / -decrypt the type is taken from the proof).  It prints the TEST VECTOR blocks in the order
of the session, the per-party ones between the reference's BEGIN PARTY / END PARTY banners, one line per party and the result;
exit status 0: accepted, 1: rejected, 2: the directory is not a session that can be verified (SessionFormatError).  The width
of the public key (the protocol info's keywidth) is params.json's "keywidth", 1 when it has none; --demo --keywidth K writes a
session under a key of width K, whose lists have 2 K W component arrays.

The directory layout is the reference's (verificatum-vmn_amd/proofdir.py); what `vmnv` reads from the protocol-info XML is
in <dir>/params.json.  THE diff that would pin parity: on a machine with a JDK + VCR, run `vmnv -t der.rho,PoS ...` on a proof
directory the Java mix-net wrote, run this tool on the same directory, and compare the values name by name (VCR's
toString() of group elements is not part of the reference tree; this tool prints hexadecimal, a curve point as (x, y)).  Over
a curve, params.json's "pgroup" (the group's description string that goes into der.rho) is a placeholder: VCR's own description
string of an ECqPGroup is not in the reference tree and must be pasted in by whoever diffs against `vmnv`."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DESCRIPTIONS = {                      # MixNetElGamalVerifyFiatShamirTool.java:82-223
    "der.rho": "Derived prefix bytes to all random oracle queries.", "bas.h": "Independent generators.",
    "PoS.s": "PoS. Seed to derive batching vector in hexadecimal notation.",
    "PoS.v": "PoS. Integer challenge in hexadecimal notation.", "PoS.A": "PoS. Batched permutation commitment.",
    "PoS.F": "PoS. Batched input ciphertexts.", "PoS.B": "PoS. Commitment components.",
    "PoS.C": "PoS. Derived intermediate values.", "PoS.D": "PoS. Derived intermediate values.",
    "PoS.Ap": "PoS. Commitment components.", "PoS.Bp": "PoS. Commitment components.", "PoS.Cp": "PoS. Commitment components.",
    "PoS.Dp": "PoS. Commitment components.", "PoS.Fp": "PoS. Commitment components.", "PoS.k_A": "PoS. Reply components.",
    "PoS.k_B": "PoS. Reply components.", "PoS.k_C": "PoS. Reply components.", "PoS.k_D": "PoS. Reply components.",
    "PoS.k_E": "PoS. Reply components.", "PoS.k_F": "PoS. Reply components.",
    "PoSC.s": "PoSC. Seed to derive batching vector in hexadecimal notation.",
    "PoSC.v": "PoSC. Integer challenge in hexadecimal notation.",
    "CCPoS.s": "CCPoS. Seed to derive batching vector in hexadecimal notation.",
    "CCPoS.v": "CCPoS. Integer challenge in hexadecimal notation.",
    # not registered by the reference (private fields of its classes): printed for diffing two builds of THIS code
    "PoSC.A": "[not in the reference] PoSC. Batched permutation commitment.", "PoSC.C": "[not in the reference] PoSC. Derived intermediate values.",
    "PoSC.D": "[not in the reference] PoSC. Derived intermediate values.", "CCPoS.A": "[not in the reference] CCPoS. Batched permutation commitment.",
    "CCPoS.B": "[not in the reference] CCPoS. Batched input ciphertexts.",
    "Dec.s": "Dec. Seed to derive batching vector in hexadecimal notation.", "Dec.v": "Dec. Integer challenge in decimal notation."}
DESCRIPTIONS.update({             # MixNetElGamalVerifyFiatShamirTool.java:82-150
    "par.version": "Version.", "par.sid": "Session identifier of mix-net.", "par.k": "Number of mix-servers.",
    "par.lambda": "Threshold number of parties needed to decrypt.",
    "par.n_e": "Bit length of components in random vectors used for batching.", "par.n_r": "Bit length of random paddings.",
    "par.n_v": "Bit length of challenges.", "par.s_PRG": "Description of PRG used for batching.",
    "par.s_Gq": "Description of underlying group.", "par.s_H": "Description of hash function used to implement random oracles.",
    "par.omega": "Width of ciphertexts.", "par.N_0": "Number of ciphertexts for which precomputation is done.",
    "bas.pk": "Joint public key.", "bas.y_l": "Public keys of threshold number of mix-servers.",
    "bas.L_0": "Original list of ciphertexts.", "bas.L_l": "Intermediate list of ciphertexts.", "u": "Permutation commitment."})
# the order in which MixNetElGamalVerifyFiatShamirSession.verify prints (:1322-1389); the active threshold is printed under the
# name par.lambda a second time (:498)
SESSION_HEAD = ["par.k", "par.lambda", "par.n_e", "par.n_r", "par.n_v", "par.s_PRG", "par.s_Gq", "par.s_H", "par.version", "par.omega",
                "bas.pk", "bas.y_l", "par.sid", "der.rho", "par.lambda.active", "bas.L_0", "par.N_0", "bas.h"]
ORDER = ["der.rho", "bas.h", "PoSC.s", "PoSC.v", "PoSC.A", "PoSC.C", "PoSC.D", "CCPoS.s", "CCPoS.A", "CCPoS.B", "CCPoS.v",
         "PoS.s", "PoS.A", "PoS.F", "PoS.B", "PoS.Ap", "PoS.Bp", "PoS.Cp", "PoS.Dp", "PoS.Fp", "PoS.v", "PoS.C",
         "PoS.D", "PoS.k_A", "PoS.k_B", "PoS.k_C", "PoS.k_D", "PoS.k_E", "PoS.k_F", "Dec.s", "Dec.v"]


def selected(name, wanted):
    """checkTestVector (MixNetElGamalVerifyFiatShamir.java:397-409): the name itself or its prefix before the dot."""
    return name in wanted or name.split(".")[0] in wanted


def group_of(vmn, ctx, params):
    if params["group"]["kind"] == "modp":
        g = params["group"]
        return vmn.ModPGroup(ctx, int(g["p"], 16), int(g["q"], 16), int(g["g"], 16))
    return vmn.ECqPGroup(ctx, params["group"]["curve"], java_widths=True)


def key_elements(tree, points):
    """The encodings of the 2 * width elements of a public key's tree node(u-half, v-half), in order.  An element is a leaf, over
    a curve (`points`) the node of its two coordinate leaves."""
    if isinstance(tree, list) and not (points and len(tree) == 2 and all(isinstance(c, bytes) for c in tree)):
        return [e for child in tree for e in key_elements(child, points)]
    return [b"".join(tree) if isinstance(tree, list) else tree]


def demo_params(args, stdgroups, **more):
    """params.json of a demo directory: the 2^(--bits) safe-prime group, or the curve --curve."""
    params = {"version": "3.1.0", "sid": "MyDemo", "auxsid": "default", "rbitlen": 100, "vbitlenro": 256, "ebitlenro": 256,
              "prg": "SHA-256", "rohash": "SHA-256", "rohash_name": "SHA-256"}
    params.update(more)
    if args.curve:
        params["pgroup"] = f"ECqPGroup({args.curve})"        # a placeholder: see the module's docstring
        params["group"] = {"kind": "ec", "curve": args.curve}
    else:
        p, q, g = stdgroups.modp_group(args.bits)
        params["pgroup"] = f"ModPGroup(safe-prime modulus=2*order+1. order bit-length = {args.bits - 1})"
        params["group"] = {"kind": "modp", "p": format(p, "x"), "q": format(q, "x"), "g": format(g, "x")}
    return params


def demo_decryption(args, vmn, ctx, proofdir, randomsource, stdgroups):
    """A synthetic list of width --width under a key shared among --parties parties (threshold --threshold), decrypted by
    proofdir.write_decryption with every party played here."""
    k, thr, width = args.parties, args.threshold, args.width
    params = demo_params(args, stdgroups, width=width, k=k, threshold=thr)
    grp = group_of(vmn, ctx, params)
    q, g = grp.q, grp.g
    rnd = randomsource.InsecureShaRandomSource(b"vmnv-demo-decrypt", q)
    coeffs = rnd.ring_array(thr)
    shares = [None] + [sum(c * pow(l, d, q) for d, c in enumerate(coeffs)) % q for l in range(1, k + 1)]
    poly = [grp.k_exp(g, c) for c in coeffs]
    pkey = [g] * width + [poly[0]] * width
    T = [grp.ringArray(rnd.ring_array(args.n)) for _ in range(width)]
    M = [grp.exp(g, grp.ringArray(rnd.ring_array(args.n))) for _ in range(width)]
    W = [grp.exp(g, t) for t in T] + [m.mul(grp.exp(poly[0], t)) for m, t in zip(M, T)]
    proofdir.write_inputs(args.nizkp, grp, params, pkey, W)
    proofdir.write_decryption(args.nizkp, grp, params, pkey, W, poly, shares, randomsource.SecureRandomSource(q), k, thr)
    print(f"wrote {args.nizkp}: {args.n} ciphertexts of width {width}, {k} parties, threshold {thr}", file=sys.stderr)


def block(name, value, printed_as=None):
    print(f"\nTEST VECTOR\n{printed_as or name} - {DESCRIPTIONS[name]}\n{value}")


def demo_session(args, vmn, ctx, proofdir, randomsource, stdgroups):
    """A synthetic list of -n ciphertexts of width --width, mixed / shuffled / decrypted by --parties parties (threshold
    --threshold, --active of them shuffling) through proofdir.write_session."""
    k, thr, width, kw = args.parties, args.threshold, args.width, args.keywidth
    params = demo_params(args, stdgroups)
    grp = group_of(vmn, ctx, params)
    q, g = grp.q, grp.g
    rnd = randomsource.InsecureShaRandomSource(b"vmnv-demo-session", q)
    coeffs = [rnd.ring_array(thr) for _ in range(kw)]                       # one polynomial per row of the key
    share = lambda j, l: sum(c * pow(l, d, q) for d, c in enumerate(coeffs[j])) % q
    rows = lambda f: f(0) if kw == 1 else tuple(f(j) for j in range(kw))    # an element of G^kw / Z_q^kw: its rows, the row itself at 1
    shares = [None] + [rows(lambda j: share(j, l)) for l in range(1, k + 1)]
    poly = [rows(lambda j: grp.k_exp(g, coeffs[j][d])) for d in range(thr)]
    y = [grp.k_exp(g, coeffs[j][0]) for j in range(kw)]
    T = [grp.ringArray(rnd.ring_array(args.n)) for _ in range(kw * width)]
    M = [grp.exp(g, grp.ringArray(rnd.ring_array(args.n))) for _ in range(kw * width)]
    W = [grp.exp(g, t) for t in T] + [m.mul(grp.exp(y[c % kw], t)) for c, (m, t) in enumerate(zip(M, T))]
    typ = proofdir.SHUFFLE_TYPE if args.shuffle else proofdir.DECRYPT_TYPE if args.decrypt else proofdir.MIX_TYPE
    proofdir.write_session(args.nizkp, grp, params, typ, W, poly[0], randomsource.SecureRandomSource(q, ctx=ctx), k, thr,
                           active=args.active or thr, n0=args.precomputed, poly=poly, shares=shares, keywidth=kw)
    print(f"wrote {args.nizkp}: a {typ} session, {args.n} ciphertexts of width {width}, key width {kw}, {k} parties, threshold {thr}",
          file=sys.stderr)


def session_main(args, vmn, ctx, proofdir):
    import json
    with open(os.path.join(args.nizkp, proofdir.PARAMS)) as f:
        params = json.load(f)
    grp = group_of(vmn, ctx, params)
    pos = not args.nopos
    expected = proofdir.SessionParams(
        type=proofdir.MIX_TYPE if args.mix else proofdir.SHUFFLE_TYPE if args.shuffle else proofdir.DECRYPT_TYPE if args.decrypt else None,
        auxsid=args.auxsid, width=args.expected_width, dec=not args.nodec, posc=pos and not args.noposc, ccpos=pos and not args.noccpos)
    wanted = set(("par,der,bas,PoS,PoSC,CCPoS,Dec" if args.t == "der,PoS" else args.t).split(","))
    vectors = {}
    try:
        verdict = proofdir.verify_session(args.nizkp, grp, params, expected, vectors, with_arrays=args.arrays)
    except proofdir.SessionFormatError as err:
        print(f"\nthe directory can not be verified: {err}")
        sys.exit(2)
    for name in SESSION_HEAD:
        if name in vectors and selected(name, wanted):
            if name == "par.lambda.active":
                block("par.lambda", vectors[name])
            else:
                block(name, vectors[name])
    for l in range(1, verdict.active_threshold + 1 if verdict.parties else 1):
        tv = vectors.get("party", {}).get(l)
        if tv is not None:
            if "PoS" in wanted:                   # checkPrintTestShuffleBegin("PoS", l)  MixNetElGamalVerifyFiatShamir.java:346-351
                print(f"\n###################### BEGIN PARTY {l} ######################")
            for name in ["u"] + [n for n in ORDER if n.startswith("PoSC.")] + ["bas.L_l"] + [n for n in ORDER if n.startswith(("CCPoS.", "PoS."))]:
                if name in tv and selected(name, wanted):
                    block(name, tv[name], f"bas.L_{l}" if name == "bas.L_l" else None)
        if "PoS" in wanted:                       # printTestShuffleEnd, for every l (:1515-1517)
            print(f"\n####################### END PARTY {l} #######################")
    for name in ("Dec.s", "Dec.v"):
        if name in vectors and selected(name, wanted):
            block(name, vectors[name])
    print()
    for p in verdict.parties:
        failed = [n for n, ok in (("PoSC", p.posc), ("CCPoS", p.ccpos), ("PoS", p.pos)) if ok is False]
        print(f"party {p.l}: {'valid' if p.verdict else 'INVALID (' + ', '.join(failed) + ')'}" +
              ("; its output was replaced by its input" if p.replaced else ""))
    if verdict.params.posc or verdict.params.ccpos:
        print(f"valid proofs: {verdict.valid_proofs} (threshold {params['threshold']})")
    if verdict.decryption is not None:
        print(f"decryption: {'valid' if verdict.decryption else 'INVALID'}; correct indices {verdict.correct}")
    print(f"verdict of the {verdict.params.type} session: {'accepted' if verdict.accepted else 'REJECTED'}")
    sys.exit(0 if verdict.accepted else 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("nizkp")
    ap.add_argument("-l", type=int, default=1)
    ap.add_argument("-t", default="der,PoS", help="comma-separated test vector names (a prefix selects its group)")
    ap.add_argument("--arrays", action="store_true", help="also the N-sized vectors (bas.h, PoS.B, PoS.Bp, PoS.k_B, PoS.k_E)")
    ap.add_argument("--demo", action="store_true", help="write the directory first: synthetic list, C++ prover")
    ap.add_argument("-n", type=int, default=100)
    ap.add_argument("--precomputed", type=int, default=0, metavar="N_0",
                    help="the directory holds a PRECOMPUTED shuffle for N_0 ciphertexts (PoSC + keep list + CCPoS files) instead of a PoS; "
                         "with --demo: write one (N_0 >= n)")
    ap.add_argument("--bits", type=int, default=2048)
    ap.add_argument("--curve", default=None, metavar="NAME",
                    help="--demo: write the directory over this named curve (P-256, secp256k1, P-521, ...) instead of a modular group; "
                         "params.json then records {kind: ec, curve: NAME}.  Its \"pgroup\" string is a placeholder: VCR's own "
                         "description string of an ECqPGroup is not in the reference tree and must be pasted in by whoever diffs against vmnv")
    ap.add_argument("-decrypt", "--decrypt", dest="decrypt", action="store_true",
                    help="verify the threshold decryption of a list instead of a shuffle; with --demo: write one")
    ap.add_argument("--list", default=None, help="-decrypt: the decrypted list (default: Ciphertexts.bt of the directory)")
    ap.add_argument("--width", type=int, default=1, help="--demo -decrypt: width of the ciphertexts")
    ap.add_argument("--keywidth", type=int, default=1, help="--demo -session: width of the public key (written to params.json)")
    ap.add_argument("--parties", type=int, default=3, help="--demo -decrypt: number of parties k")
    ap.add_argument("--threshold", type=int, default=2, help="--demo -decrypt: parties needed to decrypt")
    ap.add_argument("-session", "--session", dest="session", action="store_true",
                    help="verify the whole directory as `vmnv` does: session files, keys, every active party, the decryption")
    ap.add_argument("-mix", dest="mix", action="store_true", help="-session: check a proof of mixing")
    ap.add_argument("-shuffle", dest="shuffle", action="store_true", help="-session: check a proof of a shuffle")
    ap.add_argument("-auxsid", dest="auxsid", default="default", help="-session: the expected auxiliary session identifier")
    ap.add_argument("-width", dest="expected_width", type=int, default=0,
                    help="-session: the expected width (default: the width of params.json; negative: the width of the proof)")
    ap.add_argument("-nopos", dest="nopos", action="store_true", help="-session: do not verify the shuffles")
    ap.add_argument("-noposc", dest="noposc", action="store_true", help="-session: do not verify the proofs of shuffles of commitments")
    ap.add_argument("-noccpos", dest="noccpos", action="store_true", help="-session: do not verify the commitment-consistent proofs")
    ap.add_argument("-nodec", dest="nodec", action="store_true", help="-session: do not verify the decryption")
    ap.add_argument("--active", type=int, default=0, help="--demo -session: parties that shuffle (default: --threshold)")
    args = ap.parse_args()
    if args.session and args.nopos and (args.noposc or args.noccpos):
        ap.error('the option "-nopos" is incompatible with both "-noposc" and "-noccpos"')
    import json
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import proofdir, randomsource, stdgroups
    ctx = vmn.Context(0)
    if args.session:
        if args.demo:
            demo_session(args, vmn, ctx, proofdir, randomsource, stdgroups)
        session_main(args, vmn, ctx, proofdir)
    if args.demo and args.decrypt:
        demo_decryption(args, vmn, ctx, proofdir, randomsource, stdgroups)
    elif args.demo:
        params = demo_params(args, stdgroups, width=1)
        grp = group_of(vmn, ctx, params)
        q, g = grp.q, grp.g
        rnd = randomsource.InsecureShaRandomSource(b"vmnv-demo", q)
        y = grp.k_exp(g, rnd.ring_element())
        pkey = [g, y]
        T = grp.ringArray(rnd.ring_array(args.n))
        M = grp.exp(g, grp.ringArray(rnd.ring_array(args.n)))
        W = [grp.exp(g, T), M.mul(grp.exp(y, T))]
        params["N_0"] = args.precomputed
        proofdir.write_inputs(args.nizkp, grp, params, pkey, W)
        prover = randomsource.SecureRandomSource(q, ctx=ctx)
        if args.precomputed:
            pi, R, U, H = proofdir.write_precomputation(args.nizkp, args.l, grp, params, args.precomputed, prover)
            proofdir.write_committed_shuffle(args.nizkp, args.l, grp, params, pkey, W, prover, pi, R, U, H)
        else:
            proofdir.write_shuffle(args.nizkp, args.l, grp, params, pkey, W, prover)
        print(f"wrote {args.nizkp}: {args.n} ciphertexts, party {args.l}", file=sys.stderr)
    with open(os.path.join(args.nizkp, proofdir.PARAMS)) as f:
        params = json.load(f)
    grp = group_of(vmn, ctx, params)
    from verificatum_vmn_amd import eio
    with open(proofdir.pk_file(args.nizkp), "rb") as f:
        tree, _ = eio.decode(f.read())
    pkey = [grp.dec_el(b) for b in key_elements(tree, grp.coord_bytes is not None)]
    vectors = {}
    n0 = args.precomputed or int(params.get("N_0", 0))
    if args.decrypt:
        verdict = proofdir.verify_decryption(args.nizkp, grp, params, pkey, args.list or proofdir.l_file(args.nizkp, 0), vectors)
        for name in sorted(v for v in vectors if v.startswith("Dec.y_")):
            print(f"\nTEST VECTOR\n{name} - [not in the reference] Dec. Public key share of a party.\n{vectors[name]}")
        for name in ("Dec.s", "Dec.v"):
            if name in vectors:
                print(f"\nTEST VECTOR\n{name} - {DESCRIPTIONS[name]}\n{vectors[name]}")
        print(f"\nverdict of the decryption: {'accepted' if verdict else 'REJECTED'}")
        sys.exit(0 if verdict else 1)
    if n0:
        verdict = proofdir.verify_precomputed_shuffle(args.nizkp, args.l, grp, params, pkey, n0, vectors)
        if args.t == "der,PoS":
            args.t = "der,PoSC,CCPoS"
    else:
        verdict = proofdir.verify_shuffle(args.nizkp, args.l, grp, params, pkey, vectors, with_arrays=args.arrays)
    wanted = set(args.t.split(","))
    for name in ORDER:
        if name in vectors and selected(name, wanted):
            print(f"\nTEST VECTOR\n{name} - {DESCRIPTIONS[name]}\n{vectors[name]}")
    print(f"\nverdict of party {args.l}: {'accepted' if verdict else 'REJECTED'}" +
          (f"   verdicts(A,B,C,D,F) = {vectors['verdicts(A,B,C,D,F)']}" if "verdicts(A,B,C,D,F)" in vectors else ""))
    sys.exit(0 if verdict else 1)


if __name__ == "__main__":
    main()
