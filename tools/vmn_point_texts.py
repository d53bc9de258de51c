#!/usr/bin/env python3
"""vmn_point_texts.py — plaintexts as text over a curve group: the reference's `vmnc -plain -outi native in out` for a
curve session, and the way back.

  python tools/vmn_point_texts.py -decode [-width W] [-keywidth K] (--curve NAME | --params FILE) [--wire java|natural] IN OUT
  python tools/vmn_point_texts.py -encode [-width W] [-keywidth K] (--curve NAME | --params FILE) [--wire java|natural] IN OUT

-decode reads the raw array tree of the K W plaintext components a session left behind (Plaintexts.bt) and writes one line of
text per plaintext: the messages of its components one after the other, \\n and \\r removed, then \\n
(ProtocolElGamalInterfaceString.decodePlaintexts).  A point that holds no message gives an empty piece, a line that is not
well-formed UTF-8 is written byte for byte; both are noted on stderr and do not change the exit status.
-encode reads lines of text (ended by \\n, \\r or \\r\\n; an empty line is the empty message) and writes the raw array tree of
the K W components that hold them, at most K W L bytes per line, L the group's encode length over curves (26 over P-256).
The group is one of the reference's named curves, or the one a proof directory's params.json names (--params), at the
reference's leaf widths (--wire java, the default) or at the bytes of the field prime.  Messages are encoded as points here
(csrc/ec_encode_layout.h): a --params file that names a modular group is a usage error -- tools/vmn_texts.py serves those.
The lists are converted on the GPU (verificatum_vmn_amd.interface: encode_point_texts, decode_point_texts).

Exit status: 0 converted; 1 IN is no such list (-decode) or a line is too long (-encode: the line is named, counted from 1, on
stderr), no output is written; 2 usage; 3 no GPU (there is no host conversion to fall back to)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        self.print_usage(sys.stderr)
        sys.stderr.write("%s: %s\n" % (self.prog, message))
        sys.exit(2)


def _curve_of_params(ap, path):
    try:
        with open(path) as f:
            rec = json.load(f)["group"]
        if rec["kind"] != "ec":
            ap.error("messages are encoded as points over curve groups only (tools/vmn_texts.py takes a modular group)")
        name = rec["curve"]
        if not isinstance(name, str):
            raise ValueError("the curve is no name")
        return name
    except (OSError, ValueError, KeyError, TypeError) as e:
        ap.error("%s names no group (%s)" % (path, e))


def main(argv=None):
    ap = _Parser(prog="vmn_point_texts.py")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("-decode", action="store_true", help="raw plaintexts -> lines of text")
    what.add_argument("-encode", action="store_true", help="lines of text -> raw plaintexts")
    ap.add_argument("-width", type=int, default=1)
    ap.add_argument("-keywidth", type=int, default=1)
    grp_arg = ap.add_mutually_exclusive_group(required=True)
    grp_arg.add_argument("--curve")
    grp_arg.add_argument("--params", metavar="FILE", help="a proof directory's params.json: its group")
    ap.add_argument("--wire", choices=("java", "natural"), default="java")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("input")
    ap.add_argument("output")
    args = ap.parse_args(argv)
    if args.width < 1:
        ap.error("-width must be at least 1")
    if args.keywidth < 1:
        ap.error("-keywidth must be at least 1")
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import ecscalar, interface
    name = args.curve if args.curve is not None else _curve_of_params(ap, args.params)
    try:
        ecscalar.curve(name)
    except (KeyError, ValueError) as e:
        ap.error("unknown curve %r (%s)" % (name, e))
    if not os.path.isfile(args.input):
        sys.stderr.write("%s: no such file\n" % args.input)
        return 1
    try:
        ctx = vmn.Context(args.device)
    except vmn.VmnError as e:                          # no GPU: there is no host conversion to fall back to
        sys.stderr.write("%s\n" % e)
        return 3
    grp = vmn.ECqPGroup(ctx, name, java_widths=args.wire == "java")
    ncomp = args.keywidth * args.width
    if args.decode:
        comps = interface.read_plaintexts(grp, args.input, args.width, args.keywidth)
        if comps is None:
            sys.stderr.write("%s: not a raw list of plaintexts of width %d over this group\n" % (args.input, args.width))
            return 1
        report = {}
        text = interface.decode_point_texts(comps, report)
        with open(args.output, "wb") as f:
            f.write(text)
        if not report["all_wellformed"]:
            sys.stderr.write("%s: some points hold no message (an empty piece each)\n" % args.input)
        if not report["all_utf8"]:
            sys.stderr.write("%s: some lines are not well-formed UTF-8 (written byte for byte)\n" % args.input)
        return 0
    report = {}
    comps = interface.read_point_texts(grp, args.input, ncomp, report)
    if comps is None:
        L = interface.point_encode_length(grp)
        sys.stderr.write("%s: line %d has more than %d bytes (%d components of %d)\n"
                         % (args.input, report["first_long_line"] + 1, ncomp * L, ncomp, L))
        return 1
    interface.write_plaintexts(args.output, comps, "raw", args.keywidth)
    return 0


if __name__ == "__main__":
    sys.exit(main())
