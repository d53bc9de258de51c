#!/usr/bin/env python3
"""vmnc_convert.py — the reference's `vmnc -ciphs -ini FMT -outi FMT in out`: a ciphertext list from one interface to another,
and `vmnc -plain -outi FMT in out`: the plaintexts the mix-net left behind in the form of an interface.

  python tools/vmnc_convert.py -ciphs -ini native -outi raw [-width W] [-keywidth K] (--bits B | --curve NAME) [--wire java|natural] IN OUT
  python tools/vmnc_convert.py -plain -outi json [-width W] --bits B [--wire java|natural] IN OUT

FMT: native (one ciphertext per line, the line the hexadecimal byte tree of that ciphertext; the reference's default), raw
(one byte tree of the 2 W component arrays; what the mix-net and a proof directory hold) or json (one ciphertext per line,
{"alpha":"A","beta":"B"} with decimal strings, an array of W such pairs above width 1; modular groups only, so --curve with
json is a usage error).  -plain reads the raw array tree of the W plaintext components and writes json ("M" per line, or
["M1",...,"MW"]) or raw again; it takes no -ini.  The group is the RFC 3526 safe-prime
group of B bits or the named curve, at the reference's leaf widths (--wire java, the default) or at the bytes of the modulus.
The list is parsed, range- and membership-checked and written on the GPU (verificatum_vmn_amd.interface).
-keywidth K: the list lies under a public key of width K (the protocol info's keywidth): 2 K W component arrays, every half of a
line or of the raw tree nested once more; native and raw only -- the reference's json classes cannot hold such a list, so
-keywidth above 1 with json is a usage error.  -plain -outi raw takes it as well.

Exit status: 0 the list was converted; 1 IN is no list of the input interface (a malformed native or json line is named,
counted from 1, on stderr), no output is written; 2 usage; 3 no GPU (there is no host conversion to fall back to)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Parser(argparse.ArgumentParser):
    def error(self, message):
        self.print_usage(sys.stderr)
        sys.stderr.write("%s: %s\n" % (self.prog, message))
        sys.exit(2)


def main(argv=None):
    ap = _Parser(prog="vmnc_convert.py")
    what = ap.add_mutually_exclusive_group(required=True)
    what.add_argument("-ciphs", action="store_true", help="convert a list of ciphertexts")
    what.add_argument("-plain", action="store_true", help="write the raw plaintexts in the form of an interface (json or raw)")
    ap.add_argument("-ini", choices=("native", "raw", "json"))
    ap.add_argument("-outi", choices=("native", "raw", "json"), required=True)
    ap.add_argument("-width", type=int, default=1)
    ap.add_argument("-keywidth", type=int, default=1)
    grp_arg = ap.add_mutually_exclusive_group(required=True)
    grp_arg.add_argument("--bits", type=int)
    grp_arg.add_argument("--curve")
    ap.add_argument("--wire", choices=("java", "natural"), default="java")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("input")
    ap.add_argument("output")
    args = ap.parse_args(argv)
    if args.width < 1:
        ap.error("-width must be at least 1")
    if args.keywidth < 1:
        ap.error("-keywidth must be at least 1")
    if args.keywidth > 1 and "json" in (args.ini, args.outi):
        ap.error("the json interface cannot hold a list under a key of width above 1")
    if args.ciphs and args.ini is None:
        ap.error("-ciphs needs -ini")
    if args.plain and args.ini is not None:
        ap.error("-plain reads the raw plaintexts: it takes no -ini")
    if args.plain and args.outi == "native":
        ap.error("-plain writes json or raw")
    if args.curve is not None and "json" in (args.ini, args.outi):
        ap.error("the json interface covers modular groups only")
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import interface, stdgroups
    if args.bits is not None:
        try:
            p, q, g = stdgroups.modp_group(args.bits)
        except ValueError as e:
            ap.error(str(e))
    if not os.path.isfile(args.input):
        sys.stderr.write("%s: no such file\n" % args.input)
        return 1
    try:
        ctx = vmn.Context(args.device)
    except vmn.VmnError as e:                          # no GPU: there is no host conversion to fall back to
        sys.stderr.write("%s\n" % e)
        return 3
    if args.bits is not None:
        grp = vmn.ModPGroup(ctx, p, q, g, nbytes=None if args.wire == "java" else (args.bits + 7) // 8)
    else:
        try:
            grp = vmn.ECqPGroup(ctx, args.curve, java_widths=args.wire == "java")
        except (KeyError, ValueError, vmn.VmnError) as e:
            ap.error("unknown curve %r (%s)" % (args.curve, e))
    if args.plain:
        comps = interface.read_plaintexts(grp, args.input, args.width, args.keywidth)
        if comps is None:
            sys.stderr.write("%s: not a raw list of plaintexts of width %d over this group\n" % (args.input, args.width))
            return 1
        interface.write_plaintexts(args.output, comps, args.outi, args.keywidth)
        return 0
    report = {}
    ok = interface.convert_list(grp, args.input, args.output, args.width, args.ini, args.outi, report=report, keywidth=args.keywidth)
    if ok:
        return 0
    if args.ini == "json" and report and not report["format_ok"]:
        sys.stderr.write("%s: line %d is not a json ciphertext of width %d ({\"alpha\":\"..\",\"beta\":\"..\"} with decimal strings)\n"
                         % (args.input, report["first_bad_line"] + 1, args.width))
    elif args.ini == "native" and report and not report["format_ok"]:
        sys.stderr.write("%s: line %d is not a ciphertext of width %d over this group (%d hex digits of its byte tree)\n"
                         % (args.input, report["first_bad_line"] + 1, args.width, 2 * interface.ciphertext_line_bytes(grp, args.width, args.keywidth)))
    else:
        sys.stderr.write("%s: not a list of ciphertexts of width %d over this group in the %s interface "
                         "(format, a value out of range, or an element outside the group)\n" % (args.input, args.width, args.ini))
    return 1


if __name__ == "__main__":
    sys.exit(main())
