#!/usr/bin/env python3
"""vre.py — the reference's `vre` (ProtocolElGamalRearTool): rearrange public keys, lists of ciphertexts and lists of plaintexts.

  python tools/vre.py -pkeys -noin N -format F                      GROUP KEY.. OUT..
  python tools/vre.py -sub -inter I (-ciphs | -plain) [-width W]    GROUP PKEY IN OUT..
  python tools/vre.py -cat (-ciphs | -plain) [-width W]             GROUP PKEY IN.. OUT
  python tools/vre.py -shallow -widths WS -format F (-ciphs|-plain) GROUP PKEY IN.. OUT..
  python tools/vre.py -deep -noin N [-width W] -format F (-ciphs|-plain) GROUP KEY.. IN.. OUT..
  GROUP: (--bits B | --curve NAME) [--wire java|natural] [--device D]

The usage forms and option names are those of ProtocolElGamalRearTool.java:700-724; all files are in the raw interface, as the
reference's tool reads and writes them.  -pkeys: the first N files are public keys, one output per source of the format F
("(key,row)x(key,row):..."), its g rows and then its y rows; one position gives a plain pair.  -sub: one output per interval of
I ("s-e:s-e", intervals may intersect); -cat: the inputs one after the other.  -shallow: input i has width WS[i] ("2:1:5"), an
output picks plaintext components "(input,component)"; -deep: input i lies under KEY i, an output picks keys "(input,key)" and lies
under a key of as many rows.  In forms 2-4 PKEY is read only for its keywidth (the header of its halves); in -deep the first N
files are the keys, the next N the lists.  [NOT-IN-REF] -deep -ciphs: the reference leaves it as a commented-out block that exits
0 (:993-1007); here each half of the ciphertexts goes by the plan of the plaintexts.  The group is the RFC 3526 safe-prime group
of B bits or the named curve, as in tools/vmnc_convert.py.

The reference's `main` cannot run -pkeys, -shallow or -deep as written: getFilenames (ProtocolElGamalRearParser.java:316) rejects
end == filenames.length, which every one of those forms passes for its outputs.  The help text (:726-837) and the methods of
ProtocolElGamalRear, exercised by TestProtocolElGamalRear, are the specification here.

Exit status: 0 done; 1 an input is not what it should be (missing, no tree of the stated shape, an element outside the group, an
interval beyond the list, lists of different lengths): nothing is written; 2 usage, including a malformed format, interval or
width string, with the reference's message; 3 no GPU (there is no host path to fall back to)."""
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
    ap = _Parser(prog="vre.py", allow_abbrev=False)
    for mode, text in (("-pkeys", "rearrange public keys"), ("-sub", "split a list into sublists"), ("-cat", "concatenate lists"),
                       ("-shallow", "pick plaintext components of lists of one keywidth"), ("-deep", "pick keys of lists of one width")):
        ap.add_argument(mode, action="store_true", help=text)
    ap.add_argument("-ciphs", action="store_true")
    ap.add_argument("-plain", action="store_true")
    ap.add_argument("-noin", type=int)
    ap.add_argument("-format")
    ap.add_argument("-inter")
    ap.add_argument("-widths", default="")
    ap.add_argument("-width", type=int, default=1)
    grp_arg = ap.add_mutually_exclusive_group(required=True)
    grp_arg.add_argument("--bits", type=int)
    grp_arg.add_argument("--curve")
    ap.add_argument("--wire", choices=("java", "natural"), default="java")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("files", nargs="*")
    args = ap.parse_args(argv)
    modes = [m for m in ("pkeys", "sub", "cat", "shallow", "deep") if getattr(args, m)]
    if len(modes) != 1:
        ap.error("exactly one of -pkeys, -sub, -cat, -shallow, -deep")
    mode = modes[0]
    import __graft_entry__ as entry
    vmn = entry.load_package()
    from verificatum_vmn_amd import rearrange as rear, stdgroups
    files = args.files
    try:
        if mode in ("pkeys", "deep"):
            if args.noin is None:
                ap.error("-%s needs -noin" % mode)
            if args.noin <= 0:
                raise rear.RearrangeFormatError("Non-positive number of public keys! (%d)" % args.noin)
        if mode in ("pkeys", "shallow", "deep"):
            if args.format is None:
                ap.error("-%s needs -format" % mode)
            fmt = rear.parse_format(args.format)
        if mode != "pkeys":
            if not (args.ciphs or args.plain):
                raise rear.RearrangeFormatError("One of the options \"-plain\" or \"-ciphs\" is required!")
            if args.ciphs and args.plain:
                raise rear.RearrangeFormatError("The options \"-plain\" and \"-ciphs\" can not be combined!")
            if args.width <= 0:
                raise rear.RearrangeFormatError("Non-positive width! (%d)" % args.width)
        if mode == "pkeys":
            if len(files) < args.noin + 1:
                raise rear.RearrangeFormatError("There are too few files! (%d < %d)" % (len(files), args.noin + 1))
            pkeys, inputs, outputs = [], files[:args.noin], files[args.noin:]
            if len(fmt) != len(outputs):
                raise rear.RearrangeFormatError("The format and number of output filenames do not match!")
        elif mode == "deep":
            n = args.noin
            if 2 * n + len(fmt) != len(files):
                raise rear.RearrangeFormatError("The number of public keys (%d) plus the number of input group element arrays (%d) plus the "
                                                "number of output group element arrays (%d) specified in the output format does not equal "
                                                "the number of filenames (%d)!" % (n, n, len(fmt), len(files)))
            pkeys, inputs, outputs = files[:n], files[n:2 * n], files[2 * n:]
        else:
            if not files:
                ap.error("the raw public key comes first")
            pkeys, files = files[:1], files[1:]
            if mode == "sub":
                if args.inter is None:
                    ap.error("-sub needs -inter")
                try:
                    intervals = rear.parse_intervals(args.inter)
                except rear.RearrangeFormatError as e:
                    raise rear.RearrangeFormatError("Failed to parse intervals! (%s) %s" % (args.inter, e)) from None
                if len(files) < 2:
                    raise rear.RearrangeFormatError("Too few files! (%d < 2)" % len(files))
                if len(intervals) != len(files) - 1:
                    raise rear.RearrangeFormatError("Mismatching number of intervals and output filenames! (%d != %d)" % (len(intervals), len(files) - 1))
                inputs, outputs = files[:1], files[1:]
            elif mode == "cat":
                if len(files) < 2:
                    raise rear.RearrangeFormatError("Too few files! (%d)" % len(files))
                inputs, outputs = files[:-1], files[-1:]
            else:
                widths = rear.parse_widths(args.widths) if args.widths != "" else [1]
                if len(widths) + len(fmt) != len(files):
                    raise rear.RearrangeFormatError("The number of widths (%d) plus the number of output files (%d) specified in the output format "
                                                    "does not equal the number of filenames (%d)!" % (len(widths), len(fmt), len(files)))
                inputs, outputs = files[:len(widths)], files[len(widths):]
    except rear.RearrangeFormatError as e:
        sys.stderr.write("vre.py: %s\n" % e)
        return 2
    if args.bits is not None:
        try:
            p, q, g = stdgroups.modp_group(args.bits)
        except ValueError as e:
            ap.error(str(e))
    for path in pkeys + inputs:
        if not os.path.isfile(path):
            sys.stderr.write("%s: no such file\n" % path)
            return 1
    try:
        ctx = vmn.Context(args.device)
    except vmn.VmnError as e:                          # no GPU: there is no host path to fall back to
        sys.stderr.write("%s\n" % e)
        return 3
    if args.bits is not None:
        grp = vmn.ModPGroup(ctx, p, q, g, nbytes=None if args.wire == "java" else (args.bits + 7) // 8)
    else:
        try:
            grp = vmn.ECqPGroup(ctx, args.curve, java_widths=args.wire == "java")
        except (KeyError, ValueError, vmn.VmnError) as e:
            ap.error("unknown curve %r (%s)" % (args.curve, e))
    try:
        keywidths = []
        for path in pkeys:
            with open(path, "rb") as f:
                keywidths.append(rear.pkey_keywidth(grp, f.read(16)))
            if keywidths[-1] is None:
                raise rear.RearrangeInputError(path, "not a raw public key over this group")
        if mode == "pkeys":
            rear.pkeys_files(grp, inputs, outputs, fmt)
        elif mode == "sub":
            rear.sub_files(grp, inputs[0], outputs, intervals, args.width, keywidths[0], args.ciphs)
        elif mode == "cat":
            rear.cat_files(grp, inputs, outputs[0], args.width, keywidths[0], args.ciphs)
        elif mode == "shallow":
            rear.shallow_files(grp, inputs, outputs, widths, keywidths[0], fmt, args.ciphs)
        else:
            rear.deep_files(grp, inputs, outputs, keywidths, args.width, fmt, args.ciphs)
    except (rear.RearrangeInputError, rear.RearrangeFormatError) as e:
        sys.stderr.write("vre.py: %s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
