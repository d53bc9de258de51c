"""vmn_garray_expprod_arrays, measured two ways.

  python tools/expprod_arrays_ab.py
      the call against the host sequence it replaces (exp_scalar per base, mul, inv, mul) inside THIS build, alternating passes,
      medians and spread: parties {1, 2} of 3 at N = 10^6 over group 14 and P-256, three full-length bases at N = 10^5.
  python tools/expprod_arrays_ab.py --parent TREE
      vmn_combine_decryption_factors_wide through its own entry point, this tree against TREE (a built checkout of the parent
      commit), alternating: every pass is a fresh process per tree that builds the factors and times the combine REPS times.
      Group 14 with k = 3, threshold 2, width 1 and P-256 at width 3, N = 10^6.

Output: profiles/expprod_arrays_ab.txt."""
import os
import statistics
import sys
import time

import importlib.util
import subprocess

HERE = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
REPS = 7


def load(tree):
    """the package, its native drivers and pyref of the checkout at `tree`"""
    sys.path.insert(0, tree)
    import __graft_entry__ as E
    vmn = E.load_package()
    spec = importlib.util.spec_from_file_location("verificatum_vmn_amd.native", os.path.join(E.PKG_DIR, "native.py"))
    nat = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = nat
    spec.loader.exec_module(nat)
    from oracle import pyref
    return vmn, nat, pyref


def combine_child(tree):
    """one pass: the combine of parties {1, 2} of 3 at N = 10^6, REPS times after a warm-up, one line of times per case"""
    vmn, nat, pyref = load(tree)
    ctx = vmn.Context(0)
    p, q, g = pyref.modp_group(2048)
    N = 10 ** 6
    for label, G, width in (("group14 width 1", vmn.ModPGroup(ctx, p, q, g), 1), ("P-256 width 3", vmn.ECqPGroup(ctx, "P-256"), 3)):
        seed = lambda l, c: (b"combine/%d/%d" % (l, c)).ljust(32, b".")
        F = [None] + [[G.exp(G.g, G.ringArrayFromPRG(seed(l, c), N, 256)) for c in range(width)] for l in (1, 2)] + [None]
        arg = F if width > 1 else [f[0] if f else None for f in F]
        times = []
        for r in range(REPS + 1):
            t0 = time.perf_counter()
            out = nat.combineDecryptionFactors(arg, [0, 1, 1, 0], 3, 2, G.q)
            for o in (out if width > 1 else [out]):
                o.copyOfRange(0, 1).toBytes()
            if r:
                times.append((time.perf_counter() - t0) * 1e3)
        print("%s: %s" % (label, " ".join("%.3f" % t for t in times)), flush=True)
        del F, arg, out


def combine_ab(parent):
    got = {}
    for rnd in range(3):
        for name, tree in (("this commit", HERE), ("parent commit", os.path.abspath(parent))):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], cwd=tree, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit("pass failed in %s:\n%s" % (tree, r.stderr[-2000:]))
            for line in r.stdout.splitlines():
                if ": " in line:
                    label, vals = line.split(": ")
                    got.setdefault((label, name), []).extend(float(v) for v in vals.split())
    print("vmn_combine_decryption_factors_wide, parties {1, 2} of 3 at threshold 2, N = 10^6: 3 alternating passes per commit, each a fresh")
    print("process timing %d calls after a warm-up; wall time up to a device synchronisation, median (min - max) over all calls" % REPS)
    for (label, name), v in sorted(got.items()):
        print("%-18s %-14s median %7.2f ms  (%7.2f - %7.2f)  n = %d" % (label, name, statistics.median(v), min(v), max(v), len(v)))


if len(sys.argv) > 2 and sys.argv[1] == "--child":
    combine_child(sys.argv[2])
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[1] == "--parent":
    combine_ab(sys.argv[2])
    sys.exit(0)

vmn, _, pyref = load(HERE)
ctx = vmn.Context(0)


def sync(a):
    a.copyOfRange(0, 1).toBytes()


def old_sequence(bases, ints):
    pos = neg = None
    for b, c in zip(bases, ints):
        t = b.exp(abs(c))
        if c > 0:
            pos = t if pos is None else pos.mul(t)
        else:
            neg = t if neg is None else neg.mul(t)
    return pos if neg is None else (neg.inv() if pos is None else pos.mul(neg.inv()))


def measure(label, G, comps, ints):
    new_t, old_t = [], []
    for r in range(REPS + 1):
        for which in ("new", "old"):
            t0 = time.perf_counter()
            outs = [G.expProd(b, ints) if which == "new" else old_sequence(b, ints) for b in comps]
            for o in outs:
                sync(o)
            dt = (time.perf_counter() - t0) * 1e3
            if r:
                (new_t if which == "new" else old_t).append(dt)
            if r == 0 and which == "old":
                same = all(a.equals(b) for a, b in zip(outs, first))
            first = outs
    fmt = lambda v: "median %8.2f ms  min %8.2f  max %8.2f" % (statistics.median(v), min(v), max(v))
    print("%-58s one call: %s | host sequence: %s | equal: %s" % (label, fmt(new_t), fmt(old_t), same), flush=True)


p, q, g = pyref.modp_group(2048)
G = vmn.ModPGroup(ctx, p, q, g)
N = 10 ** 6
F = [G.exp(g, G.ringArrayFromPRG((b"ab/%d" % j).ljust(32, b"."), N, 256)) for j in range(2)]
measure("(a) group 14, parties {1,2} of 3, width 1, N = 10^6, (2, -1)", G, [F], [2, -1])
del F
N = 10 ** 5
F = [G.exp(g, G.ringArrayFromPRG((b"ab3/%d" % j).ljust(32, b"."), N, 256)) for j in range(3)]
full = [(v | (1 << 2046)) for v in pyref.stream_ints(b"ab/full", 3, q)]
measure("(b) group 14, three full-length exponents, N = 10^5", G, [F], full)
measure("(b') the same, signs (+, -, +)", G, [F], [full[0], -full[1], full[2]])
del F
C = vmn.ECqPGroup(ctx, "P-256")
N = 10 ** 6
FC = [[C.exp(C.g, C.ringArrayFromPRG((b"abc/%d/%d" % (j, c)).ljust(32, b"."), N, 256)) for j in range(2)] for c in range(3)]
measure("(a) P-256, parties {1,2} of 3, width 3, N = 10^6, (2, -1)", C, FC, [2, -1])
