"""The cells of the modular power kernels: every operation in every execution geometry, as a plain launch and as a phased one.
tests/test_power_geometry_catalogue.py checks the list itself on the CPU, tests/test_gpu_power_geometries.py runs it on the GPU.

A geometry (GEOMETRIES): name, bits, kind, the (small, tiny) thresholds that force it, S columns, `rows`, LPE lanes per element,
EPB = 256 / LPE elements per workgroup.  An operation (OPERATIONS): the entry point, the Python wrapper, the kernels it reaches,
the timing families it reports in, how its inputs are shaped.  A cell (cells()): one operation variant in one geometry at one
size, plain or phased, with the environment it runs under and its calls.  The host's rules that decide which kernel a call
reaches -- geom() and PhasePlan of csrc/vmnhip.hip, the window choices, the sliding-window schedule -- are restated here as
functions of a Rules object, so that the CPU suite can check the claims of every cell and run mutants of the rules."""
from functools import lru_cache

from oracle import pyref

BLOCK = 256                       # threads per workgroup
DEVICE_BLOCKS = 2 * 256           # workgroup slots of an MI355X: 256 compute units x blocks_per_cu() = 2
DEFAULT_THRESHOLDS = (40960, 6144)
SHARED_ARRAYS = 8                 # arrays per fused launch (csrc/modp_shared_exp.h)
FORCE = {"base": (0, 0), "wide": (2 ** 63, 0), "wide8": (2 ** 63, 2 ** 63)}
ORDER = ("base", "wide", "wide8")                 # executed multiply-adds of one call strictly increase in this order


def _geometry(bits, kind, S, rows, lpe):
    return dict(name="%d-%s" % (bits, kind), bits=bits, kind=kind, force=FORCE[kind], S=S, rows=rows, LPE=lpe, EPB=BLOCK // lpe)


GEOMETRIES = [_geometry(2048, "base", 74, 74, 1), _geometry(2048, "wide", 76, 74, 4), _geometry(2048, "wide8", 80, 74, 8),
              _geometry(3072, "base", 110, 110, 2), _geometry(3072, "wide", 112, 110, 4),
              _geometry(4096, "base", 148, 148, 4)]       # 4096 bits: the single geometry, so that its multi-array and phased cells run
BITS = (2048, 3072, 4096)


def geometries(bits):
    return [g for g in GEOMETRIES if g["bits"] == bits]


def geometry(bits, kind):
    return next(g for g in GEOMETRIES if g["bits"] == bits and g["kind"] == kind)


class Rules:
    """The host's rules, as csrc/vmnhip.hip states them."""

    def geometry_for(self, bits, items, small, tiny, always=False):
        """geom(): the kind of geometry a launch over `items` elements runs in (wide8 exists at 2048 bits, wide at 2048 and 3072)"""
        if bits == 2048 and tiny != 0 and (items <= tiny or (always and items <= small)):
            return "wide8"
        if bits not in (2048, 3072) or small == 0:
            return "base"
        return "wide" if always or items <= small else "base"

    def tiles(self, n, epb, arrays=1):
        """PhasePlan: the arrays' tiles side by side, each array with its own ragged last tile"""
        return arrays * ((n + epb - 1) // epb)

    def is_phased(self, n, epb, arrays, max_blocks, cuttable_steps):
        """PhasePlan::split: more tiles than workgroup slots, and at least two steps to cut between"""
        return self.tiles(n, epb, arrays) > min(DEVICE_BLOCKS, max_blocks or DEVICE_BLOCKS) and cuttable_steps >= 2

    def launches(self, k):
        """the fused multi-array calls: one launch per SHARED_ARRAYS arrays"""
        return (k + SHARED_ARRAYS - 1) // SHARED_ARRAYS


RULES = Rules()
geometry_for, tiles, is_phased, launches = RULES.geometry_for, RULES.tiles, RULES.is_phased, RULES.launches


def pick_window(ebits):
    """the fixed window of k_modpow / k_modpow2 / k_modpow_jobs"""
    return min(range(1, 8), key=lambda w: ((1 << w) - 2 + (ebits + w - 1) // w, w))


def sliding_window_bits(ebits):
    return min(range(2, 9), key=lambda w: ((1 << (w - 1)) + ebits // (w + 1), w))


def slide_steps(e, w):
    """slide_schedule(): the number of steps of e's schedule under odd windows of at most w bits"""
    steps, pending, i = 0, 0, e.bit_length() - 1
    while i >= 0:
        if not (e >> i) & 1:
            pending, i = pending + 1, i - 1
            continue
        lo = max(i - w + 1, 0)
        while not (e >> lo) & 1:
            lo += 1
        steps, pending, i = steps + 1, 0, lo - 1
    return steps + (1 if pending else 0)


def fixed_parts(n, nwin, fill=786432):
    """vmn_group_exp_fixed: the pieces an element's chain of nwin - 1 products is cut into (fill = VMN_FIXED_SPLIT_FILL; 0 = uncut)"""
    parts = 1
    while parts < 16 and 2 * parts * n <= fill and nwin // (2 * parts) >= 4:
        parts *= 2
    return parts


def product_mads(geom):
    """note_work(): the multiply-adds of one Montgomery product in a geometry"""
    return 2 * geom["rows"] * geom["S"]


# ---- operations -------------------------------------------------------------------------------------------------------------
OPERATIONS = {
    "exp_array": dict(entry="vmn_garray_exp_array", wrapper="X.exp(E)", kernels=("k_modpow", "k_modpow_phased"), families=("modpow",),
                      inputs="one array, per-element exponents below q: 0, 1, q - 1 and 1 << (bits(q) - 1) among them", phased=True),
    "exp_scalar_sliding": dict(entry="vmn_garray_exp_scalar", wrapper="X.exp(e)", kernels=("k_modpow_shared", "k_modpow_shared_phased"),
                               families=("modpow",), inputs="one array, one exponent above 32 bits per call", phased=True),
    "exp_scalar_fixed": dict(entry="vmn_garray_exp_scalar", wrapper="X.exp(e)", kernels=("k_modpow", "k_modpow_phased"), families=("modpow",),
                             inputs="one array; 0xC0FFEE11, and a full-length exponent under VMN_SLIDING_WINDOW=0: exponent stride 0",
                             phased=True),
    "exp_scalar_multi": dict(entry="vmn_garray_exp_scalar_multi", wrapper="expMulti(arrays, e)",
                             kernels=("k_modpow_shared_multi", "k_modpow_shared_multi_phased", "k_modpow_shared"), families=("modpow",),
                             inputs="k = 3 and k = 9 distinct arrays (a launch of eight and one of one), one exponent above 32 bits", phased=True),
    "exp_scalars_multi": dict(entry="vmn_garray_exp_scalars_multi", wrapper="expMultiEach(arrays, exps)",
                              kernels=("k_modpow_shared_each", "k_modpow_shared_each_phased"), families=("modpow",),
                              inputs="k = 3 arrays under a full-length exponent, one of about 200 bits and (1 << 33) + 1", phased=True),
    "exp2": dict(entry="vmn_garray_exp2", wrapper="X.exp2(e, Y, F, fbits)", kernels=("k_modpow2", "k_modpow2_phased"), families=("modpow",),
                 inputs="a shared 256-bit e with 613-bit f[i]; e = 0; e longer than every f", phased=True),
    "exp_pair": dict(entry="vmn_garray_exp_pair", wrapper="X.expPair(e, Y, F, fbits)", kernels=("k_modpow_jobs",), families=("modpow",),
                     inputs="(nx, ny) equal and unequal, either job the longer one; VMN_PAIR_MIXED=0, so that a wide launch is k_modpow_jobs itself",
                     phased=False),
    "exp_fixed": dict(entry="vmn_group_exp_fixed", wrapper="G.exp(base, E)", kernels=("k_fixed_level", "k_fixed_exp"),
                      families=("fixed_table", "fixed"), inputs="200 exponents below q; VMN_FIXED_WINDOW 2, 5, 11; the chain uncut and cut",
                      phased=False),
}
MISSING_CELLS = {("exp_pair", "phased"): "vmn_garray_exp_pair has no phased kernel: arrays of more tiles than fit take two ordinary launches",
                 ("exp_fixed", "phased"): "k_fixed_exp runs one workgroup per tile: there is no phase plan"}
MULTI_K = 9                       # arrays of the pool: SHARED_ARRAYS + 1
FIXED_N = 200
FIXED_WINDOWS = (2, 5, 11)
SHORT_E = 0xC0FFEE11


def plain_sizes(epb):
    """one ragged tile; a second tile of one element"""
    return (epb - 1, epb + 1)


def phased_size(epb):
    """three tiles on two workgroup slots, the third ragged"""
    return 2 * epb + epb // 2 + 1


def nmax(bits):
    """the longest array of a modulus size: the phased single-array size of its base geometry"""
    return phased_size(geometry(bits, "base")["EPB"])


def multi_nmax(bits):
    return geometry(bits, "base")["EPB"] + 1


# ---- inputs -------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def inputs(bits):
    """Everything the cells of one modulus size work on.  Arrays: MULTI_K pool arrays of squares mod p, array 0 of nmax elements with
    1 and p - 1 in front (p - 1 is no subgroup element, but no power asks), the others of EPB + 1; exponents by name."""
    p, q, g = pyref.modp_group(bits)
    tag = b"powgeom/%d/" % bits
    n0, n1 = nmax(bits), multi_nmax(bits)
    xs = [[pow(1 + v % (p - 1), 2, p) for v in pyref.stream_ints(tag + b"x%d" % c, n0 if c == 0 else n1, p)] for c in range(MULTI_K)]
    xs[0][0], xs[0][1], xs[1][0] = 1, p - 1, p - 1
    ys = [pow(x, 3, p) for x in xs[0][::-1]]
    qb = q.bit_length()
    full = pyref.stream_ints(tag + b"e", 1, q)[0] | (3 << (qb - 2))          # full length, its top bits set; below q, whose top 63 bits are ones
    assert full < q and full.bit_length() == qb
    shared = {"full": full, "q-1": q - 1, "(1<<33)+1": (1 << 33) + 1, "1<<200": 1 << 200, "short": SHORT_E,
              "e200": pyref.stream_ints(tag + b"e200", 1, 1 << 199)[0] | (1 << 199),
              "e256": pyref.stream_ints(tag + b"e256", 1, 1 << 255)[0] | (1 << 255), "zero": 0, "e700": (1 << 700) + 12345}
    es = pyref.stream_ints(tag + b"es", n0, q)
    es[0], es[1], es[2], es[3] = 0, 1, q - 1, 1 << (qb - 1)
    fs = pyref.stream_ints(tag + b"fs", n0, 1 << 613)
    fs[0], fs[1], fs[2] = 0, 1 << 612, (1 << 613) - 1
    fixed_es = pyref.stream_ints(tag + b"fixed", FIXED_N, q)
    fixed_es[0], fixed_es[1], fixed_es[2], fixed_es[3] = 0, 1, q - 1, 1 << (qb - 1)
    return dict(p=p, q=q, g=g, xs=xs, ys=ys, shared=shared, es=es, fs=fs, fixed_es=fixed_es, fixed_base=pow(g, 12345, p))


EXP2_FORMS = (("e256", 613), ("zero", 613), ("e700", 41))       # (shared exponent, bits of the per-element ones)


@lru_cache(maxsize=None)
def expected(bits, orc):
    """The expected values of one modulus size, from the GMP oracle `orc`, once, on the longest arrays: every cell compares with a
    prefix (a power of a prefix of an array is the prefix of the array's powers; results never depend on the geometry)."""
    I = inputs(bits)
    xs, ys, sh = I["xs"], I["ys"], I["shared"]
    want = dict(exp_array=orc.exp_array(xs[0], I["es"]))
    want["scalar"] = {(0, name): orc.exp_scalar(xs[0], sh[name]) for name in ("full", "q-1", "(1<<33)+1", "1<<200", "short", "e200", "e256", "zero", "e700")}
    for c in range(1, MULTI_K):
        want["scalar"][(c, "full")] = orc.exp_scalar(xs[c], sh["full"])
    for c in (1, 2):
        for name in ("(1<<33)+1", "e200"):
            want["scalar"][(c, name)] = orc.exp_scalar(xs[c], sh[name])
    want["yf"] = {fbits: orc.exp_array(ys, [f % (1 << fbits) for f in I["fs"]]) for fbits in sorted({fb for _, fb in EXP2_FORMS})}
    want["exp2"] = {(name, fbits): orc.mul(want["scalar"][(0, name)], want["yf"][fbits]) for name, fbits in EXP2_FORMS}
    want["fixed"] = orc.exp_fixed(I["fixed_base"], I["fixed_es"])
    return want


# ---- cells --------------------------------------------------------------------------------------------------------------------
def _cuttable(op, bits, call):
    """the steps a launch of the call can be cut between: what PhasePlan::split is given"""
    I = inputs(bits)
    qb, sh = I["q"].bit_length(), I["shared"]
    if op == "exp_array":
        return (qb + pick_window(qb) - 1) // pick_window(qb) - 1
    if op == "exp_scalar_fixed":
        eb = max(1, sh[call["e"]].bit_length())
        return (eb + pick_window(eb) - 1) // pick_window(eb) - 1
    if op in ("exp_scalar_sliding", "exp_scalar_multi"):
        e = sh[call["e"]]
        return slide_steps(e, sliding_window_bits(e.bit_length())) - 1
    if op == "exp_scalars_multi":
        es = [sh[name] for name in call["es"]]
        w = sliding_window_bits(max(e.bit_length() for e in es))
        return max(slide_steps(e, w) for e in es) - 1
    if op == "exp2":
        eb, fb = max(1, sh[call["e"]].bit_length()), call["fbits"]
        w = min(pick_window(max(eb, fb)), 5)
        return max((eb + w - 1) // w, (fb + w - 1) // w)
    raise KeyError(op)


def _cell(op, variant, geom, form, n, calls, env=None, max_blocks=None, arrays=1):
    env = dict(env or {})
    if max_blocks:
        env["VMN_MODPOW_MAX_BLOCKS"] = str(max_blocks)
    cid = "%s-%d-%s-%s-n%d" % (variant, geom["bits"], geom["kind"], form, n) + ("-mb%d" % max_blocks if max_blocks else "")
    return dict(id=cid, op=op, variant=variant, bits=geom["bits"], kind=geom["kind"], geometry=geom["name"], form=form, n=n, arrays=arrays,
                max_blocks=max_blocks, env=env, calls=calls,
                row="%s-%d-%s-n%d" % (variant, geom["bits"], form, n) + ("-mb%d" % max_blocks if max_blocks else ""))


@lru_cache(maxsize=None)
def cells():
    """Every cell.  A call: dict(kind=..., per-kind fields, env = knobs of this call alone, launches = {family: count})."""
    out = []
    for geom in GEOMETRIES:
        epb = geom["EPB"]
        single = [("plain", n, None) for n in plain_sizes(epb)] + [("phased", phased_size(epb), 2)]
        for form, n, mb in single:
            one = {"modpow": 1}
            out.append(_cell("exp_array", "exp_array", geom, form, n, [dict(kind="exp_array", launches=one)], max_blocks=mb))
            # ((1 << 33) + 1 and 1 << 200 are schedules of two steps: one step to cut, so no phases -- the plain cells have them)
            names = ("full", "q-1", "(1<<33)+1", "1<<200") if form == "plain" else ("full", "q-1", "e200")
            out.append(_cell("exp_scalar_sliding", "exp_scalar_sliding", geom, form, n,
                             [dict(kind="exp_scalar", e=name, launches=one) for name in names], max_blocks=mb))
            out.append(_cell("exp_scalar_fixed", "exp_scalar_fixed", geom, form, n,
                             [dict(kind="exp_scalar", e="short", launches=one),
                              dict(kind="exp_scalar", e="full", env={"VMN_SLIDING_WINDOW": "0"}, launches=one)], max_blocks=mb))
            out.append(_cell("exp2", "exp2", geom, form, n, [dict(kind="exp2", e=name, fbits=fbits, launches=one) for name, fbits in EXP2_FORMS],
                             max_blocks=mb))
        multi = [("plain", n, None) for n in plain_sizes(epb)] + [("phased", n, mb) for n in plain_sizes(epb) for mb in (2, 1)]
        for form, n, mb in multi:
            out.append(_cell("exp_scalar_multi", "exp_scalar_multi_k3", geom, form, n,
                             [dict(kind="exp_multi", k=3, e=name, launches={"modpow": RULES.launches(3)}) for name in ("full", "(1<<33)+1" if form == "plain" else "e200")],
                             max_blocks=mb, arrays=3))
            out.append(_cell("exp_scalars_multi", "exp_scalars_multi_k3", geom, form, n,
                             [dict(kind="exp_multi_each", k=3, es=("full", "e200", "(1<<33)+1"), launches={"modpow": RULES.launches(3)})],
                             max_blocks=mb, arrays=3))
        out.append(_cell("exp_scalar_multi", "exp_scalar_multi_k9", geom, "plain", epb + 1,
                         [dict(kind="exp_multi", k=MULTI_K, e="full", launches={"modpow": RULES.launches(MULTI_K)})], arrays=MULTI_K))
        pair_sizes = ((epb - 1, epb - 1), (epb + 1, epb - 1), (epb - 1, epb + 1))
        out.append(_cell("exp_pair", "exp_pair", geom, "plain", epb + 1,
                         [dict(kind="exp_pair", nx=nx, ny=ny, e="e256", fbits=613, launches={"modpow": 1}) for nx, ny in pair_sizes],
                         env={"VMN_PAIR_MIXED": "0"}))       # (it matters where a launch runs wide: k_modpow_jobs<Cfg<76, 4>> itself)
        for w in FIXED_WINDOWS:
            for cut, env in (("uncut", {"VMN_FIXED_SPLIT_FILL": "0"}), ("cut", {})):
                out.append(_cell("exp_fixed", "exp_fixed_w%d_%s" % (w, cut), geom, "plain", FIXED_N,
                                 [dict(kind="exp_fixed", w=w, cut=cut == "cut", launches={"fixed_table": w, "fixed": 1})],
                                 env=dict(env, VMN_FIXED_WINDOW=str(w))))
    assert len({c["id"] for c in out}) == len(out)
    return out


def cuttable_steps(cell):
    """per call of a cell that has a phase plan"""
    return [_cuttable(cell["op"], cell["bits"], call) for call in cell["calls"]]


def call_items(cell, call):
    """the number of elements geom() is asked about for a call under the default thresholds (exp_fixed: see fixed_items)"""
    if call["kind"] == "exp_pair":
        return (call["nx"] + call["ny"] + 1) // 2
    if call["kind"] in ("exp_multi", "exp_multi_each"):
        return min(call["k"], SHARED_ARRAYS) * cell["n"]                # (a ninth array's launch of its own asks about n: smaller still)
    return cell["n"]


def fixed_nwin(bits, w):
    qb = inputs(bits)["q"].bit_length()
    return (qb + w - 1) // w


def fixed_items(cell, call):
    """the elements of k_fixed_exp's launch: n x pieces"""
    return cell["n"] * (fixed_parts(cell["n"], fixed_nwin(cell["bits"], call["w"])) if call["cut"] else 1)


def fixed_level_lanes(bits, w):
    """the lanes of the w - 1 levels of a table's build (level l: (2^l - 1) products per window); geom() is asked per level"""
    return [((1 << l) - 1) * fixed_nwin(bits, w) for l in range(1, w)]
