"""GPU suite: every modular power kernel in every execution geometry, as a plain launch and as a phased one -- the cells of
tests/power_geometry_cases.py.  By default the geometry depends on the number of elements, and the exact oracle can only afford
a few hundred: without forcing, a 2048-bit power only ever runs eight lanes per element (Cfg<80, 8>) and a 3072-bit one four
(Cfg<112, 4>), while the benchmark's sizes run one resp. two lanes per element.  Every cell forces its geometry through the two
thresholds, sets its knobs, calls the Python wrapper and compares with the GMP oracle by exact equality.

WITNESS.  A threshold the library ignored would let a cell pass without running what it names, so every cell runs inside
timing_enable / timing_report and asserts
  - the launches of the operation's family, from the catalogue's rule (one per call; ceil(k / 8) for the fused multi-array
    calls; w launches of fixed_table and one of fixed for a fixed base);
  - that the SAME calls on the same inputs, forced into each geometry of the modulus size in turn, report strictly more
    executed multiply-adds from base to wide to wide8.  This order is derived from the code, not measured: note_work() prices a
    product at 2 rows S and a squaring at rows S + rows (S + SQR_BLK LPE) / 2 with (rows, S, LPE) = (74, 74, 1), (74, 76, 4),
    (74, 80, 8) resp. (110, 110, 2), (110, 112, 4), so it holds for any counts of products and squarings; only k_modpow in
    Cfg<74, 1> reports the count of its 71 limbs of 29 bits, which lies below the wide one;
  - that the same calls under the DEFAULT thresholds report exactly the figure of the geometry geometry_for() names for the
    size: wide8 at 2048 bits, wide at 3072 bits.  So the forced runs were different geometries, and the unforced suite never
    reaches base.  (A table's levels ask geom() about their own lane counts, the upper ones of w = 11 above the threshold: the
    default figure of fixed_table is the sum the rule gives level by level, to the seven digits the report prints.)
At 4096 bits there is one geometry: the witness is the launch count alone.  The phased form leaves no mark in the report; its
witness is the catalogue's is_phased under the cell's VMN_MODPOW_MAX_BLOCKS (tests/test_power_geometry_catalogue.py).

The expected values are computed once per modulus size on the longest arrays and sliced to prefixes.

Wall time on one MI355X, taken once: this module alone 43 s (192 tests, none above 1.5 s, the oracle's values included).
pytest -m gpu over the whole suite, one run on one machine: 654 s with this module (2563 tests), of which this module's tests
took 42 s -- 612 s for the 2371 tests of the parent commit."""
import os

import pytest

import power_geometry_cases as X

pytestmark = pytest.mark.gpu

DEFAULT = int(os.environ.get("VMN_WIDE_MAX", X.DEFAULT_THRESHOLDS[0]))
DEFAULT8 = int(os.environ.get("VMN_WIDE8_MAX", X.DEFAULT_THRESHOLDS[1]))
REPORT_DIGITS = 1e-6                      # the report prints multiply-adds as %.6e
RESULTS = {}                              # (row, where) -> what run() found: the same calls at the same size run once per geometry


@pytest.fixture(scope="module")
def world(vmn, gpu_ctx, oracle_for):
    """per modulus size: the group, the inputs and the oracle's values (computed once, on first use)"""
    made = {}

    def get(bits):
        if bits not in made:
            I = X.inputs(bits)
            made[bits] = dict(I=I, G=vmn.ModPGroup(gpu_ctx, I["p"], I["q"], I["g"]), want=X.expected(bits, oracle_for(I["p"], I["q"])))
        return made[bits]
    return get


@pytest.fixture
def thresholds(gpu_ctx):
    """set(small, tiny); the defaults are back when the test ends, however it ends"""
    def set_(small, tiny):
        gpu_ctx.set_small_array_threshold(small)
        gpu_ctx.set_tiny_array_threshold(tiny)
    try:
        yield set_
    finally:
        set_(DEFAULT, DEFAULT8)


def do_call(vmn, W, n, call):
    """(the call's results as lists of integers, the expected lists)"""
    I, G, want = W["I"], W["G"], W["want"]
    sh, kind = I["shared"], call["kind"]
    up = lambda c, m=n: G.toElementArray(I["xs"][c][:m], checked=False)
    if kind == "exp_array":
        return [up(0).exp(G.ringArray(I["es"][:n])).toInts()], [want["exp_array"][:n]]
    if kind == "exp_scalar":
        return [up(0).exp(sh[call["e"]]).toInts()], [want["scalar"][(0, call["e"])][:n]]
    if kind == "exp_multi":
        got = vmn.PGroupElementArray.expMulti([up(c) for c in range(call["k"])], sh[call["e"]])
        return [r.toInts() for r in got], [want["scalar"][(c, call["e"])][:n] for c in range(call["k"])]
    if kind == "exp_multi_each":
        got = vmn.PGroupElementArray.expMultiEach([up(c) for c in range(call["k"])], [sh[name] for name in call["es"]])
        return [r.toInts() for r in got], [want["scalar"][(c, name)][:n] for c, name in enumerate(call["es"])]
    fbits = call.get("fbits")
    if kind == "exp2":
        F = G.ringArray([f % (1 << fbits) for f in I["fs"][:n]])
        Y = G.toElementArray(I["ys"][:n], checked=False)
        return [up(0).exp2(sh[call["e"]], Y, F, fbits).toInts()], [want["exp2"][(call["e"], fbits)][:n]]
    if kind == "exp_pair":
        nx, ny = call["nx"], call["ny"]
        F = G.ringArray([f % (1 << fbits) for f in I["fs"][:ny]])
        gx, gy = up(0, nx).expPair(sh[call["e"]], G.toElementArray(I["ys"][:ny], checked=False), F, fbits)
        return [gx.toInts(), gy.toInts()], [want["scalar"][(0, call["e"])][:nx], want["yf"][fbits][:ny]]
    assert kind == "exp_fixed"
    G.releaseFixed(I["fixed_base"])                       # (a cached table would serve: every cell builds its own)
    try:
        return [G.exp(I["fixed_base"], G.ringArray(I["fixed_es"])).toInts()], [want["fixed"]]
    finally:
        G.releaseFixed(I["fixed_base"])


def run(cell, where, vmn, gpu_ctx, world, thresholds, monkeypatch):
    """The cell's calls with every launch forced into geometry `where` (or "default": the thresholds as they stand in
    production).  {"wrong": the calls whose values differ from the oracle's, "launches", "mads": per family of the operation}."""
    key = (cell["row"], where)
    if key in RESULTS:
        return RESULTS[key]
    W = world(cell["bits"])
    thresholds(*((DEFAULT, DEFAULT8) if where == "default" else X.FORCE[where]))
    wrong = []
    with monkeypatch.context() as mp:
        for name, value in cell["env"].items():
            mp.setenv(name, value)
        gpu_ctx.timing_enable(True)
        try:
            gpu_ctx.timing_reset()
            for call in cell["calls"]:
                with monkeypatch.context() as mc:
                    for name, value in call.get("env", {}).items():
                        mc.setenv(name, value)
                    got, want = do_call(vmn, W, cell["n"], call)
                if got != want:
                    wrong.append({k: v for k, v in call.items() if k != "launches"})
            report = gpu_ctx.timing_report()
        finally:
            gpu_ctx.timing_enable(False)
            gpu_ctx.timing_reset()
    thresholds(DEFAULT, DEFAULT8)
    families = X.OPERATIONS[cell["op"]]["families"]
    RESULTS[key] = dict(wrong=wrong, launches={f: report.get(f, (0, 0.0, 0.0, 0.0))[0] for f in families},
                        mads={f: report.get(f, (0, 0.0, 0.0, 0.0))[2] for f in families})
    return RESULTS[key]


def default_fixed_table_mads(cell):
    """the levels of the cell's table under the default thresholds, each in the geometry geom() gives its lanes"""
    return sum(lanes * X.product_mads(X.geometry(cell["bits"], X.geometry_for(cell["bits"], lanes, DEFAULT, DEFAULT8)))
               for call in cell["calls"] for lanes in X.fixed_level_lanes(cell["bits"], call["w"]))


@pytest.mark.parametrize("cell", X.cells(), ids=lambda c: c["id"])
def test_cell(cell, vmn, gpu_ctx, world, thresholds, monkeypatch):
    families = X.OPERATIONS[cell["op"]]["families"]
    launches = {f: sum(call["launches"][f] for call in cell["calls"]) for f in families}
    args = (vmn, gpu_ctx, world, thresholds, monkeypatch)
    own = run(cell, cell["kind"], *args)
    print(cell["id"], own)
    assert not own["wrong"], (cell["id"], own["wrong"])
    assert own["launches"] == launches, (cell["id"], own["launches"])
    kinds = [g["kind"] for g in X.geometries(cell["bits"])]
    if len(kinds) == 1:
        return                                              # 4096 bits: no geometry to tell apart
    # the same calls in every geometry of this modulus size, and as production would run them
    runs = {kind: run(cell, kind, *args) for kind in kinds}
    runs["default"] = run(cell, "default", *args)
    print(cell["id"], {where: r["mads"] for where, r in runs.items()})
    for where, r in runs.items():
        assert not r["wrong"] and r["launches"] == launches, (cell["id"], where, r)
    for f in families:
        figures = [runs[kind]["mads"][f] for kind in kinds]
        assert figures[0] > 0 and all(a < b for a, b in zip(figures, figures[1:])), (cell["id"], f, kinds, figures)
    lands = {X.geometry_for(cell["bits"], X.fixed_items(cell, call) if call["kind"] == "exp_fixed" else X.call_items(cell, call), DEFAULT, DEFAULT8)
             for call in cell["calls"]}
    assert lands == {"wide8" if cell["bits"] == 2048 else "wide"}, (cell["id"], lands)
    land = lands.pop()
    for f in families:
        if f == "fixed_table":
            assert runs["default"]["mads"][f] == pytest.approx(default_fixed_table_mads(cell), rel=REPORT_DIGITS), cell["id"]
        else:
            assert runs["default"]["mads"][f] == runs[land]["mads"][f], (cell["id"], f, land)
