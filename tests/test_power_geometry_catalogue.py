"""CPU suite: the catalogue of power-kernel cells (tests/power_geometry_cases.py) itself.  Every (operation x geometry x plain /
phased) cell that exists has a case, and the two that do not are named; every size is ragged against its geometry's tile as
claimed; every phased case is phased by the host's rule under its VMN_MODPOW_MAX_BLOCKS and every plain one is not; the forcing
thresholds reach the geometry a cell names, and under the DEFAULT thresholds every size of the catalogue lands in wide8 (2048
bits) resp. wide (3072 bits) -- which is why only forcing reaches the other cells.  Mutants of the restated rules (never of a
kernel) show that these checks can fail: each is caught by the checks named beside it."""
import pytest

import power_geometry_cases as X


def check_cells(R):
    """every cell that exists has a case; the missing ones are named"""
    have = {(c["op"], c["geometry"], c["form"]) for c in X.cells()}
    for op, spec in X.OPERATIONS.items():
        for geom in X.GEOMETRIES:
            assert (op, geom["name"], "plain") in have, (op, geom["name"])
            if spec["phased"]:
                assert (op, geom["name"], "phased") in have, (op, geom["name"])
            else:
                assert (op, "phased") in X.MISSING_CELLS and (op, geom["name"], "phased") not in have, op
    assert set(X.MISSING_CELLS) == {(op, "phased") for op, spec in X.OPERATIONS.items() if not spec["phased"]}
    assert set(X.MISSING_CELLS) == {("exp_pair", "phased"), ("exp_fixed", "phased")}
    assert [(g["name"], g["S"], g["LPE"], g["EPB"]) for g in X.GEOMETRIES] == [
        ("2048-base", 74, 1, 256), ("2048-wide", 76, 4, 64), ("2048-wide8", 80, 8, 32), ("3072-base", 110, 2, 128), ("3072-wide", 112, 4, 64),
        ("4096-base", 148, 4, 64)]
    assert all(g["force"] == X.FORCE[g["kind"]] for g in X.GEOMETRIES)
    assert X.FORCE == {"base": (0, 0), "wide": (2 ** 63, 0), "wide8": (2 ** 63, 2 ** 63)}
    for c in X.cells():
        for call in c["calls"]:
            assert set(call["launches"]) == set(X.OPERATIONS[c["op"]]["families"]), c["id"]
            if "k" in call:
                assert call["launches"]["modpow"] == R.launches(call["k"]) == (2 if call["k"] == 9 else 1), c["id"]
    assert {call["k"] for c in X.cells() if c["op"] == "exp_scalar_multi" for call in c["calls"]} == {3, 9}


def check_sizes(R):
    """every size is ragged against its EPB as claimed"""
    for c in X.cells():
        epb, n = X.geometry(c["bits"], c["kind"])["EPB"], c["n"]
        if c["op"] == "exp_fixed":
            assert n == X.FIXED_N == 200, c["id"]
            continue
        if c["op"] == "exp_pair":
            sizes = {(call["nx"], call["ny"]) for call in c["calls"]}
            assert sizes == {(epb - 1, epb - 1), (epb + 1, epb - 1), (epb - 1, epb + 1)}, c["id"]
            continue
        assert n % epb != 0, c["id"]
        if c["form"] == "plain" or c["arrays"] > 1:
            assert n in (epb - 1, epb + 1) and R.tiles(n, epb) == (1 if n == epb - 1 else 2), c["id"]     # one ragged tile; a second tile of one element
            assert R.tiles(n, epb, c["arrays"]) == c["arrays"] * (1 if n == epb - 1 else 2), c["id"]
        else:
            assert n == 2 * epb + epb // 2 + 1 and R.tiles(n, epb) == 3 and c["max_blocks"] == 2, c["id"]     # three tiles on two slots, the third ragged
        assert n <= X.nmax(c["bits"]) <= 641 and (c["arrays"] == 1 or n <= X.multi_nmax(c["bits"])), c["id"]
    assert X.nmax(2048) == 641 and {c["n"] for c in X.cells() if c["id"].startswith("exp_array-2048-base-phased")} == {641}
    for op in ("exp_scalar_multi", "exp_scalars_multi"):
        for geom in X.GEOMETRIES:
            got = {(c["n"], c["max_blocks"]) for c in X.cells() if c["op"] == op and c["geometry"] == geom["name"] and c["form"] == "phased"}
            assert got == {(n, mb) for n in (geom["EPB"] - 1, geom["EPB"] + 1) for mb in (2, 1)}, (op, geom["name"])


def check_forms(R):
    """every phased case is phased under its VMN_MODPOW_MAX_BLOCKS, every plain case is not"""
    for c in X.cells():
        if not X.OPERATIONS[c["op"]]["phased"]:
            assert c["form"] == "plain" and c["max_blocks"] is None, c["id"]
            continue
        epb = X.geometry(c["bits"], c["kind"])["EPB"]
        for call, steps in zip(c["calls"], X.cuttable_steps(c)):
            k = call.get("k", 1)
            groups = [min(X.SHARED_ARRAYS, k - a0) for a0 in range(0, k, X.SHARED_ARRAYS)]          # the arrays of each launch
            if c["form"] == "phased":
                assert c["max_blocks"] in (1, 2) and c["env"]["VMN_MODPOW_MAX_BLOCKS"] == str(c["max_blocks"]), c["id"]
                assert all(R.is_phased(c["n"], epb, ga, c["max_blocks"], steps) for ga in groups), (c["id"], call)
                if c["arrays"] > 1 and c["n"] == epb - 1:
                    assert not R.is_phased(c["n"], epb, 1, c["max_blocks"], steps), (c["id"], "no array alone would be phased")
            else:
                assert c["max_blocks"] is None and "VMN_MODPOW_MAX_BLOCKS" not in c["env"], c["id"]
                assert not any(R.is_phased(c["n"], epb, ga, None, steps) for ga in groups), (c["id"], call)
    # 1 << 200 is a schedule of two steps: with one step to cut there are no phases, so it stays in the plain cells
    assert X.slide_steps(1 << 200, X.sliding_window_bits(201)) == 2
    assert not R.is_phased(641, 256, 1, 2, 1) and R.is_phased(641, 256, 1, 2, 2)


def _calls_items(c):
    for call in c["calls"]:
        if call["kind"] == "exp_fixed":
            yield X.fixed_items(c, call)
        else:
            yield X.call_items(c, call)
            if call.get("k", 1) > X.SHARED_ARRAYS:
                yield (call["k"] - X.SHARED_ARRAYS) * c["n"]


def check_forced(R):
    """the thresholds of a cell's geometry send every launch of the cell there"""
    for c in X.cells():
        geom = X.geometry(c["bits"], c["kind"])
        for items in _calls_items(c):
            assert R.geometry_for(c["bits"], items, *geom["force"]) == c["kind"], (c["id"], items)
        for call in c["calls"]:
            if call["kind"] == "exp_fixed":
                assert all(R.geometry_for(c["bits"], lanes, *geom["force"]) == c["kind"] for lanes in X.fixed_level_lanes(c["bits"], call["w"]))


def check_default(R):
    """under the default thresholds every size of the catalogue runs wide8 at 2048 bits and wide at 3072 bits"""
    assert X.DEFAULT_THRESHOLDS == (40960, 6144)
    lands = {2048: "wide8", 3072: "wide", 4096: "base"}
    for c in X.cells():
        for items in _calls_items(c):
            assert R.geometry_for(c["bits"], items, *X.DEFAULT_THRESHOLDS) == lands[c["bits"]], (c["id"], items)


CHECKS = {"cells": check_cells, "sizes": check_sizes, "forms": check_forms, "forced": check_forced, "default": check_default}


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_the_catalogue_holds_under_the_hosts_rules(name):
    CHECKS[name](X.RULES)


def test_inputs_are_as_the_cells_describe_them():
    for bits in X.BITS:
        I = X.inputs(bits)
        p, q, sh = I["p"], I["q"], I["shared"]
        assert p.bit_length() == bits and len(I["xs"]) == X.MULTI_K == X.SHARED_ARRAYS + 1
        assert len(I["xs"][0]) == len(I["ys"]) == len(I["es"]) == len(I["fs"]) == X.nmax(bits)
        assert all(len(x) == X.multi_nmax(bits) for x in I["xs"][1:]) and len({tuple(x[:8]) for x in I["xs"]}) == X.MULTI_K      # distinct arrays
        assert I["xs"][0][0] == 1 and I["xs"][0][1] == p - 1 and all(0 < v < p for x in I["xs"] for v in x)
        assert sh["full"].bit_length() == q.bit_length() and sh["full"] >> (q.bit_length() - 2) == 3 and sh["full"] < q
        assert (sh["q-1"], sh["(1<<33)+1"], sh["1<<200"], sh["short"]) == (q - 1, (1 << 33) + 1, 1 << 200, 0xC0FFEE11)
        assert sh["short"].bit_length() == 32 and sh["e200"].bit_length() == 200 and sh["e256"].bit_length() == 256 and sh["zero"] == 0
        assert all(sh[name].bit_length() > 32 for name in ("full", "q-1", "(1<<33)+1", "1<<200", "e200"))
        assert sh["e700"].bit_length() > 41                                   # the shared exponent longer than every f
        assert I["es"][:4] == [0, 1, q - 1, 1 << (q.bit_length() - 1)] and all(0 <= e < q for e in I["es"])
        assert I["fs"][:3] == [0, 1 << 612, (1 << 613) - 1] and max(I["fs"]).bit_length() == 613
        assert len(I["fixed_es"]) == X.FIXED_N and I["fixed_es"][:4] == I["es"][:4]
        # 200 elements are cut into pieces under the default fill, for every window of the catalogue
        assert all(X.fixed_parts(X.FIXED_N, X.fixed_nwin(bits, w)) == 16 and X.fixed_parts(X.FIXED_N, X.fixed_nwin(bits, w), 0) == 1
                   for w in X.FIXED_WINDOWS)


class IgnoresTiny(X.Rules):
    def geometry_for(self, bits, items, small, tiny, always=False):
        return super().geometry_for(bits, items, small, 0, always)


class IgnoresSmall(X.Rules):
    def geometry_for(self, bits, items, small, tiny, always=False):
        return super().geometry_for(bits, items, 0, tiny, always)


class TilesOf256(X.Rules):
    def tiles(self, n, epb, arrays=1):
        return super().tiles(n, 256, arrays)


class PhasedFromEqual(X.Rules):
    def is_phased(self, n, epb, arrays, max_blocks, cuttable_steps):
        return self.tiles(n, epb, arrays) >= min(X.DEVICE_BLOCKS, max_blocks or X.DEVICE_BLOCKS) and cuttable_steps >= 2


@pytest.mark.parametrize("mutant,caught_by", [(IgnoresTiny, {"forced", "default"}), (IgnoresSmall, {"forced", "default"}),
                                              (TilesOf256, {"sizes", "forms"}), (PhasedFromEqual, {"forms"})])
def test_a_mutant_of_the_rules_is_caught_by_the_named_checks(mutant, caught_by):
    failed = {}
    for name, check in CHECKS.items():
        try:
            check(mutant())
        except AssertionError as err:
            failed[name] = str(err)[:200]
    print(mutant.__name__, "caught by:", {name: failed[name] for name in sorted(failed)})
    assert set(failed) == caught_by, (mutant.__name__, failed)
