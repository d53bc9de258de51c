"""CPU suite: the register / scratch report of the shared-exponent kernels whose arrays each walk a schedule of their own
(k_modpow_shared_each, k_modpow_shared_each_phased; csrc/modp_shared_exp.h).  They are the body of k_modpow_shared /
k_modpow_shared_phased with the array, its schedule and its step count picked per tile from a by-value table: the pick must
stay scalar -- no scratch -- and must not cost a wave: every instantiation shows an occupancy not below that of the one-array
kernel of the same geometry in the same report."""
import os
import re

import pytest

from test_resource_usage import HIPCC, report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.parametrize("unit", ["inst_2048", "inst_2048_wide", "inst_small"])
def test_each_array_kernels_no_scratch_and_no_lost_wave(unit, tmp_path):
    rep = report(unit, tmp_path)
    pairs = (("k_modpow_shared_eachINS_3Cfg", "k_modpow_sharedINS_3Cfg"),
             ("k_modpow_shared_each_phasedINS_3Cfg", "k_modpow_shared_phasedINS_3Cfg"))
    seen = set()
    for each_key, one_key in pairs:
        eachs = {k: v for k, v in rep.items() if each_key in k}
        assert eachs, (each_key, sorted(rep)[:5])
        for name, r in eachs.items():
            geometry = re.search(r"CfgILi(\d+)ELi(\d+)E", name).group(0)
            ones = [v for k, v in rep.items() if one_key + geometry[3:] in k]
            assert len(ones) == 1, (name, geometry)
            assert r["scratch"] == 0, (name, r)
            assert r["occupancy"] >= ones[0]["occupancy"], (name, r, ones[0])
            seen.add(geometry)
    want = {"inst_2048": {"CfgILi74ELi1E"}, "inst_2048_wide": {"CfgILi76ELi4E", "CfgILi80ELi8E"},
            "inst_small": {"CfgILi10ELi1E", "CfgILi14ELi1E", "CfgILi19ELi1E", "CfgILi37ELi1E"}}[unit]
    assert seen == want, seen
