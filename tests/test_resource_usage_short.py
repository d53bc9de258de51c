"""CPU suite: the register / scratch report of the two power kernels on the short rows, k_modpow<Cfg<74, 1>, true> and
k_modpow_phased<Cfg<74, 1>, true> (csrc/inst_2048_short.hip) -- as tests/test_resource_usage.py reads it for the kernels on the
general rows, and with its bounds: two waves per SIMD, no more scratch than the prologue's few dwords.  The short kernels hold two
modulus limbs and -1/N less, and load N itself once per element where they leave the domain; neither may cost a spill in the rows."""
import os

import pytest

from test_resource_usage import HIPCC, report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_short_row_kernels_keep_two_waves_and_the_general_kernels_scratch_bounds(tmp_path):
    rep = report("inst_2048_short", tmp_path)
    plain = {k: v for k, v in rep.items() if "k_modpowINS_3CfgILi74ELi1EEELb1E" in k}
    phased = {k: v for k, v in rep.items() if "k_modpow_phasedINS_3CfgILi74ELi1EEELb1E" in k}
    assert len(plain) == 1 and len(phased) == 1, sorted(rep)
    for name, r in plain.items():
        assert r["occupancy"] == 2 and r["scratch"] <= 256, (name, r)
    for name, r in phased.items():
        assert r["occupancy"] == 2 and r["scratch"] <= 320, (name, r)
