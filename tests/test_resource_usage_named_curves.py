"""CPU suite: the register / scratch report (as tests/test_resource_usage.py) of the general-a curve kernels over 10 limbs
(csrc/inst_g10.hip: brainpoolp256r1, secp256k1, prime239v1-3).  The two kernels that add runs of normalised rows -- the first
bucket level of a multi-exponentiation and the fixed-base powers -- must not spill and keep two waves per SIMD, as P-256's do;
the variable-base scalar multiplication stays within the bound P-256's is held to."""
import os

import pytest

from test_resource_usage import HIPCC, report


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_general_a_point_kernels_over_10_limbs_do_not_spill(tmp_path):
    rep = report("inst_g10", tmp_path)
    for key in ("k_ec_bucket_levelILi10ELb1ELi1E", "k_ec_fixed_expILi10ELi1E"):
        hits = {k: v for k, v in rep.items() if key in k}
        assert hits, key
        for name, r in hits.items():
            assert r["scratch"] == 0 and r["occupancy"] >= 2, (name, r)
    hits = {k: v for k, v in rep.items() if "k_ec_mulvarILi10ELi1E" in k}
    assert hits
    for name, r in hits.items():
        assert r["scratch"] <= 240 and r["occupancy"] >= 2, (name, r)
    hits = {k: v for k, v in rep.items() if "k_ec_importILi10ELi8ELi1E" in k}      # (no per-thread byte buffer: see test_resource_usage.py)
    assert hits
    for name, r in hits.items():
        assert r["scratch"] == 0, (name, r)
