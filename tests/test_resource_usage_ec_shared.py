"""CPU suite: the register / spill / scratch report of the curve power under one scalar (k_ec_mulshared, csrc/ec_kernels.h),
cross-compiled for gfx950 in every instance of VMN_FOR_CURVES, after the pattern of tests/test_resource_usage_expprod_arrays.py:
a translation unit per instance, written to a temporary directory, that includes the tree's headers and instantiates the new
kernel with the eight-array descriptor that carries a schedule per array (ECEachArrays, the heaviest of the three) and
k_ec_expprod of the same instance, the kernel its loop is modelled on; the units compile side by side.

Asserted, from the compiler's -Rpass-analysis=kernel-resource-usage remarks:
  * every instance: no scratch, 0 spilled SGPRs;
  * where k_ec_expprod reports no accumulation register (10 limbs with a = -3, 9 limbs with a general a): 0 spilled VGPRs and no
    fewer waves per SIMD than k_ec_expprod;
  * elsewhere: at most S spilled VGPRs and no more than k_ec_expprod reports (there what the compiler moves into accumulation
    registers it reports partly as `AGPRs`, partly as `VGPRs Spill`, see the docstring of the pattern)."""
import os

import pytest

from conftest import ROOT
from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import CURVES, compile_report

from concurrent.futures import ThreadPoolExecutor

EC_UNIT = """#include "ec_kernels.h"
template __global__ void vmn::k_ec_mulshared<%(S)d, vmn::%(K)s, vmn::ECEachArrays>(vmn::ECEachArrays, vmn::u32, vmn::u32, const vmn::ECSharedStep*, int, int,
                                                                           size_t, vmn::ECDev, vmn::u32*);
template __global__ void vmn::k_ec_expprod<%(S)d, vmn::%(K)s>(vmn::u32*, vmn::ECExpProdArrays, const vmn::SlideStep*, int, size_t, vmn::ECDev, vmn::u32*);
"""


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    """{(S, kind): {"new": figures of k_ec_mulshared, "old": figures of k_ec_expprod}}"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("ec_shared_units")
    jobs = {(S, K): (str(d / ("ec_%d_%s.hip" % (S, K))), EC_UNIT % dict(S=S, K=K)) for S, _, K in CURVES}
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        futures = {key: pool.submit(compile_report, *job) for key, job in jobs.items()}
        raw = {key: f.result() for key, f in futures.items()}
    out = {}
    for key, rep in raw.items():
        new = [v for k, v in rep.items() if "k_ec_mulshared" in k]
        old = [v for k, v in rep.items() if "k_ec_expprod" in k]
        assert len(new) == 1 and len(old) == 1, (key, sorted(rep))
        out[key] = {"new": new[0], "old": old[0]}
        print(key, "new", new[0], "compared with", old[0])
    return out


def test_every_curve_instance_is_compiled(reports):
    assert len(CURVES) == 9 and set(reports) == {(S, K) for S, _, K in CURVES}


def test_no_scratch_and_no_spilled_scalar_register_anywhere(reports):
    for key, r in reports.items():
        assert r["new"]["scratch"] == 0 and r["new"]["sspill"] == 0, (key, r["new"])


def test_spills_and_waves_against_the_kernel_the_loop_is_modelled_on(reports):
    clean = bounded = 0
    for (S, K), r in reports.items():
        n, o = r["new"], r["old"]
        if o["agpr"] == 0:
            clean += 1
            assert n["vspill"] == 0 and n["occupancy"] >= o["occupancy"], ((S, K), n, o)
        else:
            bounded += 1
            assert n["vspill"] <= S and n["vspill"] <= o["vspill"], ((S, K), n, o)
    assert clean >= 2 and clean + bounded == len(CURVES)                   # (P-256 and the general 9-limb field fit two waves)
