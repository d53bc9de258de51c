"""CPU suite: the register / spill / scratch report of the kernels of the text interface over curve groups
(csrc/ec_encode_kernels.h), cross-compiled for gfx950 in translation units of their own that include the tree's headers.  From the
compiler's -Rpass-analysis=kernel-resource-usage remarks: k_ec_textlines_fold holds no scratch, spills nothing and uses no
accumulation register; the same holds for k_ec_encode_search and k_ec_encode_root of the NIST kind at S = 10 (P-256) and S = 15
(P-384); of the general kind at S = 10 their scratch stays within the 240 bytes that tests/test_resource_usage_named_curves.py
grants the general-a point kernels of that size.  The figures are printed (DESIGN.md's table is taken from them)."""
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import compile_report

UNIT = """#include "ec_encode_kernels.h"
template __global__ void vmn::k_ec_encode_search<%(S)d, %(NW)d, vmn::%(K)s>(vmn::u32*, const uint8_t*, size_t, vmn::u32, vmn::ECDev, vmn::u32*);
template __global__ void vmn::k_ec_encode_root<%(S)d, vmn::%(K)s, false>(vmn::u32*, size_t, vmn::ECDev, vmn::u32*);
"""
SHAPES = ((10, 8, "EC_NIST"), (15, 12, "EC_NIST"), (10, 8, "EC_GENERAL"))
NEW_KERNELS = ("k_ec_encode_search", "k_ec_encode_root")


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("point_text_units")
    jobs = {(S, K): (str(d / ("ec_encode_%d_%s.hip" % (S, K))), UNIT % dict(S=S, NW=NW, K=K)) for S, NW, K in SHAPES}
    with ThreadPoolExecutor(max_workers=min(4, os.cpu_count() or 1)) as pool:
        futures = {key: pool.submit(compile_report, *job) for key, job in jobs.items()}
        raw = {key: f.result() for key, f in futures.items()}
    out = {}
    for key, rep in raw.items():
        for k in NEW_KERNELS + ("k_ec_textlines_fold",):
            hits = [v for name, v in rep.items() if k in name]
            assert len(hits) == 1, (key, k, sorted(rep))
            out[key + (k,)] = hits[0]
            print(key, k, hits[0])
    return out


def test_the_fold_holds_no_scratch_and_spills_nothing(reports):
    r = reports[(10, "EC_NIST", "k_ec_textlines_fold")]
    assert (r["scratch"], r["vspill"], r["sspill"], r["agpr"]) == (0, 0, 0, 0), r


@pytest.mark.parametrize("S", (10, 15))
@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_search_and_root_of_the_nist_kind_hold_no_scratch_and_spill_nothing(reports, S, kernel):
    r = reports[(S, "EC_NIST", kernel)]
    assert (r["scratch"], r["vspill"], r["sspill"], r["agpr"]) == (0, 0, 0, 0), (S, kernel, r)


@pytest.mark.parametrize("kernel", NEW_KERNELS)
def test_search_and_root_of_the_general_kind_stay_within_the_scratch_of_its_point_kernels(reports, kernel):
    r = reports[(10, "EC_GENERAL", kernel)]
    assert r["scratch"] <= 240, (kernel, r)
