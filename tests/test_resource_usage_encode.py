"""CPU suite: the register / spill / scratch report of the kernels of the text interface behind a session, cross-compiled for
gfx950 in translation units of their own that include the tree's headers: the four byte-level kernels of csrc/encode_kernels.h
(k_textlines_records, k_textlines_fold, k_textlines_lengths, k_textlines_emit) and the residue fix of csrc/modp_kernels.h in every
geometry it is instantiated in (k_jacobi_fix with one lane per element up to 2048 bits, k_jacobi_fix_lanes above), each beside the
membership kernel of the same geometry, with which it shares the Jacobi loop.  From the compiler's
-Rpass-analysis=kernel-resource-usage remarks: no kernel holds scratch, none spills a vector or a scalar register, none uses an
accumulation register; and the fix -- which reads its row again for the store instead of keeping a second copy -- stays within
the 2 S <= 148 + a few registers of the membership kernel's loop: at most 8 VGPRs more in any geometry."""
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import compile_report

TEXT_KERNELS = ("k_textlines_records", "k_textlines_fold", "k_textlines_lengths", "k_textlines_emit")
ONE_LANE = ((10, 1), (14, 1), (19, 1), (37, 1), (74, 1))
LANES = ((110, 2), (148, 4), (296, 8), (592, 16))
JACOBI_UNIT = """#include "modp_kernels.h"
template __global__ void vmn::k_jacobi_member%(sfx)s<vmn::Cfg<%(S)d, %(LPE)d>>(const vmn::u32*, size_t, const vmn::u32*, vmn::u32*);
template __global__ void vmn::k_jacobi_fix%(sfx)s<vmn::Cfg<%(S)d, %(LPE)d>>(vmn::u32*, size_t, const vmn::u32*);
"""


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("encode_units")
    jobs = {"text": (str(d / "textlines.hip"), '#include "encode_kernels.h"\n')}
    for S, LPE in ONE_LANE + LANES:
        jobs[(S, LPE)] = (str(d / ("jacobi_%d_%d.hip" % (S, LPE))), JACOBI_UNIT % dict(S=S, LPE=LPE, sfx="" if LPE == 1 else "_lanes"))
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        futures = {key: pool.submit(compile_report, *job) for key, job in jobs.items()}
        raw = {key: f.result() for key, f in futures.items()}
    out = {}
    for k in TEXT_KERNELS:
        hits = [v for name, v in raw["text"].items() if k in name]
        assert len(hits) == 1, (k, sorted(raw["text"]))
        out[k] = hits[0]
        print(k, hits[0])
    for key in ONE_LANE + LANES:
        fix = [v for name, v in raw[key].items() if "k_jacobi_fix" in name]
        member = [v for name, v in raw[key].items() if "k_jacobi_member" in name]
        assert len(fix) == 1 and len(member) == 1, (key, sorted(raw[key]))
        out[key] = {"fix": fix[0], "member": member[0]}
        print(key, "fix", fix[0], "member", member[0])
    return out


@pytest.mark.parametrize("kernel", TEXT_KERNELS)
def test_the_text_kernels_hold_no_scratch_and_spill_nothing(reports, kernel):
    r = reports[kernel]
    assert (r["scratch"], r["vspill"], r["sspill"], r["agpr"]) == (0, 0, 0, 0), (kernel, r)


@pytest.mark.parametrize("geometry", ONE_LANE + LANES)
def test_the_residue_fix_fits_like_the_membership_kernel(reports, geometry):
    fix, member = reports[geometry]["fix"], reports[geometry]["member"]
    for r in (fix, member):
        assert (r["scratch"], r["vspill"], r["sspill"], r["agpr"]) == (0, 0, 0, 0), (geometry, r)
    assert fix["vgpr"] <= member["vgpr"] + 8 and fix["occupancy"] >= min(member["occupancy"], 2), (geometry, fix, member)
