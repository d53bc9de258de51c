"""CPU suite: the register / spill / scratch report of the kernels of vmn_garray_expprod_arrays (k_modpow_expprod,
csrc/modp_shared_exp.h; k_ec_expprod, csrc/ec_kernels.h), cross-compiled for gfx950 in EVERY geometry of VMN_FOR_SIZES and every
instance of VMN_FOR_CURVES.  Each geometry gets a translation unit of its own, written to a temporary directory, that includes
the tree's headers and instantiates only the new kernel and the kernel it is compared with (a kernel's registers do not depend
on its neighbours in the unit, and the whole instantiation units take minutes each); the units compile side by side.

The criterion is that neither kernel reports a spilled register.  What is asserted, from the compiler's
-Rpass-analysis=kernel-resource-usage remarks (VGPRs, AGPRs, `VGPRs Spill`, `SGPRs Spill`, ScratchSize):
  * k_modpow_expprod, all 12 geometries: 0 spilled VGPRs, 0 spilled SGPRs, no accumulation register, no scratch; in Cfg<74, 1> no
    more VGPRs and no fewer waves than k_modpow_shared<Cfg<74, 1>> of the same tree (both figures are read, none is written
    here).
  * k_ec_expprod within 256 registers per lane (no accumulation register in use: 9 and 10 limbs at two waves): 0 spilled VGPRs,
    0 spilled SGPRs, no scratch.
  * k_ec_expprod above 256 registers per lane (13 limbs and more, and the two instances bound to one wave): no scratch and
    0 spilled SGPRs, but NOT 0 spilled VGPRs.  The criterion is deliberately relaxed there.  The architectural file is full by
    construction, and what the compiler moves into accumulation registers it reports partly as `AGPRs`, partly as
    `VGPRs Spill`: 0 at 13 limbs, 2 at 15 limbs (both kinds), 2 (NIST) and 10 (general) at 21 limbs, where k_ec_add, one bare
    point addition, reports 14 and 18.  Asserted in place of 0: at most S spilled VGPRs -- one field element's worth of moves
    against the 32 S^2 multiply-adds of the one point addition they can occur in, under 0.25 % at S = 13 -- and no more than
    k_ec_add<S, KIND> of the same unit wherever that kernel spills at all."""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from conftest import ROOT
from test_resource_usage import HIPCC

CSRC = os.path.join(ROOT, "verificatum-vmn_amd", "csrc")


def lists():
    """VMN_FOR_SIZES and VMN_FOR_CURVES as vmnhip.hip states them: [(S, NW, LPE)], [(S, NW, kind)]."""
    src = open(os.path.join(CSRC, "vmnhip.hip")).read()
    sizes = re.search(r"#define VMN_FOR_SIZES\(X\)(.*)", src).group(1)
    curves = re.search(r"#define VMN_FOR_CURVES\(X\)((?:.*\\\n)*.*)", src).group(1)
    return ([tuple(int(v) for v in m) for m in re.findall(r"X\((\d+), (\d+), (\d+)\)", sizes)],
            [(int(s), int(nw), k) for s, nw, k in re.findall(r"X\((\d+), (\d+), (EC_\w+)\)", curves)])


SIZES, CURVES = lists()
MODP_UNIT = """#include "modp_shared_exp.h"
template __global__ void vmn::k_modpow_expprod<vmn::Cfg<%(S)d, %(LPE)d>>(vmn::ExpProdArrays, vmn::u32, vmn::u32, const vmn::SlideStep*, vmn::u32,
                                                                 const vmn::u32*, vmn::u32, vmn::u32*);
template __global__ void vmn::k_modpow_shared<vmn::Cfg<%(S)d, %(LPE)d>>(vmn::u32*, const vmn::u32*, const vmn::SlideStep*, int, int, size_t,
                                                                const vmn::u32*, vmn::u32, vmn::u32*);
"""
EC_UNIT = """#include "ec_kernels.h"
template __global__ void vmn::k_ec_expprod<%(S)d, vmn::%(K)s>(vmn::u32*, vmn::ECExpProdArrays, const vmn::SlideStep*, int, size_t, vmn::ECDev, vmn::u32*);
template __global__ void vmn::k_ec_add<%(S)d, vmn::%(K)s>(vmn::u32*, const vmn::u32*, const vmn::u32*, size_t, size_t, vmn::ECDev);
"""


def compile_report(path, text):
    with open(path, "w") as f:
        f.write(text)
    log = subprocess.run([HIPCC, "-std=c++20", "-O3", "--offload-arch=gfx950", "--cuda-device-only", "-fPIC", "-I", CSRC, "-c", path, "-o", path + ".o",
                          "-Rpass-analysis=kernel-resource-usage"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=1800).stdout.decode()
    out = {}
    for block in re.split(r"remark: [^\n]*Function Name: ", log)[1:]:
        get = lambda key: (lambda m: int(m.group(1)) if m else None)(re.search(key + r": (\d+)", block))
        out[block.split()[0]] = {"vgpr": get(r" VGPRs"), "agpr": get("AGPRs"), "vspill": get("VGPRs Spill"), "sspill": get("SGPRs Spill"),
                                 "scratch": get(r"ScratchSize \[bytes/lane\]"), "occupancy": get(r"Occupancy \[waves/SIMD\]")}
    assert out, log[-3000:]
    for name, r in out.items():
        assert None not in r.values(), (name, r)
    return out


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    """{("modp", S, LPE) | ("ec", S, kind): {"new": figures, "old": figures of the kernel compared with}}"""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("expprod_units")
    jobs = {("modp", S, LPE): (str(d / ("modp_%d_%d.hip" % (S, LPE))), MODP_UNIT % dict(S=S, LPE=LPE)) for S, _, LPE in SIZES}
    jobs.update({("ec", S, K): (str(d / ("ec_%d_%s.hip" % (S, K))), EC_UNIT % dict(S=S, K=K)) for S, _, K in CURVES})
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        futures = {key: pool.submit(compile_report, *job) for key, job in jobs.items()}
        raw = {key: f.result() for key, f in futures.items()}
    out = {}
    for key, rep in raw.items():
        new_key, old_key = ("k_modpow_expprod", "k_modpow_shared") if key[0] == "modp" else ("k_ec_expprod", "k_ec_add")
        new = [v for k, v in rep.items() if new_key in k]
        old = [v for k, v in rep.items() if old_key in k]
        assert len(new) == 1 and len(old) == 1, (key, sorted(rep))
        out[key] = {"new": new[0], "old": old[0]}
        print(key, "new", new[0], "compared with", old[0])
    return out


def test_every_geometry_and_every_curve_instance_is_compiled(reports):
    assert len(SIZES) == 12 and len(CURVES) == 9, (SIZES, CURVES)          # the lists were read whole
    assert set(reports) == {("modp", S, LPE) for S, _, LPE in SIZES} | {("ec", S, K) for S, _, K in CURVES}


def test_modular_kernel_needs_no_more_registers_than_the_shared_power_at_2048_bits(reports):
    n, o = reports[("modp", 74, 1)]["new"], reports[("modp", 74, 1)]["old"]
    assert n["vgpr"] <= o["vgpr"] and n["occupancy"] >= o["occupancy"], (n, o)


def test_modular_kernel_spills_nothing_in_any_geometry(reports):
    for key, r in reports.items():
        if key[0] == "modp":
            n = r["new"]
            assert (n["vspill"], n["sspill"], n["scratch"], n["agpr"]) == (0, 0, 0, 0), (key, n)


def test_curve_kernel_spills_nothing_within_256_registers_and_is_bounded_above(reports):
    seen_small = seen_large = 0
    for key, r in reports.items():
        if key[0] != "ec":
            continue
        S, n, o = key[1], r["new"], r["old"]
        assert n["scratch"] == 0 and n["sspill"] == 0, (key, n)
        if n["agpr"] == 0:
            seen_small += 1
            assert n["vspill"] == 0, (key, n)
        else:
            seen_large += 1
            assert n["occupancy"] == 1 and n["vspill"] <= S, (key, n)
            if o["vspill"] > 0:
                assert n["vspill"] <= o["vspill"], (key, n, o)
    assert seen_small >= 2 and seen_small + seen_large == len(CURVES)      # (P-256 and the general 9-limb field fit two waves)
