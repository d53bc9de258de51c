"""CPU suite: the register / spill / scratch report of the kernels behind vmn_permutation_from_prg / _from_keys
(csrc/permutation_kernels.h), cross-compiled for gfx950 in a translation unit of their own.  From the compiler's
-Rpass-analysis=kernel-resource-usage remarks: k_perm_planes, k_perm_hist, k_perm_scatter and k_perm_inverse hold no scratch,
spill nothing and use no accumulation register.  The figures are printed."""
import os

import pytest

from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import compile_report

UNIT = '#include "permutation_kernels.h"\n'
KERNELS = ("k_perm_planes", "k_perm_hist", "k_perm_scatter", "k_perm_inverse")


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    rep = compile_report(str(tmp_path_factory.mktemp("permutation_unit") / "permutation.hip"), UNIT)
    out = {}
    for k in KERNELS:
        hits = [v for name, v in rep.items() if k in name]
        assert len(hits) == 1, (k, sorted(rep))
        out[k] = hits[0]
        print(k, hits[0])
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_the_kernel_holds_no_scratch_and_spills_nothing(reports, kernel):
    r = reports[kernel]
    assert (r["scratch"], r["vspill"], r["sspill"], r["agpr"]) == (0, 0, 0, 0), (kernel, r)
