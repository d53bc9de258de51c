"""CPU suite: the register / spill / scratch report of k_rows_segments, the kernel behind vmn_garray_from_segments
(csrc/light_kernels.h), cross-compiled for gfx950 in a translation unit of its own.  From the compiler's
-Rpass-analysis=kernel-resource-usage remarks: the kernel holds no scratch, spills nothing and uses no accumulation register.
The figures are printed."""
import os

import pytest

from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import compile_report

UNIT = '#include "light_kernels.h"\n'
KERNEL = "k_rows_segments"


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    rep = compile_report(str(tmp_path_factory.mktemp("rearrange_unit") / "rearrange.hip"), UNIT)
    hits = [v for name, v in rep.items() if KERNEL in name]
    assert len(hits) == 1, (KERNEL, sorted(rep))
    print(KERNEL, hits[0])
    return hits[0]


def test_the_kernel_holds_no_scratch_and_spills_nothing(report):
    assert (report["scratch"], report["vspill"], report["sspill"], report["agpr"]) == (0, 0, 0, 0), report
