"""CPU suite: the register / spill / scratch report of the kernels of the native ciphertext interface (csrc/light_kernels.h:
k_hexlines_count and k_hexlines_walk, the line discovery; k_hexlines_decode; k_hexlines_encode), cross-compiled for gfx950 in a
translation unit of its own that includes the tree's header.  From the compiler's -Rpass-analysis=kernel-resource-usage remarks:
no kernel holds scratch, none spills a vector or a scalar register, none uses an accumulation register."""
import os

import pytest

from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import compile_report

KERNELS = ("k_hexlines_count", "k_hexlines_walk", "k_hexlines_decode", "k_hexlines_encode")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("hexlines_unit")
    rep = compile_report(str(d / "hexlines.hip"), '#include "light_kernels.h"\n')
    out = {}
    for k in KERNELS:
        hits = [v for name, v in rep.items() if k in name]
        assert len(hits) == 1, (k, sorted(rep))
        out[k] = hits[0]
        print(k, hits[0])
    return out


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_scratch_and_no_spills(report, kernel):
    r = report[kernel]
    assert (r["scratch"], r["vspill"], r["sspill"], r["agpr"]) == (0, 0, 0, 0), (kernel, r)
