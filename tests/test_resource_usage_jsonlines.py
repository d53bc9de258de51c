"""CPU suite: the register / spill / scratch report of the kernels of the json ciphertext interface (csrc/decimal_kernels.h:
k_jsonlines_scan, k_dec_to_rows, k_rows_to_dec, k_jsonlines_emit, and the two small kernels of the 64-bit line offsets,
k_jsonlines_lengths and k_jsonlines_offsets), cross-compiled for gfx950 in a translation unit of its own that includes the
tree's header.  From the compiler's -Rpass-analysis=kernel-resource-usage remarks: no kernel holds scratch, none spills a
vector or a scalar register, none uses an accumulation register."""
import os

import pytest

from test_resource_usage import HIPCC
from test_resource_usage_expprod_arrays import compile_report

KERNELS = ("k_jsonlines_scan", "k_dec_to_rows", "k_rows_to_dec", "k_jsonlines_emit", "k_jsonlines_lengths", "k_jsonlines_offsets")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("jsonlines_unit")
    rep = compile_report(str(d / "jsonlines.hip"), '#include "decimal_kernels.h"\n')
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
