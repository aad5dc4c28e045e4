"""What the compiler made of the clocked kernels (CPU test; reads the code-object notes as tests/test_code_object.py does).
The clock-scheduled column bands run 8 blocks of 256 threads per CU in fp32 -- the 32-wave cap and the LDS cap at once -- so the kernel
must stay within 64 VGPRs and 20 KiB of LDS, without vector spills or scratch; and its poll loop is scalar code that used to reload
spilled lane masks: the scalar spills must not grow beyond what the kernel had before its tile life was shortened (93 in fp32, 68 in
fp64; 62 and 32 after it).
The LDS bound of 20 KiB is the fp32 kernel's: an fp64 tile's products alone are 24 KiB (3072 slots of 8 bytes) and that kernel has always
run 5 blocks per CU (31 312 bytes with 256 x 11, 20 944 with 256 x 7), so for fp64 the bound is those 5 blocks in 160 KiB."""
import os

import pytest

from conftest import ROOT
from test_code_object import READELF, kernel_resources

PREFIX = "_ZN5mspmv15tile_kernel_vecI"
TAIL = "ENS_7ClockedENS_6AssignENS_8StreamedE"


@pytest.fixture(scope="module")
def product_kernels():
    return kernel_resources(os.path.join(ROOT, "merge_spmv_amd", "libmspmv.so"))


def _one(rows, shape):
    found = [r for n, r in rows.items() if n.startswith(PREFIX + shape + TAIL)]
    assert len(found) == 1, (shape, len(found))
    return found[0]


@pytest.mark.skipif(not os.path.exists(READELF), reason="needs ROCm's llvm-readelf")
def test_clocked_fp32_kernel_keeps_eight_blocks_per_cu(product_kernels):
    r = _one(product_kernels, "fLi256ELi11")
    assert r["vgpr_count"] <= 64, r
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] <= 20480, r
    assert r["sgpr_spill_count"] <= 93, r


@pytest.mark.skipif(not os.path.exists(READELF), reason="needs ROCm's llvm-readelf")
@pytest.mark.parametrize("shape", ["dLi256ELi11", "dLi256ELi7"])
def test_clocked_fp64_kernels(product_kernels, shape):
    r = _one(product_kernels, shape)
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
    assert r["group_segment_fixed_size"] * 5 <= 160 * 1024, r
    assert r["sgpr_spill_count"] <= 68, r
