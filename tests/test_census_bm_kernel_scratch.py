"""No scratch in the kernels a census StereoBM call adds (CPU test on the built library, in
the way of tests/test_census_kernel_scratch.py): every instance of the lanes kernel
(2 disparity blocks x 9 block sizes x 2 descriptor widths) and both of the general form."""
import os
import re

import pytest

from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_census_bm_kernels_have_no_scratch():
    ks = kernel_scratch()
    lanes = {k: v for k, v in ks.items() if re.search(r"bm_census_match2_kernel", k)}
    general = {k: v for k, v in ks.items() if re.search(r"bm_census_match_kernel", k)}
    assert len(lanes) == 2 * 9 * 2, sorted(lanes)
    assert len(general) == 2, sorted(general)
    bad = {k: v for k, v in {**lanes, **general}.items() if v}
    assert not bad, f"census BM kernels with scratch: {bad}"
