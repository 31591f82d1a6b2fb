"""No scratch in the kernels a census call adds (CPU test on the built library, in the
way of tests/test_hh4_kernel_scratch.py): the census transform, the census form of the
LDS-ring cost kernel, and the LDS-ring kernels it shares its device code with."""
import os
import re

import pytest

from tests.test_kernel_scratch import LIB, LLVM, kernel_scratch


@pytest.mark.skipif(not os.path.exists(LIB) or not os.path.exists(f"{LLVM}/llvm-readelf"),
                    reason="library not built / no ROCm llvm tools")
def test_census_kernels_have_no_scratch():
    ks = kernel_scratch()
    picked = {}
    for pat in (r"census_kernel", r"sgbm_cost_census_kernel", r"sgbm_cost_kernelILi1E", r"sgbm_cost_kernelILi3E"):
        hit = {k: v for k, v in ks.items() if re.search(pat, k)}
        assert hit, f"no kernel matches {pat}"
        picked.update(hit)
    # the transform and the cost form are two kernels, not one name matched twice
    assert any("sgbm_cost_census_kernel" in k for k in picked)
    assert any(re.search(r"\d+census_kernel", k) and "cost" not in k for k in picked)
    bad = {k: v for k, v in picked.items() if v}
    assert not bad, f"census kernels with scratch: {bad}"
