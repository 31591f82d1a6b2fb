"""SGBM on costs that leave int16, on the device, bit for bit.

Every case of tests/sgbm_wrap_cases.py runs on a fresh context created under the case's
environment and every int16 of every frame is compared with
oracle.sgbm(..., flags = variant | ORC_F_COST_WRAP): the wrapping cost-row update of OpenCV's
non-SIMD build, which is what the cost kernels and the recurrence are written to reproduce
(DESIGN.md §4b-wrap).  The inputs really wrap -- 3 % - 77 % of each cost volume is above 32767,
one case passes 65535 -- and the saturating update would give another map in 2.9 % - 80 % of
the pixels: both are asserted on the CPU by tests/test_sgbm_wrap_cases.py, which also shows
that the table covers every form the general recurrence takes.  Before it computes, a case
asserts the CU count the forms are stated for and the plan word of its context.

The first run of these cases (profiles/sgbm_wrap/README.md) equalled neither update in any
case: the final kernels' S sum read a wrapped cost as unsigned.  They now carry a signed S
(DESIGN.md §4b-wrap).

Reference: Disparity::sgbm (src/disparity.cpp:6-10) -> cv::StereoSGBM::compute."""
import numpy as np
import pytest

from tests import sgbm_wrap_cases as wc
from tests.test_gpu_kernel_forms import check_form, device_batch, fresh_context, matcher  # noqa: F401
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu


def run_case(gpu, mvsv, fresh_context, name):  # noqa: F811
    """The case's maps from the device, one per frame."""
    from mvstereovision3_amd import _lib
    from tests.sgbm_color_restate import one_live_channel
    c = wc.case(name)
    ctx = fresh_context(c.env)
    m = matcher(mvsv, c)
    m.setVariant(c.variant)
    check_form(gpu, ctx, c, m)
    pairs = wc.frames(c)
    with _lib.use_context(ctx):
        if c.kind == "bgr":
            # channel 1 carries the grey pair, the others the constant ftzero (cost 0): the grey pair's map
            L, R = one_live_channel(pairs[0][0], pairs[0][1], 1, max(c.params["pre_filter_cap"], 15) | 1)
            return [m.compute_bgr(L, R)]
        if c.n == 1:
            return [m.compute(pairs[0][0], pairs[0][1])]
        Lb, Rb = device_batch(gpu, pairs)
        out = m.compute(Lb, Rb)
        _lib.synchronize(0)
        return list(out.cpu().numpy())


@pytest.mark.parametrize("name", wc.names())
def test_wrapped_costs(gpu, mvsv, oracle, fresh_context, name):  # noqa: F811
    got = run_case(gpu, mvsv, fresh_context, name)
    refs = wc.references(name)
    assert len(got) == len(refs)
    for i, (g, (flagged, plain)) in enumerate(zip(got, refs)):
        want = flagged if wc.COST_FLAG else plain
        print(f"{name} frame {i}: {int((g != flagged).sum())} of {g.size} differ from the wrapping update, "
              f"{int((g != plain).sum())} from the saturating one")
        assert g.dtype == np.int16 and np.array_equal(g, want), f"{name} {wc.case(name).env} frame {i}: " + report(g, want)
