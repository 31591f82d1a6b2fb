"""The kernel forms only switches and full frames reach, on the device, bit for bit.

Every case of tests/kernel_form_cases.py runs on a fresh context created under the case's
environment (one context per environment setting, closed when the setting changes) and
every frame is compared with oracle.sgbm / oracle.bm through np.array_equal.  Before it
computes, a case asserts that the device has the CU count the table was checked for, that
mvsv_sgbm_plan of its context gives the plan word the host check printed for the case
(tests/test_kernel_forms.py compares that word with the stated form: this ties
mvsv_create's environment parsing to the KernelOptions of the table) and, on schedule 0,
that path_aggregation counts one launch per direction.

The library reports nothing that tells apart the tile height, the band permutation, the
placement of the L->R lines, the cost kernel or the BM kernel: for those the host check
of tests/test_kernel_forms.py, which runs sgbm_make_plan on the same options and shape,
is the evidence that the case reaches its form.

Groups: tile heights 24..120 (MVSV_COST_TY) at image heights TY - 1, TY + 1, 2 TY + 3; the
XCD band permutation of sgbm_cost2_kernel with MVSV_COST_XCD unset and 0; the general
kernels MVSV_KERNELS selects; MVSV_LINES_AUX 0 / 1 / 2 with batches A, B, A back to back.
Reference: Disparity::sgbm / Disparity::bm (src/disparity.cpp:6-22) -> cv::StereoSGBM /
cv::StereoBM::compute."""
import numpy as np
import pytest

from tests import kernel_form_cases as kc
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh_context():
    """fresh_context(env) -> a context created under exactly `env` (every other launch-shape
    variable unset).  One context lives at a time: it is closed when another setting is asked for."""
    from mvstereovision3_amd import _lib
    live = {}

    def close():
        for ctx in live.values():
            ctx.close()
        live.clear()

    def get(env):
        key = tuple(sorted(env.items()))
        if key not in live:
            close()
            with pytest.MonkeyPatch.context() as mp:
                for name in kc.ENV_ALL:
                    mp.delenv(name, raising=False)
                for k, v in env.items():
                    mp.setenv(k, v)
                live[key] = _lib.Context(0)  # a fresh context reads the environment
        return live[key]

    try:
        yield get
    finally:
        close()


def matcher(mvsv, c):
    p = c.params
    if c.kind == "bm":
        m = mvsv.StereoBM.create(p["num_disparities"], p["block_size"])
        for k, v in p.items():
            setattr(m._params, k, v)
        return m
    return mvsv.StereoSGBM.create(p["min_disparity"], p["num_disparities"], p["block_size"], p["p1"], p["p2"],
                                  p["disp12_max_diff"], p["pre_filter_cap"], p["uniqueness_ratio"],
                                  p["speckle_window_size"], p["speckle_range"], p["mode"])


def want_maps(oracle, c, pairs):
    return [oracle.bm(L, R, c.params) if c.kind == "bm" else oracle.sgbm(L, R, c.params) for L, R in pairs]


def check_form(gpu, ctx, c, m):
    """The CU count the table was checked for, and the plan word of this context."""
    from mvstereovision3_amd import _lib
    assert gpu.cuda.get_device_properties(0).multi_processor_count == kc.CUS, "the table's forms are stated for 256 CUs"
    if c.kind != "bm":
        got = _lib.sgbm_plan(ctx, c.n, c.W, c.H, m._params, 3 if c.kind == "bgr" else 1)
        assert got == c.form["bits"], f"{c.name}: plan word {got} under {c.env}, the host check gives {c.form['bits']}"


def device_batch(gpu, pairs):
    dev = gpu.device("cuda", 0)
    return (gpu.from_numpy(np.stack([q[0] for q in pairs])).to(dev), gpu.from_numpy(np.stack([q[1] for q in pairs])).to(dev))


def run_case(gpu, mvsv, oracle, fresh_context, name):
    from mvstereovision3_amd import _lib
    from tests.sgbm_color_restate import one_live_channel
    c = kc.case(name)
    ctx = fresh_context(c.env)
    m = matcher(mvsv, c)
    check_form(gpu, ctx, c, m)
    pairs = kc.frames(c)
    count = "launches" in c.form
    with _lib.use_context(ctx):
        if count:
            _lib.profile_reset(ctx)
            _lib.profile_enable(ctx, True)
        try:
            if c.kind == "bgr":
                # channel 1 carries the grey pair, the others the constant ftzero (cost 0): the grey pair's map
                L, R = one_live_channel(pairs[0][0], pairs[0][1], 1, max(c.params["pre_filter_cap"], 15) | 1)
                got = [m.compute_bgr(L, R)]
            elif c.n == 1:
                got = [m.compute(pairs[0][0], pairs[0][1])]
            else:
                Lb, Rb = device_batch(gpu, pairs)
                out = m.compute(Lb, Rb)
                _lib.synchronize(0)
                got = list(out.cpu().numpy())
        finally:
            if count:
                _lib.profile_enable(ctx, False)
        if count:
            # schedule 0: one launch per direction (4: MODE_SGBM, 7: MODE_HH); R->L is the final kernel's
            launches = _lib.profile_read(ctx)["path_aggregation"][1]
            assert launches == c.form["launches"], f"{name}: path_aggregation counted {launches} launches"
    for i, (g, w) in enumerate(zip(got, want_maps(oracle, c, pairs))):
        assert np.array_equal(g, w), f"{name} {c.env} frame {i}: " + report(g, w)


@pytest.mark.parametrize("name", kc.names("ty"))
def test_cost_tile_heights(gpu, mvsv, oracle, fresh_context, name):
    """Tile heights 24..120 of both cost kernels: the register-ring kernel with the residual
    plane (and MODE_HH's pinned bottom rows), with LDS ring slots (blockSize 15) and with the
    bit-sliced emission, the LDS-ring kernel on a colour pair; a tile taller than the image, a
    last tile of one row, three tiles with a short last one.  (The tile height is the host
    check's evidence.)"""
    run_case(gpu, mvsv, oracle, fresh_context, name)


@pytest.mark.parametrize("name", kc.names("xcd"))
def test_cost_band_permutation(gpu, mvsv, oracle, fresh_context, name):
    """sgbm_cost2_kernel's XCD renumbering of its blocks at 8 and 24 row bands x frames, two
    and three tile columns, bands of one frame and of several, against blockIdx order
    (MVSV_COST_XCD=0) and a 9-band control.  (Whether it applies is the host check's evidence.)"""
    run_case(gpu, mvsv, oracle, fresh_context, name)


@pytest.mark.parametrize("name", kc.names("gen"))
def test_general_kernels(gpu, mvsv, oracle, fresh_context, name):
    """MVSV_KERNELS: the one-wave-per-scanline path and final kernels (their full forms at
    D 128 / 256), the LDS-ring cost kernel on grey pairs, both together, the 16-lane kernels
    one launch per direction, the register-ring cost kernel without a compile-time pair count,
    and the 16x16-tile BM kernel, each on shapes the specialised kernels cover."""
    run_case(gpu, mvsv, oracle, fresh_context, name)


@pytest.mark.parametrize("name", kc.names("lines"))
def test_lines_placement_back_to_back(gpu, mvsv, oracle, fresh_context, name):
    """The L->R lines on the context stream after the strips (0), on the second stream before
    (1) and after them (2): batch A, a different batch B and A again on one context with no
    synchronisation between the calls; all nine frames are read after the last call.  A wait
    missing between the second stream and the next call's kernels would mix the batches."""
    from mvstereovision3_amd import _lib
    c = kc.case(name)
    ctx = fresh_context(c.env)
    m = matcher(mvsv, c)
    check_form(gpu, ctx, c, m)
    A, B = kc.frames(c, 0), kc.frames(c, 1)
    assert not any(np.array_equal(a[0], b[0]) for a in A for b in B)
    dA, dB = device_batch(gpu, A), device_batch(gpu, B)
    outs = [gpu.empty((c.n, c.H, c.W), dtype=gpu.int16, device=dA[0].device) for _ in range(3)]
    gpu.cuda.synchronize()
    with _lib.use_context(ctx):
        for (Lb, Rb), out in zip((dA, dB, dA), outs):
            m.compute(Lb, Rb, out)
        _lib.synchronize(0)
    got = [o.cpu().numpy() for o in outs]
    wA, wB = want_maps(oracle, c, A), want_maps(oracle, c, B)
    for call, (g, w) in enumerate(zip(got, (wA, wB, wA))):
        for i in range(c.n):
            assert np.array_equal(g[i], w[i]), f"{name} call {call} frame {i}: " + report(g[i], w[i])
