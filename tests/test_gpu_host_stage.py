"""The host-pointer calls against their _device siblings, and against each other on
one context (GPU).

Every host-pointer call stages one frame through the context's arena
(csrc/mvsv_stage.hpp) and runs the _device call on it.  So the same numpy input,
once through the host entry point from a view whose rows are 5 elements wider than
the image, once as a contiguous device tensor through the _device entry point, must
give the same bits: maps, images, min / max, counts and sums.  Then a sequence of
calls of different sizes on one context, where one call's slices land on what another
call left behind, with and without an mvsv_trim in the middle: every result must be
the one a fresh context gives for that call alone.

Shapes: 37 x 23 for the map and image calls (a ragged tail on the 8-element, the
4-byte and the tight row rule), 70 x 41 with 16 disparities for the matchers and tm
(accepted by their validation, not a multiple of 8 wide).  mvsv_dmap2pcl shares
host_cloud with mvsv_point_cloud and keeps its own file tests."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 37, 23      # maps and images
MW, MH = 70, 41    # matchers, tm, and the view that grows the arena
P = ctypes.c_void_p


def wide(a):
    """A view of a copy of `a` (H, W[, C]) whose rows are 5 pixels wider than the image."""
    buf = np.full((a.shape[0], a.shape[1] + 5) + a.shape[2:], 113, a.dtype)
    buf[:, :a.shape[1]] = a
    v = buf[:, :a.shape[1]]
    assert v.strides[0] == (a.shape[1] + 5) * a[0, 0].nbytes and not v.flags.c_contiguous
    return v


@pytest.fixture(scope="module")
def inputs(mvsv):
    rng = np.random.default_rng(20261021)
    inp = {}
    for w, h in ((W, H), (MW, MH)):
        d = rng.integers(-40, 900, (h, w)).astype(np.int16)
        d[rng.random((h, w)) < 0.3] = 0
        inp["dmap", w, h] = wide(d)
        _, _, nx, ny = mvsv.samplepoint_layout(w, h)
        inp["means", w, h] = rng.uniform(0, 900, 81).astype(np.float32)
        inp["values", w, h] = rng.uniform(0, 900, nx * ny).astype(np.float32)
    inp["img"] = wide(rng.integers(0, 256, (H, W), dtype=np.uint8))
    inp["img2"] = wide(rng.integers(0, 256, (H, W), dtype=np.uint8))
    inp["bgr"] = wide(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
    L, R = mvsv.synth_pair(7, MW, MH, 0, 16)
    inp["L"], inp["R"] = wide(L), wide(R)
    inp["Lbgr"] = wide(np.stack([L, np.roll(L, 1, 0), 255 - L], -1))
    inp["Rbgr"] = wide(np.stack([R, np.roll(R, 1, 0), 255 - R], -1))
    Q = np.eye(4, dtype=np.float32)
    Q[0, 3], Q[1, 3], Q[2, 3], Q[3, 2], Q[2, 2] = -W / 2, -H / 2, 30.0, 0.25, 0.0
    inp["Q"] = np.ascontiguousarray(Q.reshape(16))
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float32)
    inp["maps"] = [np.ascontiguousarray(m) for m in (xs + 0.37, ys - 0.21, xs - 1.6, ys + 0.74)]
    inp["K"] = np.array([[30.0, 0, W / 2], [0, 31.0, H / 2], [0, 0, 1]], np.float64)
    inp["dist"] = np.array([0.05, -0.02, 0.001, -0.002, 0.003], np.float64)
    return inp


class Calls:
    """The fifteen host-pointer calls and their _device twins on one context, each
    returning its results as a tuple of numpy arrays."""

    def __init__(self, mvsv, torch, inp):
        from mvstereovision3_amd import _lib
        self._lib, self.lib, self.torch, self.inp, self.mvsv = _lib, _lib.lib(), torch, inp, mvsv
        self.ctx = _lib.Context(0)
        self.h = self.ctx.handle
        self.sgbm_p = _lib.SgbmParams()
        self.lib.mvsv_sgbm_params_default(ctypes.byref(self.sgbm_p))
        self.sgbm_p.num_disparities, self.sgbm_p.block_size = 16, 5
        self.sgbm_p.speckle_window_size, self.sgbm_p.speckle_range = 20, 2
        self.bm_p = _lib.BmParams()
        self.lib.mvsv_bm_params_default(ctypes.byref(self.bm_p), 16, 9)

    def close(self):
        self.ctx.close()

    def ok(self, rc):
        self._lib.check(rc, self.h)

    def on_host(self):
        self.ok(self.lib.mvsv_use_own_stream(self.h))

    def dev(self, a):
        """`a` as a contiguous device tensor, the context bound to the current stream."""
        t = self.torch.as_tensor(np.ascontiguousarray(a), device="cuda:0")
        self.ok(self.lib.mvsv_set_stream(self.h, P(self.torch.cuda.current_stream(t.device).cuda_stream)))
        return t

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device="cuda:0")

    def trim(self):
        self.ok(self.lib.mvsv_trim(self.h))

    # ---- matchers and tm -------------------------------------------------------
    def _match(self, host, fn, params, L, R, cn):
        if host:
            out = np.empty((MH, MW), np.int16)
            self.on_host()
            self.ok(fn(self.h, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], MW, MH, ctypes.byref(params),
                       out.ctypes.data, MW))
            return (out,)
        l, r, out = self.dev(L), self.dev(R), self.empty((MH, MW), self.torch.int16)
        self.ok(fn(self.h, 1, l.data_ptr(), MW * cn, MW * MH * cn, r.data_ptr(), MW * cn, MW * MH * cn, MW, MH,
                   ctypes.byref(params), out.data_ptr(), MW, MW * MH))
        return (out.cpu().numpy(),)

    def sgbm(self, host):
        fn = self.lib.mvsv_sgbm if host else self.lib.mvsv_sgbm_device
        return self._match(host, fn, self.sgbm_p, self.inp["L"], self.inp["R"], 1)

    def sgbm_bgr(self, host):
        fn = self.lib.mvsv_sgbm_bgr if host else self.lib.mvsv_sgbm_bgr_device
        return self._match(host, fn, self.sgbm_p, self.inp["Lbgr"], self.inp["Rbgr"], 3)

    def bm(self, host):
        fn = self.lib.mvsv_bm if host else self.lib.mvsv_bm_device
        return self._match(host, fn, self.bm_p, self.inp["L"], self.inp["R"], 1)

    def tm(self, host):
        L, R, k = self.inp["L"], self.inp["R"], 5
        if host:
            out = np.empty((MH, MW), np.uint8)
            self.on_host()
            self.ok(self.lib.mvsv_tm(self.h, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], MW, MH, k,
                                     out.ctypes.data, MW))
            return (out,)
        l, r, out = self.dev(L), self.dev(R), self.empty((MH, MW), self.torch.uint8)
        self.ok(self.lib.mvsv_tm_device(self.h, 1, l.data_ptr(), MW, MW * MH, r.data_ptr(), MW, MW * MH, MW, MH, k,
                                        out.data_ptr(), MW, MW * MH, 1))
        return (out.cpu().numpy(),)

    # ---- map calls ---------------------------------------------------------------
    def mean_grid(self, host):
        d = self.inp["dmap", W, H]
        if host:
            out = np.empty(81, np.float32)
            self.on_host()
            self.ok(self.lib.mvsv_mean_disparity_grid(self.h, d.ctypes.data, d.strides[0] // 2, W, H, out.ctypes.data))
            return (out,)
        t, out = self.dev(d), self.empty((81,), self.torch.float32)
        self.ok(self.lib.mvsv_mean_disparity_grid_device(self.h, 1, t.data_ptr(), W, W * H, W, H, out.data_ptr()))
        return (out.cpu().numpy(),)

    def samplepoints(self, host):
        d, n = self.inp["dmap", W, H], len(self.inp["values", W, H])
        assert n > 0
        if host:
            out = np.empty(n, np.float32)
            self.on_host()
            self.ok(self.lib.mvsv_samplepoint_values(self.h, d.ctypes.data, d.strides[0] // 2, W, H, 2, out.ctypes.data))
            return (out,)
        t, out = self.dev(d), self.empty((n,), self.torch.float32)
        self.ok(self.lib.mvsv_samplepoint_values_device(self.h, 1, t.data_ptr(), W, W * H, W, H, 2, out.data_ptr()))
        return (out.cpu().numpy(),)

    def normalize(self, host):
        d = self.inp["dmap", W, H]
        if host:
            out, mm = np.empty((H, W), np.uint8), np.empty(2, np.int16)
            self.on_host()
            self.ok(self.lib.mvsv_normalize_minmax(self.h, d.ctypes.data, d.strides[0] // 2, W, H, 0.0, 255.0,
                                                   out.ctypes.data, W, mm.ctypes.data))
            return out, mm
        t, out, mm = self.dev(d), self.empty((H, W), self.torch.uint8), self.empty((2,), self.torch.int16)
        self.ok(self.lib.mvsv_normalize_minmax_device(self.h, 1, t.data_ptr(), W, W * H, W, H, 0.0, 255.0,
                                                      out.data_ptr(), W, W * H, mm.data_ptr()))
        return out.cpu().numpy(), mm.cpu().numpy()

    def view(self, host, w=W, h=H):
        d, means, values = self.inp["dmap", w, h], self.inp["means", w, h], self.inp["values", w, h]
        spec = self.mvsv.utility.view_spec(15, (600.0, 100.0), (700.0, 50.0), 2)
        if host:
            out, mm = np.empty((h, w, 3), np.uint8), np.empty(2, np.int16)
            spec.means, spec.values = means.ctypes.data, values.ctypes.data
            self.on_host()
            self.ok(self.lib.mvsv_view(self.h, d.ctypes.data, d.strides[0] // 2, w, h, ctypes.byref(spec),
                                       out.ctypes.data, 3 * w, mm.ctypes.data))
            return out, mm
        t, tm, tv = self.dev(d), self.dev(means), self.dev(values)
        out, mm = self.empty((h, w, 3), self.torch.uint8), self.empty((2,), self.torch.int16)
        spec.means, spec.values = tm.data_ptr(), tv.data_ptr()
        self.ok(self.lib.mvsv_view_device(self.h, 1, t.data_ptr(), w, w * h, w, h, ctypes.byref(spec), out.data_ptr(),
                                          3 * w, 3 * w * h, mm.data_ptr()))
        return out.cpu().numpy(), mm.cpu().numpy()

    def big_view(self, host):
        return self.view(host, MW, MH)

    def cloud(self, host, cap=W * H):
        d, Q = self.inp["dmap", W, H], self.inp["Q"]
        if host:
            rec, count, mm = np.zeros((cap, 4), np.float32), ctypes.c_int(-1), np.empty(2, np.int32)
            self.on_host()
            self.ok(self.lib.mvsv_point_cloud(self.h, d.ctypes.data, d.strides[0] // 2, W, H, Q.ctypes.data,
                                              rec.ctypes.data, cap, ctypes.byref(count), mm.ctypes.data))
            n = count.value
        else:
            t = self.dev(d)
            rec, cnt = self.empty((cap, 4), self.torch.float32), self.empty((1,), self.torch.int32)
            mm = self.empty((2,), self.torch.int32)
            self.ok(self.lib.mvsv_point_cloud_device(self.h, 1, t.data_ptr(), W, W * H, W, H, Q.ctypes.data,
                                                     rec.data_ptr(), cap, cnt.data_ptr(), mm.data_ptr()))
            rec, n, mm = rec.cpu().numpy(), int(cnt.cpu()[0]), mm.cpu().numpy()
        assert n > 10  # both a full and a clipped cloud have records
        return rec[:min(n, cap)].view(np.int32), np.array([n]), mm

    def small_cloud(self, host):
        return self.cloud(host, 10)

    # ---- image calls -------------------------------------------------------------
    def resize(self, host):
        a, fx, fy = self.inp["img"], 0.6, 1.7
        dw, dh = self.mvsv.rectify.resize_size(W, H, fx, fy)
        if host:
            out = np.empty((dh, dw), np.uint8)
            self.on_host()
            self.ok(self.lib.mvsv_resize(self.h, a.ctypes.data, a.strides[0], W, H, fx, fy, out.ctypes.data, dw))
            return (out,)
        t, out = self.dev(a), self.empty((dh, dw), self.torch.uint8)
        self.ok(self.lib.mvsv_resize_device(self.h, 1, t.data_ptr(), W, W * H, W, H, fx, fy, out.data_ptr(), dw, dw * dh))
        return (out.cpu().numpy(),)

    def prepare_gray(self, host):
        a = self.inp["bgr"]
        dw, dh = self.mvsv.prepare_size(W, H, True)
        if host:
            out = np.empty((dh, dw), np.uint8)
            self.on_host()
            self.ok(self.lib.mvsv_prepare_gray(self.h, a.ctypes.data, a.strides[0], W, H, 1, 0, out.ctypes.data, dw))
            return (out,)
        t, out = self.dev(a), self.empty((dh, dw), self.torch.uint8)
        self.ok(self.lib.mvsv_prepare_gray_device(self.h, 1, t.data_ptr(), 3 * W, 3 * W * H, W, H, 1, 0, out.data_ptr(),
                                                  dw, dw * dh))
        return (out.cpu().numpy(),)

    def rectify(self, host):
        L, R, maps = self.inp["img"], self.inp["img2"], self.inp["maps"]
        x0, y0, x1, y1 = 2, 1, 35, 22
        if host:
            oL, oR = np.empty((y1 - y0, x1 - x0), np.uint8), np.empty((y1 - y0, x1 - x0), np.uint8)
            arr = (P * 4)(*[m.ctypes.data for m in maps])
            roi = self._lib.Rect(x0, y0, x1, y1)
            self.on_host()
            self.ok(self.lib.mvsv_rectify_pair(self.h, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], W, H,
                                               arr, ctypes.byref(roi), oL.ctypes.data, x1 - x0, oR.ctypes.data, x1 - x0))
            return oL, oR
        outs = []
        for side, img in enumerate((L, R)):
            t, mx, my = self.dev(img), self.dev(maps[2 * side]), self.dev(maps[2 * side + 1])
            out = self.empty((H, W), self.torch.uint8)
            self.ok(self.lib.mvsv_remap_device(self.h, 1, t.data_ptr(), W, W * H, W, H, mx.data_ptr(), my.data_ptr(), W,
                                               out.data_ptr(), W, W * H, W, H))
            outs.append(out.cpu().numpy()[y0:y1, x0:x1])
        return tuple(outs)

    def sharpness(self, host):
        a, roi = self.inp["img"], self._lib.Rect(3, 2, 33, 20)
        if host:
            value, s4 = ctypes.c_double(), ctypes.c_int64()
            self.on_host()
            self.ok(self.lib.mvsv_sharpness(self.h, a.ctypes.data, a.strides[0], W, H, ctypes.byref(roi),
                                            ctypes.byref(value), ctypes.byref(s4)))
            assert value.value == self.mvsv.utility.sharpness_value(s4.value, 30 * 18)
            return (np.array([s4.value], np.int64),)
        t, out = self.dev(a), self.empty((1,), self.torch.int64)
        self.ok(self.lib.mvsv_sharpness_device(self.h, 1, t.data_ptr(), W, W * H, W, H, ctypes.byref(roi), out.data_ptr()))
        return (out.cpu().numpy(),)

    def undistort(self, host, in_place=False):
        K, dist = self.inp["K"], self.inp["dist"]
        if host:
            # in place: the outputs are the (strided) inputs themselves
            L, R = (wide(self.inp["img"]), wide(self.inp["img2"])) if in_place else (self.inp["img"], self.inp["img2"])
            oL, oR = (L, R) if in_place else (np.empty((H, W), np.uint8), np.empty((H, W), np.uint8))
            self.on_host()
            self.ok(self.lib.mvsv_undistort_pair(self.h, L.ctypes.data, L.strides[0], R.ctypes.data, R.strides[0], W, H,
                                                 K.ctypes.data, dist.ctypes.data, 5, K.ctypes.data, None, 0,
                                                 oL.ctypes.data, oL.strides[0], oR.ctypes.data, oR.strides[0]))
            return np.array(oL), np.array(oR)
        outs = []
        for img, dc in ((self.inp["img"], dist), (self.inp["img2"], None)):
            xy, frac = self.mvsv.undistort_maps(K, dc, (W, H))
            t, txy, tfr = self.dev(img), self.dev(xy), self.dev(frac.view(np.int16))
            out = self.empty((H, W), self.torch.uint8)
            self.ok(self.lib.mvsv_remap_fixed_device(self.h, 1, t.data_ptr(), W, W * H, W, H, txy.data_ptr(), W,
                                                     tfr.data_ptr(), W, out.data_ptr(), W, W * H, W, H))
            outs.append(out.cpu().numpy())
        return tuple(outs)

    def undistort_in_place(self, host):
        return self.undistort(host, in_place=True)


ALL = ["sgbm", "sgbm_bgr", "bm", "tm", "mean_grid", "samplepoints", "normalize", "view", "cloud", "small_cloud",
       "resize", "prepare_gray", "rectify", "sharpness", "undistort", "undistort_in_place"]
# the order of the issue's sequence: small, a larger one that grows the arena, small again, ...
SEQUENCE = ["normalize", "big_view", "cloud", "sgbm", "sharpness", "undistort_in_place"]


def same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: result {k}: {g.dtype}{g.shape} != {w.dtype}{w.shape}"
        assert g.tobytes() == w.tobytes(), f"{what}: result {k} differs in {int((g != w).sum())} elements"


@pytest.fixture(scope="module")
def calls(gpu, mvsv, inputs):
    c = Calls(mvsv, gpu, inputs)
    yield c
    c.close()


@pytest.fixture(scope="module")
def alone(gpu, mvsv, inputs):
    """Each call of SEQUENCE on a fresh context that runs nothing else."""
    ref = {}
    for name in SEQUENCE:
        c = Calls(mvsv, gpu, inputs)
        ref[name] = getattr(c, name)(True)
        c.close()
    return ref


@pytest.mark.parametrize("name", ALL)
def test_host_call_equals_device_call(calls, name):
    host = getattr(calls, name)(True)
    device = getattr(calls, name)(False)
    same(host, device, name)
    assert all(r.any() for r in host), f"{name}: an all-zero result proves nothing"


def test_sequence_on_one_context_equals_each_call_alone(gpu, mvsv, inputs, alone):
    c = Calls(mvsv, gpu, inputs)
    try:
        for name in SEQUENCE:
            same(getattr(c, name)(True), alone[name], f"{name} in sequence")
        for name in reversed(SEQUENCE):  # and every slice over the leftovers of a larger call
            same(getattr(c, name)(True), alone[name], f"{name} in reversed sequence")
    finally:
        c.close()


def test_trim_in_the_middle_of_a_sequence(gpu, mvsv, inputs, alone):
    c = Calls(mvsv, gpu, inputs)
    try:
        for k, name in enumerate(SEQUENCE):
            if k in (2, 4):
                c.trim()
            same(getattr(c, name)(True), alone[name], f"{name} after a trim" if k in (2, 4) else name)
    finally:
        c.close()
