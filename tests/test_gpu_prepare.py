"""bgr_gray_kernel (mvsv_prepare_gray_device) against the numpy restatement, byte
for byte: both grey variants, with and without the halving, on sizes with odd
widths and heights, clipped 2 x 2 blocks, more than one block in x (1281 columns)
and rows that end inside a lane's four pixels.  Every size runs with the source
laid out so that the packed (dword) loads are taken -- base and strides multiples
of 4 -- and so that they cannot be: an odd stride, and a view entered 3 bytes in
(a BGR ROI starting at x = 1).  Everything around the destination view is
pre-filled and must come back untouched."""
import ctypes
import functools

import numpy as np
import pytest

from tests import prepare_restate as ref

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (5, 7), (7, 5), (64, 4), (129, 6), (70, 9), (1281, 5)]  # (width, height)
GUARD = 0xA5


@functools.lru_cache(maxsize=None)
def frames(w, h, n=1):
    """n BGR frames: random bytes; in a batch the second is all 255, the third all 0."""
    f = np.random.default_rng(77 * w + h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    if n >= 3:
        f[1] = 255
        f[2] = 0
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def want(w, h, n, halve, variant):
    out = np.stack([ref.prepare(f, halve, variant) for f in frames(w, h, n)])
    out.setflags(write=False)
    return out


def layouts(w):
    """(name, source base offset, source row stride, destination base offset, destination row pad)"""
    row = 3 * w
    pad16 = (row + 15) // 16 * 16 + 16
    odd = row + 1 if row % 2 == 0 else row + 2
    return [("tight", 0, row, 0, 0), ("padded16", 0, pad16, 4, 8), ("odd", 0, odd, 1, 3), ("3 bytes in", 3, pad16, 2, 0)]


def run_device(torch, src, base, stride, fstride, w, h, halve, variant, dbase, dpad, dfpad):
    """Lay src (n, h, w, 3) out as asked, run the kernel through the C ABI, return
    (result (n, dh, dw), whole destination buffer, mask of the destination view)."""
    from mvstereovision3_amd import _lib
    n = src.shape[0]
    dw, dh = ref.prepare_size(w, h, halve)
    sbuf = np.full(base + (n - 1) * fstride + h * stride + 16, GUARD, np.uint8)
    sview = np.lib.stride_tricks.as_strided(sbuf[base:], (n, h, w, 3), (fstride, stride, 3, 1))
    sview[...] = src
    ds = dw + dpad
    dfs = dh * ds + dfpad
    dbuf = np.full(dbase + n * dfs + 16, GUARD, np.uint8)
    mask = np.zeros(dbuf.shape, bool)
    np.lib.stride_tricks.as_strided(mask[dbase:], (n, dh, dw), (dfs, ds, 1))[...] = True
    ts, td = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf).cuda()
    ctx = _lib.context(0)
    _lib.check(_lib.lib().mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               ctx.handle)
    _lib.check(_lib.lib().mvsv_prepare_gray_device(ctx.handle, n, ts.data_ptr() + base, stride, fstride, w, h,
                                                   1 if halve else 0, variant, td.data_ptr() + dbase, ds, dfs),
               ctx.handle)
    out = td.cpu().numpy()
    got = np.lib.stride_tricks.as_strided(out[dbase:], (n, dh, dw), (dfs, ds, 1)).copy()
    return got, out, mask


def check(got, out, mask, w_, what):
    bad = np.argwhere(got != w_)
    assert bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}"
    assert (out[~mask] == GUARD).all(), f"{what}: bytes outside the destination view were written"


@pytest.mark.parametrize("w,h", SIZES)
def test_single_frames(gpu, w, h):
    for name, base, stride, dbase, dpad in layouts(w):
        for halve in (True, False):
            for variant in (ref.Q14, ref.Q15):
                got, out, mask = run_device(gpu, frames(w, h), base, stride, h * stride, w, h, halve, variant, dbase,
                                            dpad, 0)
                check(got, out, mask, want(w, h, 1, halve, variant), f"{w}x{h} {name} halve={halve} variant={variant}")


@pytest.mark.parametrize("w,h", [(129, 6), (7, 5), (64, 4)])
def test_batches_with_frame_strides(gpu, w, h):
    """n = 3 (random, all 255, all 0) with frame strides larger than the frame: a
    multiple of 4 (packed loads across frames) and an odd one (narrow loads)."""
    src = frames(w, h, 3)
    pad16 = (3 * w + 15) // 16 * 16 + 16
    for name, stride, fstride in [("packed", pad16, h * pad16 + 64), ("odd frame stride", pad16, h * pad16 + 33),
                                  ("tight rows", 3 * w, 3 * w * h + 12)]:
        for halve in (True, False):
            for variant in (ref.Q14, ref.Q15):
                got, out, mask = run_device(gpu, src, 0, stride, fstride, w, h, halve, variant, 3, 5, 17)
                w_ = want(w, h, 3, halve, variant)
                check(got, out, mask, w_, f"{w}x{h} n=3 {name} halve={halve} variant={variant}")
                assert (w_[1] == 255).all() and (w_[2] == 0).all()


def test_python_api(gpu, mvsv):
    """prepare_gray on numpy arrays and device tensors, batches and ROI views."""
    big = frames(129, 6, 3)
    for halve in (True, False):
        for variant in (mvsv.GRAY_Q14, mvsv.GRAY_Q15):
            w_ = want(129, 6, 3, halve, variant)
            assert np.array_equal(mvsv.prepare_gray(big, halve, variant), w_)
            assert np.array_equal(mvsv.prepare_gray(big[0], halve, variant), w_[0])
            t = gpu.from_numpy(np.array(big)).cuda()
            got = mvsv.prepare_gray(t, halve, variant)
            assert got.is_cuda and got.dtype == gpu.uint8 and np.array_equal(got.cpu().numpy(), w_)
            # a BGR ROI starting at x = 1: 3 bytes in, the parent's stride
            roi = t[:, 1:5, 1:72]
            wr = np.stack([ref.prepare(f, halve, variant) for f in big[:, 1:5, 1:72]])
            assert np.array_equal(mvsv.prepare_gray(roi, halve, variant).cpu().numpy(), wr)
            assert np.array_equal(mvsv.prepare_gray(big[:, 1:5, 1:72], halve, variant), wr)


def test_misuse(gpu, mvsv):
    from mvstereovision3_amd import _lib
    lib, ctx = _lib.lib(), _lib.context(0)
    t = gpu.zeros(8 * 8 * 3, dtype=gpu.uint8, device="cuda")
    o = gpu.zeros(64, dtype=gpu.uint8, device="cuda")
    E = _lib.MVSV_E_INVALID_ARG
    call = lambda *a: lib.mvsv_prepare_gray_device(ctx.handle, *a)
    assert call(1, t.data_ptr(), 24, 192, 8, 8, 2, 0, o.data_ptr(), 8, 64) == E      # another factor
    assert call(1, t.data_ptr(), 24, 192, 8, 8, 1, 2, o.data_ptr(), 4, 16) == E      # unknown variant
    assert call(1, t.data_ptr(), 23, 192, 8, 8, 1, 0, o.data_ptr(), 4, 16) == E      # stride < 3 * w
    assert call(1, t.data_ptr(), 24, 192, 8, 8, 1, 0, o.data_ptr(), 3, 16) == E      # dst stride < dw
    assert call(1, t.data_ptr(), 3, 3, 1, 1, 1, 0, o.data_ptr(), 1, 1) == E          # halves to nothing
    assert call(0, t.data_ptr(), 24, 192, 8, 8, 1, 0, o.data_ptr(), 4, 16) == E
    assert call(1, None, 24, 192, 8, 8, 1, 0, o.data_ptr(), 4, 16) == E
    assert lib.mvsv_last_error(ctx.handle)
    assert call(1, t.data_ptr(), 24, 192, 8, 8, 1, 0, o.data_ptr(), 4, 16) == 0      # and the context goes on working
    gpu.cuda.synchronize()
