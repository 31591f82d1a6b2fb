"""The post filters on the device, fed chosen maps: mvsv_filter_speckles_device (the
four-launch lock-free union-find of mvsv_post.hip) and mvsv_median_blur3_device (the
packed and the scalar 3x3 median) against the C oracle, bit for bit.

The maps are those of tests/post_filter_cases.py (checked on the CPU by
tests/test_post_filter_cases.py): one component through every tile, sizes exactly on
maxSpeckleSize, every pixel its own root, thresholds on maxDiff, the int16 extremes,
every shape around the tile size -- contiguous, as strided / misaligned views, in
batches, on a context that ran a larger map before, and on more workgroups than the
device has CUs.  No tolerances: these are integer filters."""
import numpy as np
import pytest

from tests import post_filter_cases as pfc
from tests.test_gpu_parity import report

pytestmark = pytest.mark.gpu

CASES = pfc.all_cases()
PAD = 12345  # what the parent buffers hold outside a view

_want = {}


def speckle_want(oracle, m, new_val, size, max_diff, key=None):
    """The oracle's result, computed once per (case, max_size)."""
    if key is None:
        return oracle.filter_speckles(m, new_val, size, max_diff)
    k = (key, new_val, size, max_diff)
    if k not in _want:
        r = oracle.filter_speckles(m, new_val, size, max_diff)
        r.setflags(write=False)
        _want[k] = r
    return _want[k]


class Embedded:
    """frames (H, W) or (N, H, W) as a view of a larger flat int16 device buffer filled
    with PAD: row stride W + row_pad, frame stride H * (W + row_pad) + frame_pad, first
    element at `offset`."""

    def __init__(self, torch, frames, row_pad=0, offset=0, frame_pad=0):
        a = np.asarray(frames)
        self.batched = a.ndim == 3
        a3 = a if self.batched else a[None]
        n, H, W = a3.shape
        self.shape = (n, H, W)
        self.rs = W + row_pad
        self.fs = H * self.rs + frame_pad
        self.offset = offset
        total = offset + n * self.fs + 5
        self.parent = torch.full((total,), PAD, dtype=torch.int16, device="cuda")
        v = self.parent.as_strided((n, H, W), (self.fs, self.rs, 1), offset)
        v.copy_(torch.from_numpy(np.array(a3, np.int16)).cuda())  # a copy: the cases are read-only
        self.view = v if self.batched else v[0]

    def _host_view(self, flat):
        return np.lib.stride_tricks.as_strided(flat[self.offset:], self.shape,
                                               (2 * self.fs, 2 * self.rs, 2), writeable=False)

    def read(self):
        """(the view's content, whether every element outside it is still PAD)"""
        flat = self.parent.cpu().numpy()
        inside = np.zeros(flat.shape, bool)
        mask = np.lib.stride_tricks.as_strided(inside[self.offset:], self.shape, (self.fs, self.rs, 1))
        mask[...] = True
        got = np.array(self._host_view(flat))
        return (got if self.batched else got[0]), bool(np.all(flat[~inside] == PAD))


def run_speckle(torch, mvsv, m, new_val, size, max_diff, **embed):
    e = Embedded(torch, m, **embed)
    ret = mvsv.filter_speckles(e.view, new_val, size, max_diff)
    assert ret is e.view  # in place, returns its argument
    got, pad_ok = e.read()
    assert pad_ok, "the filter wrote outside its view"
    return got


# ------------------------------------------------------------------ speckle filter -----
@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_speckle_cases_contiguous(gpu, mvsv, oracle, c):
    for s in c.sizes:
        t = gpu.from_numpy(np.array(c.map)).cuda()
        assert t.is_contiguous()
        got = mvsv.filter_speckles(t, c.new_val, s, c.max_diff).cpu().numpy()
        want = speckle_want(oracle, c.map, c.new_val, s, c.max_diff, c.name)
        assert np.array_equal(got, want), f"{c.name} max_size {s}: " + report(got, want)


VIEW_CASES = [c for c in CASES if c.name.startswith(("serpentine", "comb", "noise"))]


@pytest.mark.parametrize("parity", ["odd", "even"])
@pytest.mark.parametrize("c", VIEW_CASES, ids=[c.name for c in VIEW_CASES])
def test_speckle_cases_as_views(gpu, mvsv, oracle, c, parity):
    """Row strides W + 7 and W + 40 -- whichever of the two is odd / even at this width --
    and the first element at an odd offset; the parent's padding stays."""
    W = c.map.shape[1]
    row_pad = 7 if ((W + 7) % 2 == 1) == (parity == "odd") else 40
    assert (W + row_pad) % 2 == (1 if parity == "odd" else 0)
    for s in c.sizes:
        got = run_speckle(gpu, mvsv, c.map, c.new_val, s, c.max_diff, row_pad=row_pad, offset=3)
        want = speckle_want(oracle, c.map, c.new_val, s, c.max_diff, c.name)
        assert np.array_equal(got, want), f"{c.name} max_size {s} stride W+{row_pad} ({parity}): " + report(got, want)


def check_batch(oracle, got, frames, new_val, size, max_diff, what):
    for f, m in enumerate(frames):
        want = speckle_want(oracle, m, new_val, size, max_diff)
        assert np.array_equal(got[f], want), f"{what}, frame {f}: " + report(got[f], want)


@pytest.mark.parametrize("names,max_diff,size", [
    (("noise_167x203", "serpentine_167x203", "checker_167x203"), 16, 50),
    (("noise_holes_md80_167x203", "comb_167x203", "noise_167x203"), 64, 200),
    (("serpentine_far_64x64", "checker_64x64", "serpentine_64x64"), 16, pfc.case("serpentine_64x64").sizes[0]),
    (("serpentine_far_64x64", "checker_64x64", "serpentine_64x64"), 16, pfc.case("serpentine_64x64").sizes[1]),
])
def test_speckle_batch_of_three_contiguous(gpu, mvsv, oracle, names, max_diff, size):
    """Three different cases of one shape in one launch, frame stride W * H."""
    frames = np.stack([pfc.case(n).map for n in names])
    t = gpu.from_numpy(frames).cuda()
    assert t.stride(0) == frames.shape[1] * frames.shape[2]
    got = mvsv.filter_speckles(t, -16, size, max_diff).cpu().numpy()
    check_batch(oracle, got, frames, -16, size, max_diff, f"{names} max_size {size}")


@pytest.mark.parametrize("W,H", [(40, 6), (64, 32), (33, 33)])
def test_speckle_frames_do_not_join(gpu, mvsv, oracle, W, H):
    """Frame f ends and frame f + 1 begins with a full row of one value, and the frames lie
    back to back in memory: a filter that took the batch for one tall image would join the
    two rows into a component of 2 W pixels.  Per frame they are W pixels each."""
    m = np.full((H, W), -16, np.int16)
    m[0] = m[H - 1] = 400
    m[1:H - 1, W // 2] = np.where(np.arange(H - 2) % 2 == 0, 900, -16)  # lone pixels in between
    frames = np.stack([m, m, m])
    for size, rows_kept in ((W - 1, True), (W, False), (2 * W - 1, False)):
        got = mvsv.filter_speckles(gpu.from_numpy(frames).cuda(), -16, size, 16).cpu().numpy()
        check_batch(oracle, got, frames, -16, size, 16, f"max_size {size}")
        assert bool(np.all(got[:, 0] == 400) and np.all(got[:, H - 1] == 400)) == rows_kept


@pytest.mark.parametrize("frame_pad,row_pad,offset", [(37, 0, 0), (1, 0, 0), (64, 9, 1)])
def test_speckle_batch_with_padded_frames(gpu, mvsv, oracle, frame_pad, row_pad, offset):
    frames = np.stack([pfc.case(n).map for n in ("noise_97x130", "spiral_97x130", "noise_holes_md80_97x130")])
    for size in (50, pfc.case("spiral_97x130").sizes[0], pfc.case("spiral_97x130").sizes[1]):
        got = run_speckle(gpu, mvsv, frames, -16, size, 64, row_pad=row_pad, offset=offset, frame_pad=frame_pad)
        check_batch(oracle, got, frames, -16, size, 64, f"frame stride W*H+{frame_pad} max_size {size}")


def test_speckle_context_reuse(gpu, mvsv, oracle):
    """One context, maps of changing size: the root list must be rewound by every run, and no
    parent / size / tile / local-root word of an earlier, larger run may leak into a later one."""
    from mvstereovision3_amd import _lib
    noise, small = pfc.case("noise_167x203"), pfc.case("shape_33x33")
    snake, checker = pfc.case("serpentine_167x203"), pfc.case("checker_167x203")
    order = [(noise, 200), (small, 10), (snake, snake.sizes[0]), (small, 10), (checker, 1), (noise, 200)]
    ctx = _lib.Context(0)
    results = []
    try:
        with _lib.use_context(ctx):
            for c, s in order:
                t = gpu.from_numpy(np.array(c.map)).cuda()
                results.append(mvsv.filter_speckles(t, c.new_val, s, c.max_diff).cpu().numpy())
            # the snake removed whole, right after the run that filled the root list
            t = gpu.from_numpy(np.array(snake.map)).cuda()
            results.append(mvsv.filter_speckles(t, snake.new_val, snake.sizes[1], snake.max_diff).cpu().numpy())
            order.append((snake, snake.sizes[1]))
            _lib.check(_lib.lib().mvsv_synchronize(ctx.handle), ctx.handle)
    finally:
        ctx.close()
    for k, ((c, s), got) in enumerate(zip(order, results)):
        want = speckle_want(oracle, c.map, c.new_val, s, c.max_diff, c.name)
        assert np.array_equal(got, want), f"call {k} ({c.name}, max_size {s}): " + report(got, want)
    assert results[0].tobytes() == results[5].tobytes()


def test_speckle_more_border_blocks_than_cus(gpu, mvsv, oracle):
    """4 frames of 640x480 near-critical noise: 1200 tiles, 300 border blocks per launch, so the
    cross-tile unions run concurrently on every CU.  Twice; both runs equal the oracle."""
    frames = np.stack([pfc.noise(640, 480, seed=700 + f)[0] for f in range(4)])
    runs = []
    for _ in range(2):
        t = gpu.from_numpy(frames).cuda()
        runs.append(mvsv.filter_speckles(t, -16, 1000, 64).cpu().numpy())
    assert np.array_equal(runs[0], runs[1]), "two runs of one launch differ"
    for f in range(4):
        want = speckle_want(oracle, frames[f], -16, 1000, 64)
        removed = np.count_nonzero(want != frames[f]) / want.size
        assert 0.10 <= removed <= 0.90, removed
        assert np.array_equal(runs[0][f], want), f"frame {f}: " + report(runs[0][f], want)


def test_speckle_arguments(gpu, mvsv):
    t = gpu.zeros((8, 8), dtype=gpu.int16, device="cuda")
    for bad in (32768, -32769):
        with pytest.raises(mvsv.MvsvError):
            mvsv.filter_speckles(t, bad, 10, 16)
    with pytest.raises(mvsv.MvsvError):
        mvsv.filter_speckles(t.t(), 0, 10, 16)  # column stride 8: no in-place form
    with pytest.raises(mvsv.MvsvError):
        mvsv.filter_speckles(t.to(gpu.int32), 0, 10, 16)
    with pytest.raises(mvsv.MvsvError):
        mvsv.filter_speckles(t.cpu(), 0, 10, 16)


# -------------------------------------------------------------------------- median -----
def odd_pad(W):
    return 1 if W % 2 == 0 else 2   # W + pad is odd


def even_pad(W):
    return 2 if W % 2 == 0 else 1   # W + pad is even


# name -> (source row_pad, source offset, destination row_pad, destination offset); with an even
# width only the first two meet the packed kernel's conditions, every other form is scalar
def median_forms(W):
    return {
        "contiguous": (0, 0, 0, 0),
        "even strides, aligned": (even_pad(W), 2, even_pad(W) + 2, 4),
        "odd source stride": (odd_pad(W), 0, even_pad(W), 0),
        "odd destination stride": (even_pad(W), 0, odd_pad(W), 0),
        "source starts at an odd element": (even_pad(W), 1, even_pad(W), 0),
        "destination starts at an odd element": (even_pad(W), 0, even_pad(W), 3),
    }


def run_median(torch, mvsv, src, form, frame_pads=(0, 0)):
    sp, so, dp, do = form
    s = Embedded(torch, src, row_pad=sp, offset=so, frame_pad=frame_pads[0])
    d = Embedded(torch, np.full(np.shape(src), PAD, np.int16), row_pad=dp, offset=do, frame_pad=frame_pads[1])
    ret = mvsv.median_blur3(s.view, out=d.view)
    assert ret is d.view
    got, pad_ok = d.read()
    assert pad_ok, "the median wrote outside its destination view"
    back, src_pad_ok = s.read()
    assert src_pad_ok and np.array_equal(back, src), "the median changed its source"
    return got


@pytest.mark.parametrize("H,W", pfc.MEDIAN_SHAPES)
def test_median_every_form(gpu, mvsv, oracle, H, W):
    wrong = []  # every form is run, so that a failure names all the forms (kernels) it hits
    for kind in ("full", "corners"):
        src = pfc.median_map(H, W, kind)
        want = oracle.median3x3(src)
        for name, form in median_forms(W).items():
            got = run_median(gpu, mvsv, src, form)
            if not np.array_equal(got, want):
                wrong.append(f"{H}x{W} {kind}, {name}: " + report(got, want))
        got = mvsv.median_blur3(gpu.from_numpy(src).cuda()).cpu().numpy()  # allocates its result
        if not np.array_equal(got, want):
            wrong.append(f"{H}x{W} {kind}, own result: " + report(got, want))
    assert not wrong, "\n".join(wrong)


@pytest.mark.parametrize("H,W", [(37, 130), (37, 131), (33, 64)])
@pytest.mark.parametrize("frame_pads", [(1, 0), (0, 1), (3, 5), (2, 4), (0, 0)],
                         ids=["odd src frames", "odd dst frames", "odd both", "even", "packed frames"])
def test_median_batch_of_three(gpu, mvsv, oracle, H, W, frame_pads):
    """An odd frame stride puts every second frame on an odd element: scalar kernel; an even
    one keeps the packed kernel (even W)."""
    src = np.stack([pfc.median_map(H, W, "full", seed=1), pfc.median_map(H, W, "corners", seed=2),
                    pfc.median_map(H, W, "full", seed=3)])
    got = run_median(gpu, mvsv, src, (even_pad(W), 0, even_pad(W), 0), frame_pads)
    for f in range(3):
        want = oracle.median3x3(src[f])
        assert np.array_equal(got[f], want), f"frame {f}: " + report(got[f], want)


def test_median_of_the_twin_agrees(oracle):
    from oracle import twin
    src = pfc.median_map(37, 131, "corners")
    assert np.array_equal(oracle.median3x3(src), twin.median3x3(src))


def test_median_overlap_is_refused(gpu, mvsv):
    buf = gpu.zeros((40, 64), dtype=gpu.int16, device="cuda")
    with pytest.raises(mvsv.MvsvError):
        mvsv.median_blur3(buf, out=buf)
    with pytest.raises(mvsv.MvsvError):
        mvsv.median_blur3(buf[:32], out=buf[8:])      # shifted by eight rows
    with pytest.raises(mvsv.MvsvError):
        mvsv.median_blur3(buf[:20], out=buf[19:39])   # one shared row
    with pytest.raises(mvsv.MvsvError):
        mvsv.median_blur3(buf[:20], out=buf[20:39])   # shape mismatch
    mvsv.median_blur3(buf[:20], out=buf[20:])         # back to back: fine
    gpu.cuda.synchronize()


# --------------------------------------------------------------------- composition -----
def noisy_pair(seed, W, H, shift):
    rng = np.random.default_rng(seed)
    P = np.pad(rng.integers(0, 256, (H, W)).astype(np.int64), 1, mode="edge")
    L = (sum(P[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) // 9).astype(np.uint8)
    R = np.roll(L, -shift, axis=1)
    R = np.clip(R.astype(int) + rng.integers(-6, 7, R.shape), 0, 255).astype(np.uint8)
    R[H // 3:H // 2] = rng.integers(0, 256, (H // 2 - H // 3, W))  # a band without a match
    return L, R


def test_sgbm_then_filter_is_sgbm_with_filter(gpu, mvsv):
    """compute with speckleWindowSize = 0, then the filter through its own entry point with
    StereoSGBM's arguments, equals compute with the filter on."""
    L, R = noisy_pair(11, 256, 128, 9)
    kw = dict(minDisparity=1, numDisparities=64, blockSize=5, P1=200, P2=800, disp12MaxDiff=1,
              uniquenessRatio=10, speckleRange=2)
    window = 60
    raw = mvsv.StereoSGBM.create(speckleWindowSize=0, **kw).compute(L, R)
    want = mvsv.StereoSGBM.create(speckleWindowSize=window, **kw).compute(L, R)
    assert np.count_nonzero(want != raw) > 50, "the pair gives the filter nothing to remove"
    got = mvsv.filter_speckles(gpu.from_numpy(raw).cuda(), (kw["minDisparity"] - 1) * 16, window,
                               16 * kw["speckleRange"]).cpu().numpy()
    assert np.array_equal(got, want), report(got, want)


def test_bm_then_filter_is_bm_with_filter(gpu, mvsv):
    L, R = noisy_pair(12, 256, 128, 7)
    window, rng_ = 40, 3

    def bm(w):
        m = mvsv.StereoBM.create(32, 9)
        m.setSpeckleWindowSize(w)
        m.setSpeckleRange(rng_)
        return m.compute(L, R), m.getMinDisparity()

    raw, min_d = bm(0)
    want, _ = bm(window)
    assert np.count_nonzero(want != raw) > 50, "the pair gives the filter nothing to remove"
    got = mvsv.filter_speckles(gpu.from_numpy(raw).cuda(), (min_d - 1) * 16, window, rng_).cpu().numpy()
    assert np.array_equal(got, want), report(got, want)
