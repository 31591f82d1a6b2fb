"""The device ends of the frame stream: push / push_raw / push_bgr from
torch device tensors (mvsv_stream_push*_device: one copy kernel launch per contiguous
piece of the ring, ordered against the producer's stream by events), the maps and
products handed out on the device (pop(copy_map="device"), front_map, front_display,
front_view, front_rectified), the host outputs switch and the fence.

Sizes 96 x 64 and 101 x 67: the odd width makes rows that are not dword-aligned, so
the copy kernel's dword path (96 wide, contiguous), its byte path (101 wide, and every
view entered 1 .. 3 bytes in or with an odd row stride) and, for colour rows padded to
4 bytes, the dword path's byte tail all occur.  Expected maps are the oracle's, checked
once against the one-shot compute; never another stream's."""
import functools
import json
import os

import numpy as np
import pytest

from tests import prepare_restate as ref
from tests.conftest import GOLDEN

pytestmark = pytest.mark.gpu

Q_REF = np.array(json.load(open(os.path.join(GOLDEN, "q_matrix.json")))["Q"], np.float32)
SIZES = [(96, 64), (101, 67)]
KINDS = ["sgbm", "bm"]
RANGE = (1e4, 16.0)  # (first, second): found where 16 < value < 1e4
size_ids = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731


def matcher(mvsv, kind):
    if kind == "bm":
        return mvsv.StereoBM.create(32, 9)
    return mvsv.StereoSGBM.create(0, 32, 5, 200, 800, 1, 31, 10, 50, 2, mvsv.MODE_SGBM)


def oracle_map(kind, L, R):
    """The oracle alone; at least a quarter of the map must be valid."""
    from oracle import pyoracle
    import mvstereovision3_amd as mvsv
    m = matcher(mvsv, kind)
    L, R = np.ascontiguousarray(L), np.ascontiguousarray(R)
    if kind == "bm":
        w = pyoracle.bm(L, R, m.params())
    else:
        w = pyoracle.sgbm(L, R, {k: v for k, v in m.params().items() if k != "variant"})
    assert (w > 0).mean() >= 0.25, "the expected map is mostly invalid: it would show nothing"
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def pair(size, seed):
    import mvstereovision3_amd as mvsv
    L, R = mvsv.synth_pair(0xB0000 + seed, size[0], size[1], 0, 32)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def want(size, kind, seed):
    """The oracle's map, checked once against the one-shot compute."""
    import mvstereovision3_amd as mvsv
    w = oracle_map(kind, *pair(size, seed))
    one = matcher(mvsv, kind).compute(*pair(size, seed))
    assert np.array_equal(one, w), f"the one-shot compute differs from the oracle ({size}, {kind}, seed {seed})"
    return w


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def dev_pair(torch, size, seed):
    return tuple(dev(torch, a) for a in pair(size, seed))


def dev_batch(torch, size, seeds):
    """(N, H, W) left and right tensors of the seeds' frames."""
    return tuple(dev(torch, np.stack([pair(size, s)[k] for s in seeds])) for k in (0, 1))


def assert_map(got, w, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    bad = np.argwhere(got != w)
    assert got.shape == w.shape and bad.size == 0, f"{what}: {len(bad)} mismatches, first {bad[:5].tolist()}"


# ---- 1. the same results as host pushes, every product enabled ----

@pytest.mark.parametrize("inflight", [1, 2])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_maps_and_products_from_device_frames(gpu, mvsv, size, kind, inflight):
    W, H = size
    whole = (0, 0, W, H)
    layers = mvsv.VIEW_SUBIMAGE_GRID | mvsv.VIEW_OBSTACLE_GRID | mvsv.VIEW_FOUND_TILES | mvsv.VIEW_FOUND_POINTS
    st = mvsv.DisparityStream(matcher(mvsv, kind), W, H, depth=5, grid_roi=whole, batch=3, inflight=inflight)
    st.enable_samplepoints((Q_REF, *RANGE), roi=whole)
    st.enable_display()
    st.enable_view(layers, roi=whole, mean_detector_or_range=RANGE)
    st.enable_cloud(Q_REF)
    st.enable_sharpness()
    got = []

    def pop():
        vals, count, hits = st.front_samples()
        disp, dmm = st.front_display()
        img, vmm = st.front_view()
        rec, ccount, cmm = st.front_cloud(return_minmax=True)
        sharp = st.front_sharpness(return_sums=True)
        d, means = st.pop()
        got.append((d, means, vals, count, hits, disp, dmm, img, vmm, rec, ccount, cmm, sharp))

    frames = [dev_pair(gpu, size, seed) for seed in range(11)]
    for L, R in frames:  # runs of 3 and 2 end at the ring's end: two wraps in 11 frames
        if st.pending() == 5:
            pop()
        st.push(L, R)
    while st.pending():
        pop()
    st.close()
    assert len(got) == 11
    for seed, (d, means, vals, count, hits, disp, dmm, img, vmm, rec, ccount, cmm, sharp) in enumerate(got):
        w = want(size, kind, seed)
        assert_map(d, w, f"frame {seed}")
        t = dev(gpu, w)
        assert np.array_equal(means, mvsv.mean_disparity_grid(t).cpu().numpy()), f"frame {seed}: means"
        ov = mvsv.samplepoint_values(t, 2)
        assert np.array_equal(vals, ov.cpu().numpy()), f"frame {seed}: lattice values"
        oc, oh = mvsv.samplepoint_detect(ov, (H, W), Q_REF, RANGE)
        assert count == int(oc) == len(hits), f"frame {seed}: hit count"
        assert hits.tobytes() == oh.cpu().numpy()[:count].tobytes(), f"frame {seed}: hit records"
        od, omm = mvsv.normalize_minmax(t, return_minmax=True)
        assert np.array_equal(disp, od.cpu().numpy()) and dmm == tuple(int(v) for v in omm.cpu()), f"frame {seed}: display"
        oi, oimm = mvsv.detection_view(t, layers, means=means, mean_range=RANGE, values=vals, sample_range=RANGE,
                                       return_minmax=True)
        assert np.array_equal(img, oi.cpu().numpy()) and vmm == tuple(int(v) for v in oimm.cpu()), f"frame {seed}: view"
        orec, omm2 = mvsv.point_cloud(np.array(w), Q_REF, return_minmax=True)
        assert ccount == len(orec) == int((w > 0).sum()) and cmm == (int(omm2[0]), int(omm2[1])), f"frame {seed}: cloud"
        assert rec.tobytes() == orec.tobytes(), f"frame {seed}: cloud records"
        ws = [mvsv.sharpness(g, return_sums=True) for g in pair(size, seed)]
        assert sharp == ((ws[0][0], ws[1][0]), (ws[0][1], ws[1][1])), f"frame {seed}: sharpness"
    assert not np.array_equal(want(size, kind, 0), want(size, kind, 1))  # an order mix-up would show


# ---- 2. views ----

def carve(torch, frames, offset, fill=0xA5):
    """`frames` (N, H, row bytes...) copied into a view of a larger byte buffer: entered
    `offset` bytes in, odd row stride, frame stride no multiple of 4.  Returns (buffer, view)."""
    n, h = frames.shape[:2]
    row = int(np.prod(frames.shape[2:]))
    rs = row + 6 + (row + 1) % 2      # odd
    fs = h * rs + 5
    fs += 1 if fs % 4 == 0 else 0     # no multiple of 4
    assert rs % 2 == 1 and fs % 4 != 0
    buf = torch.full((offset + n * fs + 16,), fill, dtype=torch.uint8, device="cuda")
    inner = (3, 1) if frames.ndim == 4 else (1,)
    view = buf.as_strided(tuple(frames.shape), (fs, rs) + inner, offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    return buf, view


@pytest.mark.parametrize("offset", [1, 2, 3])
@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_views_of_a_larger_tensor(gpu, mvsv, size, offset):
    W, H = size
    seeds = [0, 1, 2]
    bufs = [carve(gpu, np.stack([pair(size, s)[k] for s in seeds]), offset) for k in (0, 1)]
    before = [b.clone() for b, _ in bufs]
    st = mvsv.DisparityStream(matcher(mvsv, "bm"), W, H, depth=4, batch=2)
    st.push(bufs[0][1], bufs[1][1])                  # three frames at once ...
    st.push(bufs[0][1][1], bufs[1][1][1])            # ... and one frame of the view alone
    for i, seed in enumerate(seeds + [1]):
        assert_map(st.pop()[0], want(size, "bm", seed), f"frame {i} (seed {seed}) from a view {offset} bytes in")
    st.close()
    gpu.cuda.synchronize()
    for (b, _), was in zip(bufs, before):
        assert gpu.equal(b, was), "the enclosing tensor changed"


# ---- 3. batched push ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_batched_push_over_the_rings_end(gpu, mvsv, size, kind):
    W, H = size
    maps = {}
    for how in ("batch", "single"):
        st = mvsv.DisparityStream(matcher(mvsv, kind), W, H, depth=5, batch=3)
        for seed in range(3):
            st.push(*dev_pair(gpu, size, seed))
        for seed in range(3):
            assert_map(st.pop()[0], want(size, kind, seed), f"{how}: frame {seed}")
        if how == "batch":                            # slots 3, 4, 0, 1
            st.push(*dev_batch(gpu, size, range(3, 7)))
        else:
            for seed in range(3, 7):
                st.push(*dev_pair(gpu, size, seed))
        assert st.pending() == 4
        with pytest.raises(mvsv.MvsvError) as e:      # free slots + 1
            st.push(*dev_batch(gpu, size, [7, 8]))
        assert e.value.code == -1 and st.pending() == 4
        st.push(*dev_batch(gpu, size, [7]))           # the free slot, as a batch of one
        maps[how] = [st.pop()[0] for _ in range(5)]
        assert st.pending() == 0
        st.close()
    for i, seed in enumerate(range(3, 8)):
        assert_map(maps["batch"][i], want(size, kind, seed), f"batched frame {seed}")
        assert_map(maps["single"][i], want(size, kind, seed), f"single frame {seed}")


# ---- 4. ordering against the producer's stream, both directions ----

@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_producer_work_is_waited_for(gpu, mvsv, size):
    """Milliseconds of matmuls, then the copy of the real frame into the source, then the
    push, all on a side stream and without a synchronise: a push that did not wait for
    the producer would read the zeros."""
    torch = gpu
    W, H = size
    real = dev_pair(torch, size, 4)
    a = torch.randn(4096, 4096, device="cuda")
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)  # the BLAS library is loaded before the clock matters
    src = [torch.zeros((H, W), dtype=torch.uint8, device="cuda") for _ in range(2)]
    st = mvsv.DisparityStream(matcher(mvsv, "bm"), W, H, depth=2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(12):
            torch.mm(a, a, out=c)
        src[0].copy_(real[0], non_blocking=True)
        src[1].copy_(real[1], non_blocking=True)
        st.push(src[0], src[1])
    assert_map(st.pop()[0], want(size, "bm", 4), "the frame written by the producer's stream")
    st.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_source_may_be_reused_after_push(gpu, mvsv, size):
    """The source of an (N, H, W) batch is zeroed on the producer's stream right after its
    push.  An earlier push from a second stream that is busy with matmuls holds the
    stream's upload queue back for milliseconds, so the batch's copy is still waiting when
    the idle producer's zeroing is enqueued: if that stream did not wait for the copy, the
    copy would read zeros."""
    torch = gpu
    W, H = size
    seeds = [5, 6, 7]
    first = dev_pair(torch, size, 4)
    L, R = dev_batch(torch, size, seeds)
    a = torch.randn(4096, 4096, device="cuda")
    c = torch.empty_like(a)
    torch.mm(a, a, out=c)
    st = mvsv.DisparityStream(matcher(mvsv, "bm"), W, H, depth=4, batch=4)
    st.push(*dev_batch(torch, size, [0, 1, 2, 3]))  # a first launch allocates, which waits for the device
    for seed in range(4):
        assert_map(st.pop()[0], want(size, "bm", seed), f"warm-up frame {seed}")
    torch.cuda.synchronize()
    busy, side = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(busy):
        for _ in range(12):
            torch.mm(a, a, out=c)
        st.push(*first)
    with torch.cuda.stream(side):
        st.push(L, R)
        L.zero_()
        R.zero_()
    for seed in [4] + seeds:
        assert_map(st.pop()[0], want(size, "bm", seed), f"frame {seed}, source zeroed after the push")
    st.close()
    torch.cuda.synchronize()
    assert int(L.max()) == 0 and int(R.max()) == 0


# ---- 5. outputs ----

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_device_outputs_and_host_outputs_switch(gpu, mvsv, size, kind):
    torch = gpu
    W, H = size
    whole = (0, 0, W, H)
    st = mvsv.DisparityStream(matcher(mvsv, kind), W, H, depth=3, grid_roi=whole)
    st.enable_display()
    st.enable_view(mvsv.VIEW_SUBIMAGE_GRID | mvsv.VIEW_FOUND_TILES, roi=whole, mean_detector_or_range=RANGE)
    w = want(size, kind, 9)
    wmeans = mvsv.mean_disparity_grid(dev(torch, w)).cpu().numpy()

    def device_getters(what):
        m, means = st.front_map(device=True)
        disp, dmm = st.front_display(copy="device")
        img, vmm = st.front_view(copy="device")
        assert m.is_cuda and m.dtype == torch.int16 and disp.dtype == torch.uint8 and img.shape == (H, W, 3)
        assert_map(m, w, f"{what}: front_map")
        assert np.array_equal(means, wmeans), f"{what}: means"
        return disp.cpu().numpy(), dmm, img.cpu().numpy(), vmm

    # every host output on: the device getters equal their host counterparts
    st.push(*dev_pair(torch, size, 9))
    st.push(*pair(size, 9))
    ddisp, ddmm, dimg, dvmm = device_getters("host outputs on")
    hdisp, hdmm = st.front_display()
    himg, hvmm = st.front_view()
    assert np.array_equal(ddisp, hdisp) and ddmm == hdmm and np.array_equal(dimg, himg) and dvmm == hvmm
    od, omm = mvsv.normalize_minmax(dev(torch, w), return_minmax=True)
    assert np.array_equal(hdisp, od.cpu().numpy()) and hdmm == tuple(int(v) for v in omm.cpu())
    dmap, dmeans = st.pop(copy_map="device")
    hmap, hmeans = st.pop()
    assert dmap.is_cuda and dmap.dtype == torch.int16 and tuple(dmap.shape) == (H, W)
    assert_map(dmap, hmap, "pop(copy_map='device') vs the host pop")
    assert_map(hmap, w, "host pop")
    assert np.array_equal(dmeans, hmeans) and np.array_equal(hmeans, wmeans)
    # the host outputs off
    st.host_outputs(map=False, display=False, view=False)
    st.push(*dev_pair(torch, size, 9))
    for getter in (st.pop, lambda: st.pop(copy_map="view"), st.front_display, lambda: st.front_display(copy="view"),
                   st.front_view, lambda: st.front_view(copy="view")):
        with pytest.raises(mvsv.MvsvError) as e:
            getter()
        assert e.value.code == -1 and st.pending() == 1
    with pytest.raises(mvsv.MvsvError):
        st.host_outputs()  # a frame is pending
    disp2, dmm2, img2, vmm2 = device_getters("host outputs off")
    assert np.array_equal(disp2, hdisp) and dmm2 == hdmm and np.array_equal(img2, himg) and vmm2 == hvmm
    none, means = st.pop(copy_map=False)
    assert none is None and np.array_equal(means, wmeans) and st.pending() == 0
    st.push(*dev_pair(torch, size, 9))
    assert_map(st.pop(copy_map="device")[0], w, "pop(copy_map='device') with the host map off")
    # and on again
    st.host_outputs()
    st.push(*dev_pair(torch, size, 9))
    assert_map(st.pop()[0], w, "host pop after host_outputs()")
    st.close()


def test_slot_reuse_waits_for_the_device_pop(gpu, mvsv):
    """depth 1: the slot of a frame popped to the device is pushed again at once, and
    zero-copy readers fence before they let go of a frame."""
    size = SIZES[1]
    st = mvsv.DisparityStream(matcher(mvsv, "bm"), *size, depth=1)
    st.host_outputs(map=False)
    maps = []
    for seed in range(4):
        st.push(*dev_pair(gpu, size, seed))
        if seed % 2:
            maps.append(st.pop(copy_map="device")[0])
        else:
            maps.append(st.front_map()[0].clone())
            st.fence()
            st.pop(copy_map=False)
    for seed, m in enumerate(maps):
        assert_map(m, want(size, "bm", seed), f"frame {seed}")
    st.close()


# ---- 6. raw and colour ----

RAW_W, RAW_H = 109, 73
RAW_ROI = (4, 3, 105, 70)  # 101 x 67


@functools.lru_cache(maxsize=None)
def raw_maps():
    """A small rectification with fractional maps (1/64 px, so ties of the 1/32 rounding
    occur): the left and the right map differ by half a pixel."""
    y, x = np.mgrid[0:RAW_H, 0:RAW_W].astype(np.float64)

    def q(m):
        return (np.round(m * 64) / 64).astype(np.float32)
    lx = q(x + 0.25 + 0.01 * (y - 30))
    ly = q(y + 1.5 * np.sin(x / 23) - 0.5)
    rx = q(x + 0.765625 + 0.01 * (y - 30))
    return lx, ly, rx, ly.copy()


@functools.lru_cache(maxsize=None)
def raw_pair(seed):
    import mvstereovision3_amd as mvsv
    L, R = mvsv.synth_pair(0xB1000 + seed, RAW_W, RAW_H, 0, 32)
    L.setflags(write=False)
    R.setflags(write=False)
    return L, R


@functools.lru_cache(maxsize=None)
def want_raw(seed, kind):
    from oracle import pyoracle
    maps = raw_maps()
    x0, y0, x1, y1 = RAW_ROI
    L, R = raw_pair(seed)
    rl = np.ascontiguousarray(pyoracle.remap_linear(L, maps[0], maps[1])[y0:y1, x0:x1])
    rr = np.ascontiguousarray(pyoracle.remap_linear(R, maps[2], maps[3])[y0:y1, x0:x1])
    return rl, rr, oracle_map(kind, rl, rr)


@pytest.mark.parametrize("kind", KINDS)
def test_raw_frames_from_the_device(gpu, mvsv, kind):
    torch = gpu
    streams = {how: mvsv.DisparityStream.raw(matcher(mvsv, kind), raw_maps(), roi=RAW_ROI, depth=4, batch=3,
                                             keep_rectified=True) for how in ("device", "host")}
    assert (streams["device"].width, streams["device"].height) == SIZES[1]
    seeds = [0, 1, 2, 3]
    d = streams["device"]
    L, R = (dev(torch, np.stack([raw_pair(s)[k] for s in seeds[:2]])) for k in (0, 1))
    d.push_raw(L, R)                                 # a batch of two ...
    d.push_raw(*raw_pair(2))                         # ... a host frame in the same launch of three ...
    d.push_raw(*(dev(torch, a) for a in raw_pair(3)))  # ... and one device frame in the ring's last slot
    for s in seeds:
        streams["host"].push_raw(*raw_pair(s))
    with pytest.raises(mvsv.MvsvError):
        d.push(*dev_pair(torch, SIZES[1], 0))        # a raw stream takes raw frames
    for s in seeds:
        rl, rr, w = want_raw(s, kind)
        fl, fr = d.front_rectified()
        fl, fr = fl.cpu().numpy(), fr.cpu().numpy()
        got, _, (gl, gr) = d.pop(rectified=True)
        hgot, _, (hl, hr) = streams["host"].pop(rectified=True)
        assert_map(got, w, f"raw frame {s} vs the oracle")
        assert_map(got, hgot, f"raw frame {s} vs the stream fed from the host")
        for a, b, what in ((gl, rl, "left"), (gr, rr, "right"), (fl, rl, "front left"), (fr, rr, "front right"),
                           (hl, rl, "host left"), (hr, rr, "host right")):
            assert np.array_equal(a, b), f"raw frame {s}: rectified {what}"
    with pytest.raises(mvsv.MvsvError):
        streams["host"].front_rectified()            # empty
    for st in streams.values():
        st.close()
    plain = mvsv.DisparityStream(matcher(mvsv, kind), *SIZES[1])
    with pytest.raises(mvsv.MvsvError):
        plain.push_raw(*(dev(torch, a) for a in raw_pair(0)))
    plain.push(*pair(SIZES[1], 0))
    with pytest.raises(mvsv.MvsvError):
        plain.front_rectified()                      # not a keep_rectified stream
    assert plain.pending() == 1
    plain.close()


BGR_CASES = [((192, 128), True), ((202, 134), True), ((101, 67), False)]  # (source size, halve)


@functools.lru_cache(maxsize=None)
def bgr_pair(src, seed):
    """A synthetic stereo pair with a little colour: each channel is the grey image plus
    its own {-3 .. 3} noise."""
    import mvstereovision3_amd as mvsv
    w, h = src
    rng = np.random.default_rng(seed)
    out = []
    for g in mvsv.synth_pair(0xC0100 + seed, w, h, 0, 64 if w > 150 else 32):
        c = np.clip(g[..., None].astype(np.int64) + rng.integers(-3, 4, (h, w, 3)), 0, 255).astype(np.uint8)
        c.setflags(write=False)
        out.append(c)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def want_bgr(src, halve, seed, kind):
    L, R = (ref.prepare(c, halve, ref.Q14) for c in bgr_pair(src, seed))
    return L, R, oracle_map(kind, L, R)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", BGR_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{'halved' if c[1] else 'as-is'}")
def test_colour_frames_from_the_device(gpu, mvsv, case, kind):
    torch = gpu
    src, halve = case
    W, H = mvsv.prepare_size(*src) if halve else src
    assert (W, H) in SIZES
    sw, sh = src
    streams = {how: mvsv.DisparityStream(matcher(mvsv, kind), W, H, depth=5, batch=3) for how in ("device", "host")}
    for st in streams.values():
        st.enable_bgr((sh, sw), halve=halve)
    d = streams["device"]
    order = []
    # two contiguous frames (dword path where 3 * width allows)
    L, R = (dev(torch, np.stack([bgr_pair(src, s)[k] for s in (0, 1)])) for k in (0, 1))
    d.push_bgr(L, R)
    order += [("bgr", 0), ("bgr", 1)]
    # a host colour frame in the same launch of three
    d.push_bgr(*bgr_pair(src, 2))
    order.append(("bgr", 2))
    # a view entered 3 bytes in, odd row stride (byte path) ...
    views = [carve(torch, np.stack([bgr_pair(src, 3)[k]]), 3) for k in (0, 1)]
    before = [b.clone() for b, _ in views]
    d.push_bgr(views[0][1][0], views[1][1][0])
    order.append(("bgr", 3))
    # ... and rows padded to a multiple of 4 bytes (dword path with a byte tail where 3 * width % 4 != 0)
    pad = [torch.full((1, sh, sw + (4 - sw % 4), 3), 9, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
    for p, c in zip(pad, bgr_pair(src, 4)):
        p[0, :, :sw] = dev(torch, c)
    assert pad[0].stride(1) % 4 == 0
    d.push_bgr(pad[0][0, :, :sw], pad[1][0, :, :sw])
    order.append(("bgr", 4))
    for how, s in order:
        streams["host"].push_bgr(*bgr_pair(src, s))
    for i, (how, s) in enumerate(order):
        got, hgot = d.pop()[0], streams["host"].pop()[0]
        assert_map(got, want_bgr(src, halve, s, kind)[2], f"colour frame {i} vs the oracle on the restated pair")
        assert_map(got, hgot, f"colour frame {i} vs the stream fed from the host")
    # a grey device frame and a colour device frame in one launch
    gl, gr, gw = want_bgr(src, halve, 5, kind)
    d.set_batch(2)
    d.push(dev(torch, gl), dev(torch, gr))
    d.push_bgr(*(dev(torch, c) for c in bgr_pair(src, 6)))
    assert_map(d.pop()[0], gw, "grey device frame beside a colour one")
    assert_map(d.pop()[0], want_bgr(src, halve, 6, kind)[2], "colour device frame beside a grey one")
    torch.cuda.synchronize()
    for (b, _), was in zip(views, before):
        assert torch.equal(b, was), "the enclosing tensor changed"
    d.disable_bgr()
    with pytest.raises(mvsv.MvsvError):
        d.push_bgr(*(dev(torch, c) for c in bgr_pair(src, 6)))
    assert d.pending() == 0
    for st in streams.values():
        st.close()


@pytest.mark.parametrize("size", SIZES, ids=size_ids)
def test_host_and_device_pushes_in_one_launch(gpu, mvsv, size):
    st = mvsv.DisparityStream(matcher(mvsv, "sgbm"), *size, depth=4, batch=4)
    st.push(*pair(size, 0))
    st.push(*dev_pair(gpu, size, 1))
    st.push(*pair(size, 2))
    st.push(*dev_pair(gpu, size, 3))
    for seed in range(4):
        assert_map(st.pop()[0], want(size, "sgbm", seed), f"frame {seed}")
    st.close()


# ---- 7. refusals ----

def test_refusals(gpu, mvsv):
    torch = gpu
    size = SIZES[0]
    W, H = size
    st = mvsv.DisparityStream(matcher(mvsv, "bm"), W, H, depth=2)
    L, R = dev_pair(torch, size, 0)
    refused = {
        "dtype": (L.to(torch.int8), R.to(torch.int8)),
        "float": (L.float(), R.float()),
        "size": (L[:, :-1], R[:, :-1]),
        "rows": (L[:-1], R[:-1]),
        "unequal": (L, R[None]),
        "rank": (L[None, None], R[None, None]),
        "empty batch": (L[None][:0], R[None][:0]),
        "device with numpy": (L, pair(size, 0)[1]),
        "numpy with device": (pair(size, 0)[0], R),
        "device with a CPU tensor": (L, R.cpu()),
    }
    for what, (a, b) in refused.items():
        with pytest.raises(mvsv.MvsvError) as e:
            st.push(a, b)
        assert e.value.code == -1 and st.pending() == 0, what
    with pytest.raises(mvsv.MvsvError):
        st.pop(copy_map="device")  # empty
    with pytest.raises(mvsv.MvsvError):
        st.front_map()
    # CPU tensors take the host path
    st.push(L.cpu(), R.cpu())
    st.push(L, R)
    for i in range(2):
        assert_map(st.pop()[0], want(size, "bm", 0), f"after the refusals, frame {i}")
    st.close()


@pytest.mark.skipif("__import__('torch').cuda.device_count() < 2", reason="a wrong device index needs two devices")
def test_refused_device_index(gpu, mvsv):
    size = SIZES[0]
    st = mvsv.DisparityStream(matcher(mvsv, "bm"), *size, depth=2)
    L, R = (t.to("cuda:1") for t in dev_pair(gpu, size, 0))
    with pytest.raises(mvsv.MvsvError) as e:
        st.push(L, R)
    assert e.value.code == -1 and st.pending() == 0
    st.close()
