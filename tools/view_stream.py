#!/usr/bin/env python3
"""What the detection view costs.

1. The launches alone, HIP-event timed on device-resident maps of config 5's shape
   (1280x960, create(0, 256, 9, 648, 2592)), for 1 and 8 frames, on the aligned whole
   map, on the work-ROI view and on an odd view (x0 = 129, 1143 wide: 7 head pixels
   per row, rows that start at odd output bytes): the view with all four layers
   (minmax_kernel + view_kernel: 2 + 2 + 3 = 7 bytes per pixel) and the display map
   (minmax_kernel + normalize_u8_kernel: 5 bytes per pixel) in turns inside one loop,
   so that both see the same machine (and the view without any layer, for what the
   layers themselves cost).  The median of `--reps` launches after warm-up.

2. The config-5 stream (tools/bench_stream.py's shape: the 9x9 grid over the
   createDMapROIS work ROI, depth 24, batch 8, 2 launches in flight), variants
   switched between rounds on ONE stream, alternating for `--rounds` rounds after a
   warm-up round of each:

       a  nothing enabled
       b  display on over the work ROI           (1 byte per pixel more to download)
       c  view on over the work ROI: grids + found tiles                (3 bytes)
       d  sample points on + view with all four layers                  (3 bytes)
       e  sample points on, no view              (what d pays for the lattice alone)

   Every round pushes `--frames` host frames and takes every frame back as
   tools/display_stream.py does, with front_display / front_view(copy="view") before
   the pop.  One JSON line.

No time limit of its own: run it as `timeout -k 10 400 python tools/view_stream.py`.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(torch, mvsv, views, reps):
    from mvstereovision3_amd import _lib
    from mvstereovision3_amd.utility import view_spec
    lib, ctx = _lib.lib(), _lib.context(0)
    _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx.handle)
    out = {}
    for name, maps in views.items():
        out[name] = {}
        for n in (1, 8):
            d = maps[:n]
            H, W = d.shape[1:]
            _, _, nx, ny = mvsv.samplepoint_layout(W, H)
            means = mvsv.mean_disparity_grid(d).reshape(n, 81).contiguous()
            values = mvsv.samplepoint_values(d, 2).reshape(n, nx * ny).contiguous()
            # ranges that find about half of the tiles and of the points
            spec = view_spec(15, (float(means.median()) + 0.5, -1.0), (float(values.median()) + 0.5, -1.0))
            spec.means, spec.values = means.data_ptr(), values.data_ptr()
            base = view_spec(0)  # no layer: the display bytes as BGR
            o1 = torch.empty((n, H, W), dtype=torch.uint8, device=d.device)
            o3 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=d.device)
            mm = torch.empty((n, 2), dtype=torch.int16, device=d.device)
            tv, tn, tb = [], [], []
            for _ in range(reps + 5):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
                e[0].record()
                _lib.check(lib.mvsv_view_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                ctypes.byref(spec), o3.data_ptr(), 3 * W, 3 * H * W, mm.data_ptr()),
                           ctx.handle)
                e[1].record()
                _lib.check(lib.mvsv_normalize_minmax_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                            0.0, 255.0, o1.data_ptr(), W, H * W, mm.data_ptr()),
                           ctx.handle)
                e[2].record()
                _lib.check(lib.mvsv_view_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                ctypes.byref(base), o3.data_ptr(), 3 * W, 3 * H * W, mm.data_ptr()),
                           ctx.handle)
                e[3].record()
                torch.cuda.synchronize()
                tv.append(e[0].elapsed_time(e[1]) * 1e3)
                tn.append(e[1].elapsed_time(e[2]) * 1e3)
                tb.append(e[2].elapsed_time(e[3]) * 1e3)
            tv, tn, tb = sorted(tv[5:]), sorted(tn[5:]), sorted(tb[5:])
            uv, un = tv[len(tv) // 2], tn[len(tn) // 2]
            px = n * H * W
            _lib.check(lib.mvsv_view_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                            ctypes.byref(spec), o3.data_ptr(), 3 * W, 3 * H * W, mm.data_ptr()),
                       ctx.handle)
            red = int((o3.reshape(-1, 3) == torch.tensor([0, 0, 255], dtype=torch.uint8, device=d.device)).all(1).sum())
            out[name][str(n)] = {"view_us": round(uv, 1), "view_min_us": round(tv[0], 1), "view_max_us": round(tv[-1], 1),
                                 "view_GBps": round(7 * px / uv / 1e3, 1),
                                 "normalize_us": round(un, 1), "normalize_min_us": round(tn[0], 1),
                                 "normalize_max_us": round(tn[-1], 1), "normalize_GBps": round(5 * px / un / 1e3, 1),
                                 "view_no_layer_us": round(tb[len(tb) // 2], 1),
                                 "ratio": round(uv / un, 3), "MB_moved_view": round(7 * px / 1e6, 2),
                                 "red_pixel_share": round(red / px, 4), "launches": reps}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--order", default="abcde")
    a = ap.parse_args()
    import numpy as np
    import torch

    import mvstereovision3_amd as mvsv

    W, H, D = 1280, 960, 256
    m = mvsv.StereoSGBM.create(0, D, 9, 8 * 81, 32 * 81)
    q = json.load(open(os.path.join(ROOT, "tests", "golden", "q_matrix.json")))["Q"]
    Q = np.array(q, np.float32).reshape(4, 4)
    Q[0, 3] *= 2  # as bench_stream.py: the calibration file is for 752x480
    Q[1, 3] *= 2
    Q[2, 3] *= 2
    roi_u, _ = mvsv.create_dmap_rois((H, W), D)
    shape = (roi_u[3] - roi_u[1], roi_u[2] - roi_u[0])
    grid = mvsv.MeanDisparityDetection()
    grid.init(shape, Q, 0.1, 1.5)
    lattice = mvsv.SamplepointDetection()
    lattice.init(shape, Q, 0.1, 1.5)
    uniq = [mvsv.synth_pair(0x5EED0000 + i, W, H, 0, D) for i in range(8)]
    st = mvsv.DisparityStream(m, W, H, depth=a.depth, grid_roi=roi_u, batch=a.batch, inflight=a.inflight)
    checksum = {v: 0 for v in "bcd"}
    tiles = mvsv.VIEW_SUBIMAGE_GRID | mvsv.VIEW_OBSTACLE_GRID | mvsv.VIEW_FOUND_TILES
    current = [None]

    def switch(variant):
        if variant == current[0]:
            return
        st.disable_view()
        st.disable_display()
        st.disable_samplepoints()
        if variant == "b":
            st.enable_display(roi=roi_u)
        if variant in "de":
            st.enable_samplepoints(lattice, roi=roi_u)
        if variant == "c":
            st.enable_view(tiles, roi=roi_u, mean_detector_or_range=grid)
        if variant == "d":
            st.enable_view(tiles | mvsv.VIEW_FOUND_POINTS, roi=roi_u, mean_detector_or_range=grid)
        current[0] = variant

    def round_fps(variant, frames):
        switch(variant)

        def consume():
            if variant == "b":
                img, mm = st.front_display(copy="view")
            elif variant in "cd":
                img, mm = st.front_view(copy="view")
            if variant in "bcd":
                checksum[variant] += int(img[::97, ::89].sum()) + mm[1]  # the image is there and is read
                del img
            d, means = st.pop(copy_map="view")
            grid.build(d, 0, grid.MEAN_VALUE, means=means)
            grid.detectObstacles(write_pcl=False)

        t0 = time.perf_counter()
        for i in range(frames):
            if st.pending() == a.depth:
                consume()
            st.push(*uniq[i % 8])
        while st.pending():
            consume()
        return frames / (time.perf_counter() - t0)

    for v in "abcde":  # warm-up: allocations, first launches
        round_fps(v, a.depth)
    fps = {v: [] for v in "abcde"}
    for _ in range(a.rounds):
        for v in a.order:
            fps[v].append(round(round_fps(v, a.frames), 2))
    st.close()

    dev = torch.device("cuda", 0)
    Lt = torch.from_numpy(np.stack([u[0] for u in uniq])).to(dev)
    Rt = torch.from_numpy(np.stack([u[1] for u in uniq])).to(dev)
    maps = m.compute(Lt, Rt)
    work = maps[:, roi_u[1]:roi_u[3], roi_u[0]:roi_u[2]]
    odd = maps[:, 1:H - 1, 129:129 + 1143]
    kt = kernel_times(torch, mvsv, {"whole_map": maps, "work_roi_view": work, "odd_view_x129_w1143": odd}, a.reps)
    map_bytes = W * H * 2
    px = shape[0] * shape[1]
    extra = {"b": px + 4, "c": 3 * px + 4, "d": 3 * px + 4}
    med = {v: sorted(f)[len(f) // 2] for v, f in fps.items() if f}
    print(json.dumps({
        "workload": f"config5_stream_{W}x{H}_d{D}_view", "frames_per_round": a.frames,
        "depth": a.depth, "batch": a.batch, "inflight": a.inflight, "order": a.order, "work_roi": list(roi_u),
        "fps": fps, "fps_median": med,
        "fps_a_spread": round(max(fps["a"]) - min(fps["a"]), 2) if fps["a"] else None,
        "extra_d2h_bytes_per_frame": extra,
        "extra_d2h_share_of_map": {k: round(v / map_bytes, 4) for k, v in extra.items()},
        "kernel_us": kt,
    }))


if __name__ == "__main__":
    main()
