#!/usr/bin/env python3
"""What the display map costs in the config-5 stream (tools/bench_stream.py's
shape: 1280x960, create(0, 256, 9, 648, 2592), the 9x9 grid over the
createDMapROIS work ROI, depth 24, batch 8, 2 launches in flight).

Three variants on ONE stream, switched between rounds (the display may change
while no frame is pending), alternating a, b, c for `--rounds` rounds after a
warm-up round of each:

    a  display off                      (the stream as it was before)
    b  display on over the work ROI     (what the detector loops normalise)
    c  display on over the whole map    (liveDisparity)

Every round pushes `--frames` host frames and takes every frame back: the map as a
view of the pinned slot plus the 81 means, through MeanDisparityDetection's host
post-pass as bench_stream.py does, and in b / c front_display(copy="view") before
the pop.  Then the launches alone, HIP-event timed on device-resident maps, for 1
and 8 frames, on the aligned whole map, on the work-ROI view of it (x0 = 128: 16-byte
aligned rows too) and on an odd view (x0 = 129, 1143 wide: 7 head elements per row,
byte stores):
normalize = minmax_kernel + normalize_u8_kernel (5 bytes per pixel: two reads of the
int16 map, one 8-bit write), minmax = minmax_kernel + minmax_final_kernel (2 bytes
per pixel).  And, for scale, the same normalisation of one work-ROI map in numpy on
a host core.  One JSON line.

The variants have to alternate inside one process, so the tool sets no time limit of
its own: run it under one, e.g.

    timeout -k 10 400 python tools/display_stream.py [--frames 240] [--rounds 3] [--order acb]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(torch, views, reps=30):
    """{view: {frames: {...}}}: median HIP-event time of each entry point's launches
    (C ABI calls on torch's current stream, outputs allocated beforehand)."""
    import ctypes

    from mvstereovision3_amd import _lib
    lib, ctx = _lib.lib(), _lib.context(0)
    _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx.handle)
    out = {}
    for name, maps in views.items():
        out[name] = {}
        for n in (1, 8):
            d = maps[:n]
            H, W = d.shape[1:]
            o = torch.empty((n, H, W), dtype=torch.uint8, device=d.device)
            mm = torch.empty((n, 2), dtype=torch.int16, device=d.device)
            tn, tm = [], []
            for _ in range(reps + 3):
                e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
                e[0].record()
                _lib.check(lib.mvsv_normalize_minmax_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                            0.0, 255.0, o.data_ptr(), W, H * W, mm.data_ptr()),
                           ctx.handle)
                e[1].record()
                _lib.check(lib.mvsv_minmax_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H, 1,
                                                  mm.data_ptr()), ctx.handle)
                e[2].record()
                torch.cuda.synchronize()
                tn.append(e[0].elapsed_time(e[1]) * 1e3)
                tm.append(e[1].elapsed_time(e[2]) * 1e3)
            tn, tm = sorted(tn[3:]), sorted(tm[3:])
            un, um = tn[len(tn) // 2], tm[len(tm) // 2]
            px = n * H * W
            out[name][str(n)] = {"normalize_us": round(un, 1), "normalize_GBps": round(5 * px / un / 1e3, 1),
                                 "minmax_us": round(um, 1), "minmax_GBps": round(2 * px / um / 1e3, 1),
                                 "MB_moved_normalize": round(5 * px / 1e6, 2)}
    return out


def host_numpy_ms(np, work, reps=5):
    """cv::normalize's two passes in numpy on one host core, for scale (not bit-pinned)."""
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        lo, hi = int(work.min()), int(work.max())
        scale = 255.0 / (hi - lo) if hi > lo else 0.0
        out = np.clip(np.rint(work.astype(np.float32) * np.float32(scale) + np.float32(-lo * scale)), 0, 255)
        out.astype(np.uint8)
        t.append((time.perf_counter() - t0) * 1e3)
    return round(sorted(t)[len(t) // 2], 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--order", default="abc",
                    help="order of the variants inside a round; a repeated letter (aaabbbccc) repeats the variant "
                         "without switching, so its later rounds are free of the switch's frees and allocations")
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
    uniq = [mvsv.synth_pair(0x5EED0000 + i, W, H, 0, D) for i in range(8)]
    st = mvsv.DisparityStream(m, W, H, depth=a.depth, grid_roi=roi_u, batch=a.batch, inflight=a.inflight)
    checksum = {"b": 0, "c": 0}

    current = [None]

    def round_fps(variant, frames):
        if variant != current[0]:  # a repeated variant keeps its buffers: nothing is freed or allocated
            if variant == "a":
                st.disable_display()
            else:
                st.enable_display(roi=roi_u if variant == "b" else None)
            current[0] = variant

        def consume():
            if variant != "a":
                disp, mm = st.front_display(copy="view")
                checksum[variant] += int(disp[::97, ::89].sum()) + mm[1]  # the map is there and is read
                del disp
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

    for v in "abc":  # warm-up: allocations, first launches
        round_fps(v, a.depth)
    fps = {"a": [], "b": [], "c": []}
    for _ in range(a.rounds):
        for v in a.order:
            fps[v].append(round(round_fps(v, a.frames), 2))
    st.close()

    dev = torch.device("cuda", 0)
    Lt = torch.from_numpy(np.stack([u[0] for u in uniq])).to(dev)
    Rt = torch.from_numpy(np.stack([u[1] for u in uniq])).to(dev)
    maps = m.compute(Lt, Rt)
    work = maps[:, roi_u[1]:roi_u[3], roi_u[0]:roi_u[2]]
    # a view whose rows start 2 bytes past a 16-byte boundary and whose dense 8-bit
    # output has an odd stride: 7 head elements per row and single-byte stores
    odd = maps[:, 1:H - 1, 129:129 + 1143]
    kt = kernel_times(torch, {"whole_map": maps, "work_roi_view": work, "odd_view_x129_w1143": odd})
    map_bytes = W * H * 2
    extra = {"b": shape[0] * shape[1] + 4, "c": W * H + 4}
    print(json.dumps({
        "workload": f"config5_stream_{W}x{H}_d{D}_display", "frames_per_round": a.frames,
        "depth": a.depth, "batch": a.batch, "inflight": a.inflight, "order": a.order,
        "work_roi": list(roi_u), "work_roi_data_ptr_mod_16": int(work.data_ptr() % 16),
        "fps": fps,
        "fps_a_spread": round(max(fps["a"]) - min(fps["a"]), 2),
        "extra_d2h_bytes_per_frame": extra,
        "extra_d2h_share_of_map": {k: round(v / map_bytes, 4) for k, v in extra.items()},
        "kernel_us": kt,
        "host_numpy_normalize_ms_per_work_roi_map": host_numpy_ms(np, work[0].cpu().numpy()),
    }))


if __name__ == "__main__":
    main()
