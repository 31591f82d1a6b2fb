#!/usr/bin/env python3
"""What the focus measure costs: the sum kernel alone, and in the config-5 stream
(tools/bench_stream.py's shape: 1280x960, create(0, 256, 9, 648, 2592), the 9x9 grid
over the createDMapROIS work ROI, depth 24, batch 8, 2 launches in flight).

Kernel: mvsv_sharpness_device (sharpness_kernel + sharpness_fold_kernel) on 1 and 8
device-resident 1280x960 frames, HIP-event timed, against its byte model n * W * H
(one read of every pixel; the two halo rows of a 16-row band are not counted); for
orientation, mvsv_minmax_device (minmax_kernel + minmax_final_kernel, 2 bytes per
pixel) on int16 maps of the same size in the same process.  Also a work-ROI view
(x0 = 129: a lane's columns straddle the ROI's left edge) of the same frames.

Stream: two variants on ONE stream, switched between rounds (the measure may change
while no frame is pending), alternating for `--rounds` rounds after a warm-up round
of each:

    a  sharpness never enabled / off      (the stream as it was before)
    b  sharpness on, whole frame on both sides; front_sharpness before every pop

`--stream-only a` runs only variant a and never touches the new calls (so the same
measurement can be made with tools/bench_stream.py on a tree without them).  One
JSON line.  Run it under a time limit, e.g.

    timeout -k 10 400 python tools/setup_stream.py [--frames 240] [--rounds 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_us(torch, launch, reps=30):
    t = []
    for _ in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b) * 1e3)
    t = sorted(t[3:])
    return t[len(t) // 2]


def kernel_times(torch, frames, maps):
    from mvstereovision3_amd import _lib
    lib, ctx = _lib.lib(), _lib.context(0)
    _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx.handle)
    out = {}
    H, W = frames.shape[1:]
    views = {"whole": None, "roi_x129": _lib.Rect(129, 1, 129 + 1143, H - 1)}
    for n in (1, 8):
        f, d = frames[:n], maps[:n]
        sums = torch.empty((n,), dtype=torch.int64, device=f.device)
        mm = torch.empty((n, 2), dtype=torch.int16, device=f.device)
        row = {}
        for name, r in views.items():
            px = n * (W * H if r is None else (r.x1 - r.x0) * (r.y1 - r.y0))
            us = median_us(torch, lambda: _lib.check(lib.mvsv_sharpness_device(
                ctx.handle, n, f.data_ptr(), f.stride(1), f.stride(0), W, H,
                ctypes.byref(r) if r is not None else None, sums.data_ptr()), ctx.handle))
            row[f"sharpness_{name}_us"] = round(us, 1)
            row[f"sharpness_{name}_GBps"] = round(px / us / 1e3, 1)
        us = median_us(torch, lambda: _lib.check(lib.mvsv_minmax_device(
            ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H, 1, mm.data_ptr()), ctx.handle))
        row["minmax_us"] = round(us, 1)
        row["minmax_GBps"] = round(2 * n * W * H / us / 1e3, 1)
        row["MB_read_sharpness_whole"] = round(n * W * H / 1e6, 2)
        out[str(n)] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--order", default="ab")
    ap.add_argument("--stream-only", default=None, help="only this variant's stream rounds (no kernel timing)")
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
    grid = mvsv.MeanDisparityDetection()
    grid.init((roi_u[3] - roi_u[1], roi_u[2] - roi_u[0]), Q, 0.1, 1.5)
    uniq = [mvsv.synth_pair(0x5EED0000 + i, W, H, 0, D) for i in range(8)]
    st = mvsv.DisparityStream(m, W, H, depth=a.depth, grid_roi=roi_u, batch=a.batch, inflight=a.inflight)
    checksum = [0.0]
    current = ["a"]

    def round_fps(variant, frames):
        if variant != current[0]:
            if variant == "a":
                st.disable_sharpness()
            else:
                st.enable_sharpness()
            current[0] = variant

        def consume():
            if variant == "b":
                checksum[0] += sum(st.front_sharpness())
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

    order = a.stream_only or a.order
    for v in sorted(set(order)):  # warm-up: allocations, first launches
        round_fps(v, a.depth)
    fps = {v: [] for v in sorted(set(order))}
    for _ in range(a.rounds):
        for v in order:
            fps[v].append(round(round_fps(v, a.frames), 2))
    st.close()
    res = {"workload": f"config5_stream_{W}x{H}_d{D}_sharpness", "frames_per_round": a.frames, "depth": a.depth,
           "batch": a.batch, "inflight": a.inflight, "order": order, "fps": fps,
           "extra_d2h_bytes_per_frame": 16}
    if a.stream_only is None:
        dev = torch.device("cuda", 0)
        Lt = torch.from_numpy(np.stack([u[0] for u in uniq])).to(dev)
        Rt = torch.from_numpy(np.stack([u[1] for u in uniq])).to(dev)
        res["kernel_us"] = kernel_times(torch, Lt, m.compute(Lt, Rt))
        res["sharpness_of_frame_0"] = mvsv.sharpness(Lt[0])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
