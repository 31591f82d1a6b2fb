#!/usr/bin/env python3
"""What the lattice detector costs in the config-5 stream (tools/bench_stream.py's
shape: 1280x960, create(0, 256, 9, 648, 2592), the 9x9 grid over the
createDMapROIS work ROI, depth 24, batch 8, 2 launches in flight).

Three variants on ONE stream, switched between rounds (the lattice may change
while no frame is pending), alternating a, b, c for `--rounds` rounds after a
warm-up round of each:

    a  lattice off                      (the stream as it was before the lattice)
    b  lattice on, room for every hit   (max_hits = all points)
    c  lattice on, max_hits = 256

Every round pushes `--frames` host frames and takes every frame back: the map as a
view of the pinned slot plus the 81 means, through MeanDisparityDetection's host
post-pass as bench_stream.py does, and in b / c front_samples() before the pop (the
arrays only: SamplepointDetection's per-hit Python objects are left out, they would
measure the interpreter).  Then the two kernels alone, HIP-event timed on
device-resident maps of the work ROI, for 1 and 8 frames.  One JSON line.

The lattice lies over the work ROI, where the detectors look (1152x960: 143 x 119 =
17 017 points), not over the whole 1280x960 map (159 x 119 = 18 921); the D2H bytes
reported are for that lattice.

The variants have to alternate inside one process, so the tool sets no time limit of
its own: run it under one, e.g.

    timeout -k 10 400 python tools/samplepoint_stream.py [--frames 240] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(mvsv, torch, maps, det, reps=30):
    """{frames: {kernel: us}}: median HIP-event time of each kernel launch (C ABI
    calls on torch's current stream, outputs allocated beforehand)."""
    import ctypes

    import numpy as np

    from mvstereovision3_amd import _lib
    lib, ctx = _lib.lib(), _lib.context(0)
    _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx.handle)
    q = np.ascontiguousarray(det.mQ_32F.reshape(16))
    first, second = (float(v) for v in det.mRangeDisparity)
    npts = len(det.getSamplepointVec())
    out = {}
    for n in (1, 8):
        d = maps[:n]
        H, W = d.shape[1:]
        vals = torch.empty((n, npts), dtype=torch.float32, device=d.device)
        counts = torch.zeros((n,), dtype=torch.int32, device=d.device)
        hits = torch.empty((n, npts, 16), dtype=torch.uint8, device=d.device)
        tv, td = [], []
        for _ in range(reps + 3):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            _lib.check(lib.mvsv_samplepoint_values_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                          det.RADIUS, vals.data_ptr()), ctx.handle)
            e[1].record()
            _lib.check(lib.mvsv_samplepoint_detect_device(ctx.handle, n, vals.data_ptr(), W, H, q.ctypes.data, first,
                                                          second, npts, counts.data_ptr(), hits.data_ptr()),
                       ctx.handle)
            e[2].record()
            torch.cuda.synchronize()
            tv.append(e[0].elapsed_time(e[1]) * 1e3)
            td.append(e[1].elapsed_time(e[2]) * 1e3)
        tv, td = sorted(tv[3:]), sorted(td[3:])
        out[str(n)] = {"values_us": round(tv[len(tv) // 2], 1), "detect_us": round(td[len(td) // 2], 1),
                       "hits": counts.cpu().tolist()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=2)
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
    det = mvsv.SamplepointDetection()
    det.init(shape, Q, 0.1, 1.5)
    npts = len(det.getSamplepointVec())
    uniq = [mvsv.synth_pair(0x5EED0000 + i, W, H, 0, D) for i in range(8)]
    st = mvsv.DisparityStream(m, W, H, depth=a.depth, grid_roi=roi_u, batch=a.batch, inflight=a.inflight)
    hits_seen = {"b": 0, "c": 0}

    def round_fps(variant, frames):
        if variant == "a":
            st.disable_samplepoints()
        else:
            st.enable_samplepoints(det, roi=roi_u, max_hits=None if variant == "b" else 256)

        def consume():
            if variant != "a":
                _, count, _ = st.front_samples()
                hits_seen[variant] += count
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
    hits_seen = dict.fromkeys(hits_seen, 0)
    fps = {"a": [], "b": [], "c": []}
    for _ in range(a.rounds):
        for v in "abc":
            fps[v].append(round(round_fps(v, a.frames), 2))
    st.close()

    dev = torch.device("cuda", 0)
    Lt = torch.from_numpy(np.stack([u[0] for u in uniq])).to(dev)
    Rt = torch.from_numpy(np.stack([u[1] for u in uniq])).to(dev)
    maps = m.compute(Lt, Rt)[:, roi_u[1]:roi_u[3], roi_u[0]:roi_u[2]]
    kt = kernel_times(mvsv, torch, maps, det)
    map_bytes = W * H * 2
    extra = {"b": npts * 4 + 4 + npts * 16, "c": npts * 4 + 4 + 256 * 16}
    print(json.dumps({
        "workload": f"config5_stream_{W}x{H}_d{D}_samplepoints", "frames_per_round": a.frames,
        "depth": a.depth, "batch": a.batch, "inflight": a.inflight, "points": npts,
        "fps": fps,
        "fps_a_spread": round(max(fps["a"]) - min(fps["a"]), 2),
        "mean_hits_per_frame": {k: round(v / (a.rounds * a.frames), 1) for k, v in hits_seen.items()},
        "extra_d2h_bytes_per_frame": extra,
        "extra_d2h_share_of_map": {k: round(v / map_bytes, 4) for k, v in extra.items()},
        "kernel_us": kt,
    }))


if __name__ == "__main__":
    main()
