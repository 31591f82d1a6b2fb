#!/usr/bin/env python3
"""What the point cloud costs.  One JSON line per run.

    --part kernels   HIP-event time of the three launches of mvsv_point_cloud_device for
                     1 and 8 maps of 1280x960 (config 4's output: sgbm.yml, MODE_HH), on
                     the whole map and on an odd view, with the bytes they move: two
                     reads of the int16 map and 16 bytes per valid pixel.
    --part dmap2pcl  Utility::dmap2pcl of one such map from the host, the file going to
                     a memory-backed directory; the same points written by ply.write
                     alone (the part both trees share: text formatting), so that the
                     difference is the call "up to the point of writing the file"; the
                     D2H bytes of the call; and, where the tree has it, mvsv_point_cloud
                     alone (host map in, host records out).
    --part stream    the config-5 stream of tools/bench_stream.py (1280x960, create(0,
                     256, 9, 648, 2592), the 9x9 grid over the work ROI, depth 24,
                     batch 8, 2 launches in flight) in three states on ONE stream,
                     alternating for --rounds rounds after a warm-up round of each:
                         a  cloud never enabled / disabled
                         b  cloud over the work ROI, (count, min, max) read per frame
                         c  the same with front_cloud copying every frame's records
                     A tree without the cloud runs state a only; --variants a does the
                     same on this tree (the cloud is never enabled).

--tree DIR imports the package from another checkout (the parent commit built side by
side), so that the two can be run in turns by a script; the tool sets no time limit of
its own: run it under one, e.g.

    timeout -k 10 300 python tools/cloud_stream.py --part stream [--tree DIR]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3), "n": len(v)}


def config4_maps(mvsv, torch, n=8):
    import numpy as np
    W, H = 1280, 960
    m = mvsv.StereoSGBM.create(0, 0, 0, 0, 0)
    assert mvsv.Disparity.loadSGBMParameters(os.path.join(ROOT, "tests", "golden", "configs", "sgbm.yml"), m,
                                             mvsv.sgbmParameters())
    m.setMode(mvsv.MODE_HH)
    pairs = [mvsv.synth_pair(0x5EED0000 + i, W, H, 1, 128) for i in range(n)]
    L = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    R = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return m.compute(L, R)


def q_matrix(np):
    return np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "q_matrix.json")))["Q"], np.float32)


def part_kernels(mvsv, np, torch, reps):
    from mvstereovision3_amd import _lib
    lib, ctx = _lib.lib(), _lib.context(0)
    _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx.handle)
    maps = config4_maps(mvsv, torch)
    q = q_matrix(np)
    out = {}
    for name, view in {"whole_map": maps, "odd_view_x129_w1143": maps[:, 1:959, 129:129 + 1143]}.items():
        out[name] = {}
        for n in (1, 8):
            d = view[:n]
            H, W = d.shape[1:]
            rec = torch.empty((n, H * W, 4), dtype=torch.float32, device=d.device)
            cnt = torch.empty((n,), dtype=torch.int32, device=d.device)
            t = []
            for _ in range(reps + 3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _lib.check(lib.mvsv_point_cloud_device(ctx.handle, n, d.data_ptr(), d.stride(1), d.stride(0), W, H,
                                                       q.ctypes.data, rec.data_ptr(), H * W, cnt.data_ptr(), None),
                           ctx.handle)
                e1.record()
                torch.cuda.synchronize()
                t.append(e0.elapsed_time(e1) * 1e3)
            t = t[3:]
            valid = int(cnt.sum())
            moved = 2 * 2 * n * H * W + 16 * valid
            us = statistics.median(t)
            out[name][str(n)] = {"us": spread(t), "valid_share": round(valid / (n * H * W), 4),
                                 "MB_moved": round(moved / 1e6, 2), "GBps": round(moved / us / 1e3, 1)}
    return {"part": "kernels", "kernel_us": out}


def part_dmap2pcl(mvsv, np, torch, reps):
    from mvstereovision3_amd import _lib
    d = config4_maps(mvsv, torch, 1)[0].cpu().numpy()
    q = q_matrix(np)
    valid = int((d > 0).sum())
    tmp = tempfile.mkdtemp(dir="/dev/shm" if os.path.isdir("/dev/shm") else None)
    path = os.path.join(tmp, "pointcloud.ply")
    total, write, cloud = [], [], []
    pts = None
    for _ in range(reps + 2):
        t0 = time.perf_counter()
        mvsv.Utility.dmap2pcl(path, d, q)
        total.append((time.perf_counter() - t0) * 1e3)
        if pts is None:
            lines = open(path).read().split("end_header\n")[1].splitlines()
            pts = np.array([[float(v) for v in ln.split()[:3]] for ln in lines], np.float32)
            assert len(pts) == valid
        w = mvsv.ply("Hagen Hiller", "disparity pointcloud", d)
        t0 = time.perf_counter()
        w.write(path, pts, mvsv.ply.WITH_COLOR)
        write.append((time.perf_counter() - t0) * 1e3)
        if hasattr(mvsv, "point_cloud"):
            t0 = time.perf_counter()
            rec = mvsv.point_cloud(d, q)
            cloud.append((time.perf_counter() - t0) * 1e3)
            assert len(rec) == valid
    os.remove(path)
    os.rmdir(tmp)
    total, write, cloud = total[2:], write[2:], cloud[2:]
    has = hasattr(_lib.lib(), "mvsv_point_cloud")
    res = {"part": "dmap2pcl", "width": d.shape[1], "height": d.shape[0], "valid_pixels": valid,
           "dmap2pcl_ms": spread(total), "ply_write_alone_ms": spread(write),
           "up_to_the_write_ms": round(statistics.median(total) - statistics.median(write), 3),
           "d2h_bytes": 12 + 16 * valid if has else 16 * d.size}
    if cloud:
        res["point_cloud_host_ms"] = spread(cloud)
    return res


def part_stream(mvsv, np, torch, a):
    from mvstereovision3_amd import _lib
    W, H, D = 1280, 960, 256
    m = mvsv.StereoSGBM.create(0, D, 9, 8 * 81, 32 * 81)
    Q = q_matrix(np).reshape(4, 4).copy()
    Q[0, 3] *= 2  # as bench_stream.py: the calibration file is for 752x480
    Q[1, 3] *= 2
    Q[2, 3] *= 2
    roi_u, _ = mvsv.create_dmap_rois((H, W), D)
    shape = (roi_u[3] - roi_u[1], roi_u[2] - roi_u[0])
    grid = mvsv.MeanDisparityDetection()
    grid.init(shape, Q, 0.1, 1.5)
    uniq = [mvsv.synth_pair(0x5EED0000 + i, W, H, 0, D) for i in range(8)]
    st = mvsv.DisparityStream(m, W, H, depth=a.depth, batch=a.batch, grid_roi=roi_u, inflight=a.inflight)
    has = hasattr(st, "enable_cloud")
    variants = a.variants if has else "a"
    current = ["a"]
    seen = {"b": 0, "c": 0}
    count = ctypes.c_int(0)

    def round_fps(variant, frames):
        if variant != current[0]:
            if variant == "a":
                st.disable_cloud()
            elif current[0] == "a":  # b and c share the buffers
                st.enable_cloud(Q, roi=roi_u)
            current[0] = variant

        def consume():
            if variant == "b":
                _lib.check(_lib.lib().mvsv_stream_front_cloud(st._h, None, 0, ctypes.byref(count), None),
                           st._ctx.handle)
                seen["b"] += count.value
            elif variant == "c":
                rec, n = st.front_cloud()
                seen["c"] += len(rec)
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

    for v in variants:
        round_fps(v, a.depth)
    seen = {"b": 0, "c": 0}
    fps = {v: [] for v in variants}
    for _ in range(a.rounds):
        for v in variants:
            fps[v].append(round(round_fps(v, a.frames), 2))
    st.close()
    res = {"part": "stream", "workload": f"config5_stream_{W}x{H}_d{D}_cloud", "frames_per_round": a.frames,
           "depth": a.depth, "batch": a.batch, "inflight": a.inflight, "work_roi": list(roi_u),
           "variants": variants, "fps": fps,
           "fps_median": {v: round(statistics.median(f), 2) for v, f in fps.items()},
           "fps_a_spread": round(max(fps["a"]) - min(fps["a"]), 2)}
    if "c" in variants:
        per = a.frames * a.rounds
        res["valid_points_per_frame"] = round(seen["b"] / per)
        res["records_copied_per_frame"] = round(seen["c"] / per)
        res["extra_d2h_bytes_per_frame"] = {"b": 12, "c": 12 + 16 * round(seen["c"] / per)}
        res["map_d2h_bytes_per_frame"] = W * H * 2
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "dmap2pcl", "stream"], required=True)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--inflight", type=int, default=2)
    ap.add_argument("--variants", default="abc",
                    help="the states a stream round runs in; 'a' alone never enables the cloud (no switch, no "
                         "buffer is ever allocated or freed between rounds), as on a tree without it")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import numpy as np
    import torch

    import mvstereovision3_amd as mvsv
    assert os.path.abspath(mvsv.__file__).startswith(os.path.abspath(a.tree) + os.sep)
    if a.part == "kernels":
        res = part_kernels(mvsv, np, torch, a.reps)
    elif a.part == "dmap2pcl":
        res = part_dmap2pcl(mvsv, np, torch, a.reps)
    else:
        res = part_stream(mvsv, np, torch, a)
    res["tree"] = os.path.relpath(os.path.abspath(a.tree), ROOT)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
