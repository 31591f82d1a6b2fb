#!/usr/bin/env python3
"""A/B of the camera loop from the raw pair (trgt/liveDisparity.cpp:82-101), in one process:

  A  Stereosystem.getRectifiedImagepair (mvsv_rectify_pair: raw pair and the four
     float maps up, two full-frame remaps, two crops down, a synchronise) and
     then DisparityStream.push / pop of the rectified pair;
  B  DisparityStream.raw: push_raw / pop, rectification on the device.

liveDisparity's matcher create(0, 64, 9, 8*81, 32*81) on synthetic raw pairs and
smooth synthetic maps (sub-pixel shear + a vertical wave; the display ROI is the
frame less a 16-px border).  After a warm-up of both routes and a check that
their first maps agree, A and B alternate `--repeats` times with `--frames`
frames each; wall clock around loops that end in the last pop.

    python tools/raw_stream_ab.py [--batch 1 --inflight 1 --depth 3] [--frames 300] [--repeats 3]
    python tools/raw_stream_ab.py --only b --frames 64 ...    # one route, e.g. under rocprofv3
    python tools/raw_stream_ab.py --only remap --frames 64    # mvsv.remap of the same frames (kernel trace)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def inputs(mvsv, W, H, n=8):
    import numpy as np
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    wave = 2 * np.sin(x / 23) - 1
    maps = tuple(np.ascontiguousarray(m, np.float32) for m in
                 (x + 1.25 + 0.01 * (y - H / 2), y + wave, x + 4.75 + 0.01 * (y - H / 2), y + wave))
    roi = (16, 16, W - 16, H - 16)
    pairs = [mvsv.synth_pair(0x5EED0000 + 900 + i, W, H, 0, 64) for i in range(n)]
    return maps, roi, pairs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--depth", type=int, default=3)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--inflight", type=int, default=1)
    ap.add_argument("--only", choices=["a", "b", "remap"], help="run one route once, untimed comparison off")
    ap.add_argument("--out", help="also write the JSON result to this file")
    a = ap.parse_args()

    import numpy as np
    import torch
    import mvstereovision3_amd as mvsv
    from bench import kernel_source_sha
    from mvstereovision3_amd import calibration

    assert torch.cuda.is_available(), "needs a GPU: no time is taken without one"
    W, H = a.width, a.height
    maps, roi, pairs = inputs(mvsv, W, H)
    cw, ch = roi[2] - roi[0], roi[3] - roi[1]
    m = mvsv.StereoSGBM.create(0, 64, 9, 8 * 81, 32 * 81)  # trgt/liveDisparity.cpp:61

    if a.only == "remap":  # the launches rectify_pair_kernel replaces: 2 per frame
        dev = torch.device("cuda", 0)
        dm = [torch.from_numpy(x).to(dev) for x in maps]
        raw = [(torch.from_numpy(L).to(dev), torch.from_numpy(R).to(dev)) for L, R in pairs]
        for i in range(a.frames):
            L, R = raw[i % len(raw)]
            mvsv.remap(L, dm[0], dm[1])
            mvsv.remap(R, dm[2], dm[3])
        torch.cuda.synchronize()
        print(json.dumps({"route": "remap", "frames": a.frames, "remap_launches": 2 * a.frames}))
        return

    # route A's Stereosystem: the rectification state set directly (no calibration
    # files exist for this synthetic camera)
    ss = calibration.Stereosystem(W, H)
    ss.mMap1, ss.mMap2 = [maps[0], maps[2]], [maps[1], maps[3]]
    ss.mDisplayROI, ss.mIsInit = roi, True

    def open_a():
        return mvsv.DisparityStream(m, cw, ch, depth=a.depth, batch=a.batch, inflight=a.inflight)

    def open_b():
        return mvsv.DisparityStream.raw(m, ss, depth=a.depth, batch=a.batch, inflight=a.inflight)

    def push_a(st, pair):
        sip = mvsv.Stereopair(pair[0], pair[1])
        ss.getRectifiedImagepair(sip)
        st.push(sip.mLeft, sip.mRight)

    def push_b(st, pair):
        st.push_raw(pair[0], pair[1])

    def loop(st, push, frames, keep=None):
        t0 = time.perf_counter()
        for i in range(frames):
            if st.pending() == a.depth:
                d = st.pop(copy_map="view")[0]
                if keep is not None:
                    keep.append(d.copy())
            push(st, pairs[i % len(pairs)])
        while st.pending():
            d = st.pop(copy_map="view")[0]
            if keep is not None:
                keep.append(d.copy())
        return time.perf_counter() - t0

    routes = {"a": (open_a, push_a), "b": (open_b, push_b)}
    if a.only:
        st = routes[a.only][0]()
        loop(st, routes[a.only][1], a.frames)
        st.close()
        print(json.dumps({"route": a.only, "frames": a.frames, "batch": a.batch, "inflight": a.inflight}))
        return

    sa, sb = open_a(), open_b()
    # warm-up of every shape, and the two routes' first maps against each other
    first = max(len(pairs), 2 * a.depth)
    ka, kb = [], []
    loop(sa, push_a, first, ka)
    loop(sb, push_b, first, kb)
    assert len(ka) == len(kb) == first
    for i, (x, y) in enumerate(zip(ka, kb)):
        assert np.array_equal(x, y), f"frame {i}: routes A and B disagree at {np.argwhere(x != y)[:5].tolist()}"
    assert (ka[0] > 0).mean() > 0.5, "the maps are mostly invalid"
    wall = {"a": [], "b": []}
    for _ in range(a.repeats):
        wall["a"].append(loop(sa, push_a, a.frames))
        wall["b"].append(loop(sb, push_b, a.frames))
    sa.close()
    sb.close()
    fps = {k: [a.frames / t for t in v] for k, v in wall.items()}
    med = {k: float(np.median(v)) for k, v in fps.items()}
    res = {
        "workload": f"raw_stream_ab_{W}x{H}_roi{cw}x{ch}_d64_bs9",
        "kernel_source_sha": kernel_source_sha(),
        "frames": a.frames, "repeats": a.repeats, "depth": a.depth, "batch": a.batch, "inflight": a.inflight,
        "maps_agree_on_first_frames": first,
        "a_rectify_pair_then_push_fps": [round(v, 2) for v in fps["a"]],
        "b_push_raw_fps": [round(v, 2) for v in fps["b"]],
        "a_fps_median": round(med["a"], 2), "b_fps_median": round(med["b"], 2),
        "a_spread_pct": round(100 * (max(fps["a"]) - min(fps["a"])) / med["a"], 2),
        "b_spread_pct": round(100 * (max(fps["b"]) - min(fps["b"])) / med["b"], 2),
        "b_over_a": round(med["b"] / med["a"], 3),
        "note": "host raw pair in, int16 map out (PCIe included); wall clock around loops ending in the last pop",
    }
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
