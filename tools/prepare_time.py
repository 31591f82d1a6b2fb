#!/usr/bin/env python3
"""Time bgr_gray_kernel (mvsv_prepare_gray_device) on the GPU: a batch of colour
frames, HIP events around each call after warm-up, the median, and GB/s against
the byte model 3 * w * h + dw * dh per frame and against the HBM peak.  Run it under
rocprofv3 --kernel-trace --stats for the kernel's own time.

    python tools/prepare_time.py [--frames 8] [--width 1280] [--height 960] [--reps 200]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X, HBM3E


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--burst", type=int, default=32, help="launches between two events for the sustained figure")
    a = ap.parse_args()
    import ctypes
    import torch
    import mvstereovision3_amd as mvsv
    from mvstereovision3_amd import _lib
    lib = _lib.lib()
    n, w, h = a.frames, a.width, a.height
    bgr = torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, device="cuda")
    rows = []
    for halve in (True, False):
        for what, src in (("packed", bgr), ("narrow", bgr[:, :, 1:])):  # the view starts 3 bytes in
            sw = src.shape[2]
            vdw, vdh = mvsv.prepare_size(sw, h, halve)
            vmodel = n * (3 * sw * h + vdw * vdh)
            out = torch.empty((n, vdh, vdw), dtype=torch.uint8, device="cuda")
            ctx = _lib.context(0)
            _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       ctx.handle)
            args = (ctx.handle, n, src.data_ptr(), src.stride(1), src.stride(0), sw, h, 1 if halve else 0, 0,
                    out.data_ptr(), vdw, vdw * vdh)

            def call(k):  # k launches between two events, nothing else on the host in between
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(k):
                    lib.mvsv_prepare_gray_device(*args)
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / k

            for _ in range(20):
                _lib.check(lib.mvsv_prepare_gray_device(*args), ctx.handle)
            torch.cuda.synchronize()
            ms = [call(1) for _ in range(a.reps)]
            burst = statistics.median(call(a.burst) for _ in range(max(a.reps // 10, 5)))
            med = statistics.median(ms)
            gbs = vmodel / med / 1e6
            rows.append({"halve": halve, "loads": what, "frames": n, "width": sw, "height": h,
                         "median_us": round(med * 1e3, 2), "min_us": round(min(ms) * 1e3, 2),
                         "burst_us_per_call": round(burst * 1e3, 2),
                         "burst_gb_s": round(vmodel / burst / 1e6, 1),
                         "model_bytes": vmodel, "gb_s": round(gbs, 1),
                         "share_of_hbm_peak": round(gbs / HBM_PEAK_GBS, 4),
                         "model_floor_us": round(vmodel / HBM_PEAK_GBS / 1e3, 2)})
    print(json.dumps({"kernel": "bgr_gray_kernel", "timing": "HIP events around one mvsv_prepare_gray_device call (median_us, min_us: "
                      "launch latency included) and around --burst calls back to back (burst_us_per_call), "
                      "after 20 warm-up calls", "rows": rows}))


if __name__ == "__main__":
    main()
