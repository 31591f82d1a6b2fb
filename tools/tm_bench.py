#!/usr/bin/env python3
"""Time tm_kernel (mvsv_tm_device, Disparity::tm) on the GPU: 640 x 480 and 1280 x 960,
k = 5 (the reference's own call) and k = 9, batches of 1 and 8 frames of random bytes.
HIP events around each call after warm-up; the median, the minimum, windows per second
and an operation model against the VALU peak.

The model (counted from the kernel's loops, not measured): a window costs two column
products V (ceil(k / 4) v_dot4_u32_u8 each: 4 multiplies + 4 adds per lane-instruction),
two adds for the sliding sum and about 7 lane-instructions of float filter in phase 2;
the peak is 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz lane-instructions per second.

    python tools/tm_bench.py [--reps 30] [--out profiles/tm/tm_bench.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VALU_PEAK_LANE_INSTR = 256 * 4 * 32 * 2.4e9


def windows(w, h, k):
    """Candidate windows of one frame: (H - k) rows, W - j - k shifts for column j < W - k."""
    return (h - k) * (w - k) * (w - k + 1) // 2


def model(w, h, k):
    q = (k + 3) // 4
    per = 2 * q + 2 + 7
    return {"lane_instr_per_window": per, "int_ops_per_window": 2 * q * 8 + 2,
            "lane_instr": windows(w, h, k) * per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="640x480,1280x960")
    ap.add_argument("--ks", default="5,9")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tm", "tm_bench.json"))
    a = ap.parse_args()
    import torch
    from mvstereovision3_amd import _lib
    assert torch.cuda.is_available(), "tm_bench needs the GPU"
    lib = _lib.lib()
    ctx = _lib.context(0)
    _lib.check(lib.mvsv_set_stream(ctx.handle, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), ctx.handle)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0x5EED)
    rows = []
    for size in a.sizes.split(","):
        w, h = (int(v) for v in size.split("x"))
        for n in (int(v) for v in a.batches.split(",")):
            L = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=gen)
            R = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=gen)
            out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
            for k in (int(v) for v in a.ks.split(",")):
                args = (ctx.handle, n, L.data_ptr(), w, w * h, R.data_ptr(), w, w * h, w, h, k, out.data_ptr(), w,
                        w * h, 1)

                def call():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    _lib.check(lib.mvsv_tm_device(*args), ctx.handle)
                    e1.record()
                    e1.synchronize()
                    return e0.elapsed_time(e1)

                for _ in range(a.warmup):
                    call()
                ms = [call() for _ in range(a.reps)]
                med = statistics.median(ms)
                m = model(w, h, k)
                win = n * windows(w, h, k)
                rows.append({"width": w, "height": h, "k": k, "frames": n, "reps": a.reps,
                             "median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                             "ms_per_frame": round(med / n, 4), "windows": win,
                             "gwindows_per_s": round(win / med / 1e6, 2),
                             "model_lane_instr_per_window": m["lane_instr_per_window"],
                             "model_int_ops_per_window": m["int_ops_per_window"],
                             "model_share_of_valu_peak": round(n * m["lane_instr"] / (med * 1e-3) / VALU_PEAK_LANE_INSTR, 4),
                             "checksum": int(out.to(torch.int64).sum().item())})
                print(json.dumps(rows[-1]), flush=True)
    res = {"kernel": "tm_kernel", "device": torch.cuda.get_device_name(0),
           "timing": f"HIP events around one mvsv_tm_device call (launch latency included), {a.warmup} warm-up "
                     f"calls, median of {a.reps}; random bytes, so nearly every window is dropped by the float filter",
           "model": "share of VALU peak = modelled lane-instructions (2 * ceil(k / 4) v_dot4_u32_u8 + 2 adds + 7 "
                    "filter instructions per window) / time / (256 CUs * 4 SIMDs * 32 lanes * 2.4 GHz); a model "
                    "of the kernel's loops, not a counter reading",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"written": a.out, "rows": len(rows)}))


if __name__ == "__main__":
    main()
