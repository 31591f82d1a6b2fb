"""MODE_HH4 beside MODE_SGBM and MODE_HH of the same build: device time per stage.

Usage (on the GPU box): python tools/hh4_bench.py [--out FILE] [--warmup 5] [--calls 20]

For every shape of DESIGN.md §4p, on one context and in one run, the variants of a
shape alternate call by call (MODE_SGBM, MODE_HH, MODE_HH4, and for P2 > 15 also
MODE_HH4 under MVSV_OPT_PATH_SCHEDULE 1 and 2: what the plane-byte threshold of the
plan's rule stands on).  Every call is measured by the library's own stage timers
(mvsv_profile_enable / mvsv_profile_read: HIP event pairs around each stage); a
call's time is the sum of its stages (path_strips and path_lines lie inside
path_aggregation and are not added again), and the figures are medians over the
timed calls after the warm-up calls.  "spread" is (max - min) / median.  The maps of the
MODE_HH4 variants of a shape are compared with each other.  One JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIVE = (0, 64, 9, 648, 2592)
INNER = ("path_strips", "path_lines")  # sub-stages of path_aggregation
# (name, width, height, frames, create(...) arguments or "sgbm.yml", also the forced schedules)
SHAPES = [
    ("sgbm.yml 640x480 x1", 640, 480, 1, "sgbm.yml", False),
    ("sgbm.yml 1280x960 x1", 1280, 960, 1, "sgbm.yml", False),
    ("sgbm.yml 1280x960 x8", 1280, 960, 8, "sgbm.yml", False),
    ("live 1280x960 x1", 1280, 960, 1, LIVE, True),
    ("live 1280x960 x2", 1280, 960, 2, LIVE, True),
    ("live 1280x960 x3", 1280, 960, 3, LIVE, True),
    ("live 1280x960 x4", 1280, 960, 4, LIVE, True),
    ("live 1280x960 x8", 1280, 960, 8, LIVE, True),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import mvstereovision3_amd as mvsv
    from mvstereovision3_amd import _lib
    ctx = _lib.context(0)

    rows = []
    for name, W, H, n, create, forced in SHAPES:
        def make(mode):
            if create == "sgbm.yml":
                m = mvsv.StereoSGBM.create(0, 0, 0, 0, 0)
                assert mvsv.Disparity.loadSGBMParameters(
                    os.path.join(ROOT, "tests", "golden", "configs", "sgbm.yml"), m, mvsv.sgbmParameters())
            else:
                m = mvsv.StereoSGBM.create(*create)
            m.setMode(mode)
            return m
        # (label, matcher, MVSV_OPT_PATH_SCHEDULE)
        variants = [("MODE_SGBM", make(mvsv.MODE_SGBM), 0), ("MODE_HH", make(mvsv.MODE_HH), 0),
                    ("MODE_HH4", make(mvsv.MODE_HH4), 0)]
        if forced:
            variants += [("MODE_HH4 schedule 1", make(mvsv.MODE_HH4), 1), ("MODE_HH4 schedule 2", make(mvsv.MODE_HH4), 2)]
        p = variants[0][1].params()
        host = [mvsv.synth_pair(0x5EED0000 + i, W, H, p["min_disparity"], p["num_disparities"]) for i in range(n)]
        L = torch.from_numpy(np.stack([h[0] for h in host])).cuda()
        R = torch.from_numpy(np.stack([h[1] for h in host])).cuda()
        out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        calls = {label: [] for label, _, _ in variants}
        plans, maps = {}, {}
        for i in range(a.warmup + a.calls):
            for label, m, sched in variants:
                mvsv.set_option(mvsv.OPT_PATH_SCHEDULE, sched)
                plans[label] = _lib.sgbm_plan(ctx, n, W, H, m._params)
                _lib.profile_reset(ctx)
                _lib.profile_enable(ctx, True)
                m.compute(L, R, out)
                torch.cuda.synchronize()
                _lib.profile_enable(ctx, False)
                if i == 0:
                    maps[label] = out.clone()
                if i >= a.warmup:
                    calls[label].append({k: v[0] for k, v in _lib.profile_read(ctx).items() if v[1]})
        mvsv.set_option(mvsv.OPT_PATH_SCHEDULE, 0)
        # the MODE_HH4 schedules compute one map (whole batch, every int16)
        row = {"shape": name, "hh4_schedules_agree": all(torch.equal(maps["MODE_HH4"], v) for k, v in maps.items()
                                                          if k.startswith("MODE_HH4")), "variants": {}}
        for label, _, _ in variants:
            tot = sorted(sum(v for k, v in c.items() if k not in INNER) for c in calls[label])
            med = statistics.median(tot)
            row["variants"][label] = {
                "ms": round(med, 4), "min": round(tot[0], 4), "max": round(tot[-1], 4),
                "spread": round((tot[-1] - tot[0]) / med, 4), "plan_bits": plans[label],
                "stages": {k: round(statistics.median(c.get(k, 0.0) for c in calls[label]), 4)
                           for k in sorted({k for c in calls[label] for k in c})}}
        rows.append(row)
        print(name, {k: v["ms"] for k, v in row["variants"].items()}, file=sys.stderr, flush=True)
    doc = {"library": os.path.basename(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "calls": a.calls, "rows": rows}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
