"""Colour (BGR) against grey StereoSGBM launches: device time and stage split.

Usage (on the GPU box): python tools/color_bench.py [--out FILE] [--grey-only]
    [--warmup 5] [--calls 20]

For every shape of DESIGN.md §4o, on one context and in one run: mvsv_sgbm_device
on the grey pair and mvsv_sgbm_bgr_device on the colour pair whose channels are
that pair plus a little noise of their own.  Each call is timed with its own pair
of HIP events (5 warm-up calls, median of 20); the stage split comes from
mvsv_profile_read in a second pass, so that its event pairs do not sit inside the
timed calls.  "spread" is (max - min) / median over the 20 calls.  With
MVSV_LIBRARY set to another build of the library (the parent commit's) and
--grey-only, the same grey figures of that build.  One JSON document."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, width, height, frames, create(...) arguments or "sgbm.yml", mode)
SHAPES = [
    ("capture 640x480 x1 create(0,16,5,200,800)", 640, 480, 1, (0, 16, 5, 200, 800), 0),
    ("sgbm.yml MODE_HH 640x480 x8", 640, 480, 8, "sgbm.yml", 1),
    ("sgbm.yml MODE_HH 1280x960 x8", 1280, 960, 8, "sgbm.yml", 1),
    ("live 1280x960 x1 create(0,64,9,648,2592)", 1280, 960, 1, (0, 64, 9, 648, 2592), 0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--grey-only", action="store_true")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    import numpy as np
    import torch
    import mvstereovision3_amd as mvsv
    from mvstereovision3_amd import _lib
    ctx = _lib.context(0)

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.calls)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize()
        ms = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
        med = statistics.median(ms)
        _lib.profile_reset(ctx)
        _lib.profile_enable(ctx, True)
        for _ in range(a.calls):
            fn()
        torch.cuda.synchronize()
        _lib.profile_enable(ctx, False)
        prof = _lib.profile_read(ctx)
        return {"ms": round(med, 4), "min": round(ms[0], 4), "max": round(ms[-1], 4),
                "spread": round((ms[-1] - ms[0]) / med, 4),
                "stages": {k: round(v[0] / a.calls, 4) for k, v in prof.items() if v[1]}}

    rows = []
    for name, W, H, n, create, mode in SHAPES:
        if create == "sgbm.yml":
            m = mvsv.StereoSGBM.create(0, 0, 0, 0, 0)
            assert mvsv.Disparity.loadSGBMParameters(
                os.path.join(ROOT, "tests", "golden", "configs", "sgbm.yml"), m, mvsv.sgbmParameters())
        else:
            m = mvsv.StereoSGBM.create(*create)
        m.setMode(mode)
        p = m.params()
        host = [mvsv.synth_pair(0x5EED0000 + i, W, H, p["min_disparity"], p["num_disparities"]) for i in range(n)]
        Lg = np.stack([h[0] for h in host])
        Rg = np.stack([h[1] for h in host])
        L, R = torch.from_numpy(Lg).cuda(), torch.from_numpy(Rg).cuda()
        out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        row = {"shape": name, "grey": timed(lambda: m.compute(L, R, out))}
        if not a.grey_only:
            rng = np.random.default_rng(1)
            col = [np.clip(g[..., None].astype(np.int64) + rng.integers(-6, 7, g.shape + (3,)), 0, 255).astype(np.uint8)
                   for g in (Lg, Rg)]
            Lc, Rc = torch.from_numpy(col[0]).cuda(), torch.from_numpy(col[1]).cuda()
            row["colour"] = timed(lambda: m.compute_bgr(Lc, Rc, out))
            row["colour_over_grey"] = round(row["colour"]["ms"] / row["grey"]["ms"], 3)
            row["plan"] = {"grey": _lib.sgbm_plan(ctx, n, W, H, m._params),
                           "colour": _lib.sgbm_plan(ctx, n, W, H, m._params, channels=3)}
        rows.append(row)
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
