"""The census StereoBM call beside the SAD call of the same parameters: device time per
stage.

Usage (on the GPU box): python tools/census_bm_bench.py [--root TREE] [--out FILE] [--warmup 5] [--calls 20]
                                                          [--variants sad]

For every shape, on one run, the variants alternate call by call:

* ``sad``        compute() as shipped (prefilter + bm_match2_kernel);
* ``census97``   compute_census(window (9, 7)): two-word descriptors;
* ``census55``   compute_census(window (5, 5)): one-word descriptors.

``--root TREE`` loads the package and library of another checkout of this repository (the
parent commit's build: the baseline of the condition that the SAD kernels did not move); a
tree without the census entry points measures ``sad`` only; ``--variants sad`` makes this
tree's process run the same sequence of calls as the parent's.  Every call is measured by the
library's stage timers (mvsv_profile_enable / mvsv_profile_read: HIP event pairs around
each stage; the census transform is timed as the prefilter stage, whose place it takes; a
SAD call's prefilter kernels carry no timer, so its prefilter stage reads 0 and "ms" is its
match and post stages); figures are medians over the timed calls, "spread" is
(max - min) / median; "wall_ms" is the host time of the call up to the synchronize, which
holds every kernel of either variant.  One JSON document."""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = {"census97": (9, 7), "census55": (5, 5)}
# (name, numDisparities, blockSize, from bm.yml, width, height, frames)
SHAPES = [(f"{cfg} {W}x{H} x{n}", D, bs, yml, W, H, n)
          for cfg, D, bs, yml in (("bm.yml", 80, 21, True), ("StereoBM(64, 9)", 64, 9, False))
          for W, H in ((640, 480), (1280, 960)) for n in (1, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--variants", default=None, help="comma-separated subset, e.g. 'sad' for the A/B against a parent tree")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import mvstereovision3_amd as mvsv
    from mvstereovision3_amd import _lib
    assert os.path.dirname(os.path.abspath(mvsv.__file__)).startswith(root)
    ctx = _lib.Context(0)
    _lib.check(_lib.lib().mvsv_set_stream(ctx.handle, torch.cuda.current_stream().cuda_stream), ctx.handle)
    has_census = hasattr(mvsv.StereoBM, "compute_census")
    variants = ["sad"] + (list(WINDOWS) if has_census else [])
    if a.variants:
        variants = [v for v in variants if v in a.variants.split(",")]

    rows = []
    for name, D, bs, yml, W, H, n in SHAPES:
        m = mvsv.StereoBM.create(D, bs)
        if yml:
            assert mvsv.Disparity.loadBMParameters(os.path.join(root, "tests", "golden", "configs", "bm.yml"), m)
        p = m.params()
        host = [mvsv.synth_pair(0x5EED0000 + i, W, H, p["min_disparity"], p["num_disparities"]) for i in range(n)]
        L = torch.from_numpy(np.stack([h[0] for h in host])).cuda()
        R = torch.from_numpy(np.stack([h[1] for h in host])).cuda()
        out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        calls = {v: [] for v in variants}
        wall = {v: [] for v in variants}
        for i in range(a.warmup + a.calls):
            for v in variants:
                with _lib.use_context(ctx):
                    _lib.profile_reset(ctx)
                    _lib.profile_enable(ctx, True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if v == "sad":
                        m.compute(L, R, out)
                    else:
                        m.compute_census(L, R, out, window=WINDOWS[v])
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    _lib.profile_enable(ctx, False)
                    if i >= a.warmup:
                        calls[v].append({k: t[0] for k, t in _lib.profile_read(ctx).items() if t[1]})
                        wall[v].append((t1 - t0) * 1e3)
        row = {"shape": name, "variants": {}}
        for v in variants:
            tot = sorted(sum(c.values()) for c in calls[v])
            med = statistics.median(tot)
            stages = sorted({k for c in calls[v] for k in c})
            ws = sorted(wall[v])
            row["variants"][v] = {
                "ms": round(med, 4), "min": round(tot[0], 4), "max": round(tot[-1], 4),
                "spread": round((tot[-1] - tot[0]) / med, 4),
                "wall_ms": round(statistics.median(ws), 4), "wall_min": round(ws[0], 4), "wall_max": round(ws[-1], 4),
                "stages": {k: round(statistics.median(c.get(k, 0.0) for c in calls[v]), 4) for k in stages},
                "stage_min": {k: round(min(c.get(k, 0.0) for c in calls[v]), 4) for k in stages},
                "stage_max": {k: round(max(c.get(k, 0.0) for c in calls[v]), 4) for k in stages}}
        rows.append(row)
        print(name, {k: (v["ms"], v["wall_ms"], v["stages"]) for k, v in row["variants"].items()}, file=sys.stderr,
              flush=True)
    doc = {"tree": os.path.relpath(root, HERE), "census": has_census, "windows": {k: list(w) for k, w in WINDOWS.items()},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "calls": a.calls, "rows": rows}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
