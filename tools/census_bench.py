"""The census call beside the Birchfield-Tomasi call of the same parameters: device time
per stage.

Usage (on the GPU box): python tools/census_bench.py [--root TREE] [--out FILE] [--warmup 5] [--calls 20]

For every shape, on one run, three variants alternate call by call:

* ``bt``      compute() as shipped (register-ring cost kernel, residual / bit planes);
* ``bt_lds``  compute() on a context created with MVSV_KERNELS=cost-lds: the register-ring
              cost kernel off, so the BT launch takes the LDS-ring cost kernel -- the kernel
              whose census form a census call runs, hence the baseline of its cost stage;
* ``census``  compute_census(window (9, 7)).

``--root TREE`` loads the package and library of another checkout of this repository (the
parent commit's build: the baseline of the cost-stage condition); a tree without the census
entry points measures ``bt`` and ``bt_lds`` only.  Every call is measured by the library's
stage timers (mvsv_profile_enable / mvsv_profile_read: HIP event pairs around each stage;
the census transform is timed as the prefilter stage, whose place it takes); figures are
medians over the timed calls, "spread" is (max - min) / median.  One JSON document."""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER = ("path_strips", "path_lines")  # sub-stages of path_aggregation
WINDOW = (9, 7)
# (name, width, height, frames, mode)
SHAPES = [
    ("sgbm.yml MODE_SGBM 640x480 x1", 640, 480, 1, 0),
    ("sgbm.yml MODE_SGBM 1280x960 x1", 1280, 960, 1, 0),
    ("sgbm.yml MODE_HH 1280x960 x1", 1280, 960, 1, 1),
    ("sgbm.yml MODE_SGBM 1280x960 x8", 1280, 960, 8, 0),
    ("sgbm.yml MODE_HH 1280x960 x8", 1280, 960, 8, 1),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import numpy as np
    import torch
    import mvstereovision3_amd as mvsv
    from mvstereovision3_amd import _lib
    assert os.path.dirname(os.path.abspath(mvsv.__file__)).startswith(root)
    stream = torch.cuda.current_stream().cuda_stream

    def new_context(kernels=None):
        if kernels:
            os.environ["MVSV_KERNELS"] = kernels
        try:
            c = _lib.Context(0)
        finally:
            os.environ.pop("MVSV_KERNELS", None)
        _lib.check(_lib.lib().mvsv_set_stream(c.handle, stream), c.handle)
        return c

    contexts = {"bt": new_context(), "bt_lds": new_context("cost-lds")}
    has_census = hasattr(mvsv.StereoSGBM, "compute_census")
    if has_census:
        # on bt's context: two contexts (four streams with their second streams) in either
        # tree, so both fit the hardware queues the same way
        contexts["census"] = contexts["bt"]

    rows = []
    for name, W, H, n, mode in SHAPES:
        m = mvsv.StereoSGBM.create(0, 0, 0, 0, 0)
        assert mvsv.Disparity.loadSGBMParameters(os.path.join(root, "tests", "golden", "configs", "sgbm.yml"), m,
                                                 mvsv.sgbmParameters())
        m.setMode(mode)
        p = m.params()
        host = [mvsv.synth_pair(0x5EED0000 + i, W, H, p["min_disparity"], p["num_disparities"]) for i in range(n)]
        L = torch.from_numpy(np.stack([h[0] for h in host])).cuda()
        R = torch.from_numpy(np.stack([h[1] for h in host])).cuda()
        out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        calls = {v: [] for v in contexts}
        plans = {}
        for i in range(a.warmup + a.calls):
            for v, ctx in contexts.items():
                with _lib.use_context(ctx):
                    plans[v] = _lib.sgbm_plan(ctx, n, W, H, m._params, **({"census": WINDOW} if v == "census" else {}))
                    _lib.profile_reset(ctx)
                    _lib.profile_enable(ctx, True)
                    if v == "census":
                        m.compute_census(L, R, out, window=WINDOW)
                    else:
                        m.compute(L, R, out)
                    torch.cuda.synchronize()
                    _lib.profile_enable(ctx, False)
                    if i >= a.warmup:
                        calls[v].append({k: t[0] for k, t in _lib.profile_read(ctx).items() if t[1]})
        row = {"shape": name, "variants": {}}
        for v in contexts:
            tot = sorted(sum(t for k, t in c.items() if k not in INNER) for c in calls[v])
            med = statistics.median(tot)
            stages = sorted({k for c in calls[v] for k in c})
            row["variants"][v] = {
                "ms": round(med, 4), "min": round(tot[0], 4), "max": round(tot[-1], 4),
                "spread": round((tot[-1] - tot[0]) / med, 4), "plan_bits": plans[v],
                "stages": {k: round(statistics.median(c.get(k, 0.0) for c in calls[v]), 4) for k in stages},
                "stage_min": {k: round(min(c.get(k, 0.0) for c in calls[v]), 4) for k in stages},
                "stage_max": {k: round(max(c.get(k, 0.0) for c in calls[v]), 4) for k in stages}}
        rows.append(row)
        print(name, {k: (v["ms"], v["stages"]) for k, v in row["variants"].items()}, file=sys.stderr, flush=True)
    doc = {"tree": os.path.relpath(root, HERE), "census": has_census, "window": list(WINDOW),
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "calls": a.calls, "rows": rows}
    text = json.dumps(doc, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
