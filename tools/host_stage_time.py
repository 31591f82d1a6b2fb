"""Wall time of the host-pointer path, one library against another (run on the box):
mvsv_sgbm on a 640x480 pair with the parameters of configs/sgbm.yml and
mvsv_normalize_minmax on a 1280x960 map, each the median of 20 calls after 3 warm-ups.

  python tools/host_stage_time.py --parent variants/parent.so --head mvstereovision3_amd/libmvsv.so \\
      --out profiles/hoststage/ab.json

runs parent, head, parent, head, one child process after the other (never two at
once, each under a time limit, stopping at the first that fails).  Verdict per call:
head's slower run must lie within |parent_a - parent_b| above the slower parent run;
if the two parent runs differ by more than 5 % of their mean there is no stable
number and the verdict says so.  --one: the child, timing the library MVSV_LIBRARY names."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, CALLS = 3, 20


def median_ms(fn):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(CALLS):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def one():
    import numpy as np

    import mvstereovision3_amd as mvsv
    m = mvsv.StereoSGBM.create()
    assert mvsv.Disparity.loadSGBMParameters(os.path.join(ROOT, "tests", "golden", "configs", "sgbm.yml"), m,
                                             mvsv.disparity.sgbmParameters())
    L, R = mvsv.synth_pair(0x5EED, 640, 480, m._params.min_disparity, m._params.num_disparities)
    out = np.empty((480, 640), np.int16)
    d = np.random.default_rng(5).integers(-16, 2000, (960, 1280)).astype(np.int16)
    disp = np.empty((960, 1280), np.uint8)
    res = {"sgbm_640x480_ms": median_ms(lambda: m.compute(L, R, out)),
           "normalize_1280x960_ms": median_ms(lambda: mvsv.normalize_minmax(d, out=disp))}
    print(json.dumps(res), flush=True)


def verdict(parent_a, parent_b, head_a, head_b):
    spread, slow = abs(parent_a - parent_b), max(parent_a, parent_b)
    if spread > 0.05 * (parent_a + parent_b) / 2:
        return "no stable number: the two parent runs differ by more than 5 % of their mean"
    return "parity" if max(head_a, head_b) <= slow + spread else "head is slower"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", action="store_true")
    ap.add_argument("--parent")
    ap.add_argument("--head")
    ap.add_argument("--out")
    ap.add_argument("--timeout", type=int, default=120)
    a = ap.parse_args()
    if a.one:
        return one()
    runs = []
    for side in ("parent", "head", "parent", "head"):
        env = dict(os.environ, MVSV_LIBRARY=os.path.abspath(getattr(a, side)))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"], env=env, capture_output=True,
                           text=True, timeout=a.timeout)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-4000:], file=sys.stderr)
            sys.exit(f"{side} run ended with {r.returncode}: nothing more is started")
        runs.append(dict(json.loads(r.stdout.strip().splitlines()[-1]), side=side))
        print(runs[-1], flush=True)
    res = {"warmup": WARMUP, "calls": CALLS, "order": "parent head parent head", "runs": runs, "verdict": {}}
    for key in ("sgbm_640x480_ms", "normalize_1280x960_ms"):
        res["verdict"][key] = verdict(runs[0][key], runs[2][key], runs[1][key], runs[3][key])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
