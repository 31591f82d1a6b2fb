#!/usr/bin/env python3
"""Run one benchmark command on two sides in turns and record every run.

A side is a checkout (this tree, or the parent commit built side by side) plus extra
arguments, so the same tool compares two trees (--side parent:../parent --side tree:.)
or two modes of one tree (--side host:. --side "device:.:--device-frames").  Each run
is a child process of its own with a time limit; the first one that fails ends the
job.  The command's last output line must be a JSON object; the record keeps all of
them, the order they ran in and, for `--key`, each side's values, median, min and max.

    python tools/stream_ab.py --out profiles/devstream/host_bm.json --runs 3 --key stream_fps \\
        --side parent:/path/to/parent --side tree:. -- tools/bench_stream.py --frames 240 --matcher bm
"""
import argparse
import json
import os
import shlex
import statistics
import subprocess
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--key", default="stream_fps", help="the figure of the JSON line to summarise")
    ap.add_argument("--side", action="append", required=True, metavar="NAME:DIR[:EXTRA ARGS]")
    ap.add_argument("--timeout", type=float, default=240, help="seconds per run")
    ap.add_argument("command", nargs="+", help="script (relative to each side's DIR) and its arguments")
    a = ap.parse_args()
    sides = []
    for s in a.side:
        name, d, *extra = s.split(":", 2)
        sides.append((name, os.path.abspath(d), shlex.split(extra[0]) if extra else []))
    record = {"command": " ".join(a.command), "sides": {n: {"extra": e} for n, d, e in sides},
              "order": [], "runs": {}}
    for r in range(1, a.runs + 1):
        for name, d, extra in sides:
            tag = f"{name}_{r}"
            p = subprocess.run([sys.executable] + a.command + extra, cwd=d, capture_output=True, text=True,
                               timeout=a.timeout)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{tag} failed with status {p.returncode}: nothing more is started")
            record["order"].append(tag)
            record["runs"][tag] = json.loads(p.stdout.strip().splitlines()[-1])
            print(tag, record["runs"][tag].get(a.key), flush=True)
    record["summary"] = {}
    for name, _, _ in sides:
        v = [record["runs"][f"{name}_{r}"][a.key] for r in range(1, a.runs + 1)]
        record["summary"][name] = {"key": a.key, "values": v, "median": statistics.median(v), "min": min(v),
                                   "max": max(v)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
        f.write("\n")
    print(json.dumps(record["summary"]))


if __name__ == "__main__":
    main()
