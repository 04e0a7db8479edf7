#!/usr/bin/env python3
"""float32, int16 and int8 input on one build, and the float / int16 legs of a second build (the parent commit's tree) beside them.

Every leg is scripts/host_fed_s16.py --formats X in a FRESH process; the legs alternate (f32, s16, s8, then the other build's
f32, s16) and the whole round is run --rounds times (3).  Per format the figure kept is the median over the rounds of each
process's own median, with the smallest and largest round beside it: that spread is what a difference between two formats, or
between this build and the other, has to exceed.  All legs carry the same int8-valued capture.
    python scripts/host_fed_formats.py --out profiles/s8_host_fed.json [--other /path/to/parent/tree]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("host_fed_Gsps", "h2d_alone_Gsps", "frac_of_h2d_alone", "device_step_ms", "bank_kernel_ms", "exact_rows_kernel_ms")


def leg(tree, fmt, repeats, batches):
    # (the other tree runs THIS tree's host_fed_s16.py, copied into it: same capture, same values, its own library)
    cmd = [sys.executable, os.path.join(tree, "scripts", "host_fed_s16.py"), "--repeats", str(repeats), "--batches", str(batches),
           "--formats", fmt, "--int8-values"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("leg %s of %s failed (%d):\n%s" % (fmt, tree, r.returncode, r.stderr[-2000:]))
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--other", default="", help="a second built tree (the parent commit) whose f32 and s16 legs run in every round")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    runs = {}                                            # (build, format) -> [per-round figures]
    meta = {}
    for _ in range(args.rounds):
        for fmt in ("f32", "s16", "s8"):
            j = leg(ROOT, fmt, args.repeats, args.batches)
            meta = {k: j[k] for k in ("workload", "slots_per_batch", "batches", "repeats", "samples_per_batch", "build_id", "peak")}
            runs.setdefault(("this", fmt), []).append(j[fmt])
        if args.other:
            j = leg(args.other, "f32,s16", args.repeats, args.batches)
            meta["other_build_id"] = j["build_id"]
            for fmt in ("f32", "s16"):
                runs.setdefault(("other", fmt), []).append(j[fmt])
    res = dict(meta, rounds=args.rounds, method="fresh process per leg, legs alternating; median over rounds of each process's median, [min, max] over rounds")
    for (build, fmt), rs in runs.items():
        out = {"bytes_per_batch": rs[0]["bytes_per_batch"]}
        for k in KEYS:
            xs = [r[k]["median"] if isinstance(r[k], dict) else r[k] for r in rs]
            out[k] = {"median": round(statistics.median(xs), 3), "min": min(xs), "max": max(xs)}
        res.setdefault(build, {})[fmt] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
