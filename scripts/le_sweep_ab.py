#!/usr/bin/env python3
"""What the LE sweep (csrc/le_sweep.hip.h, BTGPU_FLAG_LE_SWEEP) costs, on one MI355X, in the `c8` configuration of bench.py's
result line (8 channels at 8 Msps, 16384 slots per step, ASYNC | LE | HEADERS, a device-resident synthetic capture with bench.py's
generator settings):

  step      ms per step with and without the flag (driver-timed, no event flags) -- and, with --parent-root DIR (a built checkout of
            the parent commit), of the parent's library in the same alternation: the reference for "the flag is free when off"
  tail      with BTGPU_FLAG_TIMING the tail of a batch (finish -> nsym -> header sweep [-> LE sweep] -> record copies) with and
            without the flag: the difference is the new kernels' time where they run, beside the next batches' kernels

Every run is a fresh child process, the forms alternating, three runs each: medians and spreads.
Writes profiles/le_sweep_ab.json.

    python scripts/le_sweep_ab.py [--slots 16384] [--out profiles/le_sweep_ab.json] [--parent-root DIR]
"""
import argparse
import gc
import importlib
import importlib.util
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FS, FC = 8e6, 2476.5e6


def load_pkg(root):
    d = os.path.join(root, "gr-bluetooth_amd")
    spec = importlib.util.spec_from_file_location("gr_bluetooth_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["gr_bluetooth_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def child(form, slots, timing, root):
    import torch
    pkg = load_pkg(root)
    synth = importlib.import_module("gr_bluetooth_amd.synth")
    flags = pkg.FLAG_ASYNC | pkg.FLAG_LE | pkg.FLAG_HEADERS | pkg.FLAG_EXACT_PAYLOAD | (pkg.FLAG_TIMING if timing else 0)
    if form == "on":
        flags |= pkg.FLAG_LE_SWEEP
    blk = pkg.multi_sniffer(FS, FC, 10.0, False, device=0, max_batch_slots=slots, flags=flags)
    d = blk.design
    laps = tuple((0x24D952 + 0x10101 * i) & 0xFFFFFF for i in range(8))
    seg, _ = synth.make_segment_torch(FS, FC, 0, slots, "cuda:0", left_pad=d.history - 1 + d.left_margin, laps=laps, seed=1, snr_db=25.0,
                                      occupancy=0.3, cfo_hz=75e3, max_payload_bits=2745)
    seg = seg.contiguous()
    torch.cuda.synchronize()
    aa = 0

    def step(last):
        nonlocal aa
        blk.process_device(seg.data_ptr(), seg.shape[0], 0, slots, left_margin=d.left_margin)
        if last:
            blk.flush()
        hits = blk.poll_arrays()
        aa += int((hits["kind"] == pkg.KIND_AA).sum())
        return len(hits)

    gc.collect()
    gc.disable()
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.15:                       # clocks up
        step(False)
    step(True)
    torch.cuda.synchronize()
    K = 20
    tm0 = blk.timing()
    aa = 0
    t0 = time.perf_counter()
    n = 0
    for i in range(K):
        n += step(i == K - 1)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    tm1 = blk.timing()
    r = {"form": form, "timing": bool(timing), "ms_per_step": el / K * 1e3, "records_per_step": n // K, "aa_records_per_step": aa // K}
    if timing:
        k = pkg.K_FINISH if hasattr(pkg, "K_FINISH") else 5
        r["tail_ms"] = (tm1.kernel_ms[k] - tm0.kernel_ms[k]) / max(1, tm1.kernel_launches[k] - tm0.kernel_launches[k])
    gc.enable()
    print(json.dumps(r))
    blk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "le_sweep_ab.json"))
    ap.add_argument("--parent-root", default="", help="a built checkout of the parent commit: its `off` form runs in the alternation")
    ap.add_argument("--child", default="")
    ap.add_argument("--timing", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child("off" if a.child == "parent" else a.child, a.slots, a.timing, a.parent_root if a.child == "parent" else ROOT)
    forms = (["parent"] if a.parent_root else []) + ["off", "on"]
    runs = {}
    for rep in range(3):
        for timing in (0, 1):
            for form in forms:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--slots", str(a.slots), "--timing", str(timing),
                                    "--parent-root", a.parent_root], capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    return 2                                     # nothing more is started on the device behind a failed run
                runs.setdefault(form + ("_timing" if timing else ""), []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"slots_per_step": a.slots, "runs": runs, "summary": {}}
    s = out["summary"]
    for name, rs in runs.items():
        v = sorted(r["ms_per_step"] for r in rs)
        s[name] = {"ms_per_step_median": v[1], "ms_per_step_spread": v[-1] - v[0], "records_per_step": rs[0]["records_per_step"],
                   "aa_records_per_step": rs[0]["aa_records_per_step"]}
        if "tail_ms" in rs[0]:
            t = sorted(r["tail_ms"] for r in rs)
            s[name].update(tail_ms_median=t[1], tail_ms_spread=t[-1] - t[0])
    s["device_sweeps_ms"] = s["on_timing"]["tail_ms_median"] - s["off_timing"]["tail_ms_median"]
    s["step_on_minus_off_ms"] = s["on"]["ms_per_step_median"] - s["off"]["ms_per_step_median"]
    if a.parent_root:
        s["step_off_minus_parent_ms"] = s["off"]["ms_per_step_median"] - s["parent"]["ms_per_step_median"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(s, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
