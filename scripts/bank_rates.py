#!/usr/bin/env python3
"""The general-M bank (csrc/pfbg.hip.h) against its yardsticks, on one MI355X:

  80 Msps / 2441 MHz / 79 channels, the drop-in block's flags (ASYNC | LE | HEADERS) + TIMING_BANK, a device-resident synthetic capture:
      default (POLYPHASE + STAGED + exact rows)   against   BTGPU_AUTO=direct (the path these rates had before)
  64 Msps, the same flags:   BTGPU_BANK_FORM=mfma   against   the default there (pfbm_kernel)          -- reported, not gated

Each configuration runs in a fresh child process, alternating, three runs each; a step = one process_device over the batch, its time
from device events around enough steps for >= 0.5 s.  Writes profiles/bank_mfma_rates.json; exit status 1 when the 80 Msps default
does not beat its yardstick by more than the spread of the runs.

    python scripts/bank_rates.py [--slots 48] [--out profiles/bank_mfma_rates.json]
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = [("80_default", 80e6, {}), ("80_auto_direct", 80e6, {"BTGPU_AUTO": "direct"}),
           ("64_default_pfbm", 64e6, {}), ("64_bank_form_mfma", 64e6, {"BTGPU_BANK_FORM": "mfma"})]


def load_pkg():
    d = os.path.join(ROOT, "gr-bluetooth_amd")
    spec = importlib.util.spec_from_file_location("gr_bluetooth_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["gr_bluetooth_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def child(fs, slots):
    import numpy as np
    import torch
    pkg = load_pkg()
    synth = importlib.import_module("gr_bluetooth_amd.synth")
    fc = 2441e6
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, le=True, flags=pkg.FLAG_ASYNC | pkg.FLAG_HEADERS | pkg.FLAG_TIMING_BANK, max_batch_slots=slots)
    d = blk.design
    iq, _ = synth.make_capture(fs, fc, slots, laps=(0x24D952, 0x4831DD, 0x9E8B33), seed=80, snr_db=20, occupancy=0.6, cfo_hz=30e3)
    x = np.concatenate([np.zeros(d.history - 1 + d.left_margin, np.complex64), iq.astype(np.complex64)])
    dev = torch.from_numpy(x.view(np.float32).reshape(-1, 2)).cuda()

    def steps(n):
        for _ in range(n):
            blk.process_device(dev.data_ptr(), len(x), 0, slots, left_margin=d.left_margin)
            blk.poll_arrays()
        blk.flush()
        blk.poll_arrays()

    steps(10)                                                    # clocks up, first-launch costs out
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n, ms = 8, 0.0
    while True:
        t0 = blk.timing()
        e0.record(); steps(n); e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 500.0:
            break
        n *= 2
    t1 = blk.timing()
    bank = (t1.kernel_ms[0] - t0.kernel_ms[0]) / n
    exact = (t1.kernel_ms[7] - t0.kernel_ms[7]) / n
    nch = d.high_channel - d.low_channel + 1
    instants = d.samples_per_slot // d.decimation * slots
    print(json.dumps({"ms_per_step": ms / n, "gsamples_per_s": slots * d.samples_per_slot / (ms / n) / 1e6, "bank_ms": bank, "exact_rows_ms": exact,
                      "bank_ns_per_instant_channel": bank * 1e6 / (instants * nch), "steps": n, "channelizer": d.channelizer, "squelch": d.squelch,
                      "exact_form": blk.exact_form()}))
    blk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bank_mfma_rates.json"))
    ap.add_argument("--child", type=float, default=0.0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.slots)
    runs = {name: [] for name, _, _ in CONFIGS}
    for _ in range(3):
        for name, fs, env in CONFIGS:
            e = dict(os.environ, **env)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(fs), "--slots", str(a.slots)], env=e,
                               capture_output=True, text=True, timeout=120)
            if r.returncode != 0:
                sys.stderr.write(r.stderr)
                return 2                                         # nothing more is started on the device behind a failed run
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"slots_per_step": a.slots, "runs": runs, "summary": {}}
    for name, rs in runs.items():
        v = sorted(r["ms_per_step"] for r in rs)
        out["summary"][name] = {"ms_per_step_median": v[1], "ms_per_step_spread": v[-1] - v[0],
                                "gsamples_per_s_median": sorted(r["gsamples_per_s"] for r in rs)[1],
                                "bank_ms_median": sorted(r["bank_ms"] for r in rs)[1], "exact_rows_ms_median": sorted(r["exact_rows_ms"] for r in rs)[1],
                                "bank_ns_per_instant_channel_median": sorted(r["bank_ns_per_instant_channel"] for r in rs)[1]}
    s = out["summary"]
    spread = max(s["80_default"]["ms_per_step_spread"], s["80_auto_direct"]["ms_per_step_spread"])
    out["summary"]["speedup_80_default_over_direct"] = s["80_auto_direct"]["ms_per_step_median"] / s["80_default"]["ms_per_step_median"]
    out["summary"]["wins_80"] = bool(s["80_auto_direct"]["ms_per_step_median"] - s["80_default"]["ms_per_step_median"] > spread)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"], indent=1))
    return 0 if out["summary"]["wins_80"] else 1


if __name__ == "__main__":
    sys.exit(main())
