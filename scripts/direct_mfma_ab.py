#!/usr/bin/env python3
"""The direct-form banks on the matrix pipe (csrc/ddc_mfma.hip.h) against the vector-ALU form, on one MI355X:

  25 Msps   AUTO = DIRECT / DIRECT (segmented: 625 * sps is no multiple of the decimation)
  60 Msps   AUTO = POLYPHASE + the DIRECT squelch
  100 Msps  explicit DIRECT / DIRECT (shared grid, 79 channels)

each with BTGPU_DIRECT_FORM=valu and =mfma, at 2441 MHz, flags LE | TIMING, a device-resident synthetic capture.  Each run is a fresh
child process, the two forms alternating, three runs each; a step = one process_device over the batch, its time from device events
around enough steps for >= 0.3 s, the banks' own times from btgpu_last_timing.  Writes profiles/direct_mfma_ab.json: medians, the
ratio valu / mfma and the TFLOP/s of the reference's multiply-adds (8 * ntaps per output).

    python scripts/direct_mfma_ab.py [--slots 16] [--out profiles/direct_mfma_ab.json]
"""
import argparse
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [("25", 25e6, False), ("60", 60e6, False), ("100", 100e6, True)]     # (name, rate, explicit DIRECT / DIRECT)


def load_pkg():
    d = os.path.join(ROOT, "gr-bluetooth_amd")
    spec = importlib.util.spec_from_file_location("gr_bluetooth_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["gr_bluetooth_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def child(fs, direct, slots):
    import numpy as np
    import torch
    pkg = load_pkg()
    synth = importlib.import_module("gr_bluetooth_amd.synth")
    fc = 2441e6
    kw = dict(channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT) if direct else {}
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, le=True, flags=pkg.FLAG_TIMING, max_batch_slots=slots, **kw)
    d = blk.design
    iq, _ = synth.make_capture(fs, fc, slots, laps=(0x24D952, 0x4831DD, 0x9E8B33), seed=80, snr_db=20, occupancy=0.6, cfo_hz=30e3)
    x = np.concatenate([np.zeros(d.history - 1 + d.left_margin, np.complex64), iq.astype(np.complex64)])
    dev = torch.from_numpy(x.view(np.float32).reshape(-1, 2)).cuda()

    def steps(n):
        for _ in range(n):
            blk.process_device(dev.data_ptr(), len(x), 0, slots, left_margin=d.left_margin)
            blk.poll_arrays()

    steps(2)                                                     # clocks up, first-launch costs out
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 2
    while True:
        t0 = blk.timing()
        e0.record(); steps(n); e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= 300.0:
            break
        n *= 2
    t1 = blk.timing()
    nch = d.high_channel - d.low_channel + 1
    seg = d.samples_per_slot % d.decimation != 0
    outs_ch = (d.ddc_out * slots if seg else d.samples_per_slot // d.decimation * (slots - 1) + d.ddc_out) * nch
    outs_n = (d.noise_out if seg else d.samples_per_slot // d.decimation) * slots * nch
    r = {"ms_per_step": ms / n, "steps": n, "channelizer": d.channelizer, "squelch": d.squelch, "direct_form": blk.direct_form(),
         "channels": nch, "decimation": d.decimation}
    for name, k, outs, ntaps, on in (("channel", 0, outs_ch, d.ntaps_channel, d.channelizer == pkg.CHANNELIZER_DIRECT),
                                     ("noise", 2, outs_n, d.ntaps_noise, d.squelch == pkg.SQUELCH_DIRECT)):
        kms = (t1.kernel_ms[k] - t0.kernel_ms[k]) / n
        r[name + "_bank_ms"] = kms
        r[name + "_bank_tflops"] = 8.0 * ntaps * outs / (kms * 1e9) if on and kms > 0 else None      # (None: not a direct-form bank here)
    print(json.dumps(r))
    blk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "direct_mfma_ab.json"))
    ap.add_argument("--child", type=float, default=0.0)
    ap.add_argument("--direct", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, bool(a.direct), a.slots)
    runs = {}
    for _ in range(3):
        for name, fs, direct in RATES:
            for form in ("valu", "mfma"):
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(fs), "--direct", str(int(direct)), "--slots", str(a.slots)],
                                   env=dict(os.environ, BTGPU_DIRECT_FORM=form), capture_output=True, text=True, timeout=150)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    return 2                                     # nothing more is started on the device behind a failed run
                runs.setdefault(name + "_" + form, []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"slots_per_step": a.slots, "runs": runs, "summary": {}}
    med = lambda rs, k: None if rs[0][k] is None else sorted(r[k] for r in rs)[1]
    for name, rs in runs.items():
        v = sorted(r["ms_per_step"] for r in rs)
        out["summary"][name] = {"ms_per_step_median": v[1], "ms_per_step_spread": v[-1] - v[0],
                                **{k + "_median": med(rs, k) for k in ("channel_bank_ms", "noise_bank_ms", "channel_bank_tflops", "noise_bank_tflops")}}
    s = out["summary"]
    for name, _, _ in RATES:
        v, m = s[name + "_valu"], s[name + "_mfma"]
        s[name + "_valu_over_mfma"] = {"step": v["ms_per_step_median"] / m["ms_per_step_median"],
                                       "channel_bank": v["channel_bank_ms_median"] / m["channel_bank_ms_median"] if m["channel_bank_tflops_median"] else None,
                                       "noise_bank": v["noise_bank_ms_median"] / m["noise_bank_ms_median"],
                                       "faster_beyond_spread": bool(v["ms_per_step_median"] - m["ms_per_step_median"] > max(v["ms_per_step_spread"], m["ms_per_step_spread"]))}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out["summary"], indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
