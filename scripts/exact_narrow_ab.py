#!/usr/bin/env python3
"""The narrow form of the exact rows' kernel (csrc/exact_narrow.hip.h) against the sparse form, on one MI355X:

  c8   8 Msps, 2476.5 MHz, 8 channels, 16384 slots per step (BASELINE configs[1], bench.py's c8 leg and its capture)
  16   16 Msps, 2440 MHz, 15 channels, 8192 slots per step

each with BTGPU_EXACT_FORM=sparse and =narrow, in the block's configuration (ASYNC | LE | HEADERS, + TIMING_BANK), and the same again
with BTGPU_FLAG_EXACT_ALL.  Each run is a fresh child process, the two forms alternating, three runs each; a child times 30 steps
(one process_device over the batch each) on the wall clock behind 150 ms of load, the exact rows' kernel from btgpu_last_timing
(BTGPU_K_EXACT, per launch).  Writes profiles/exact_narrow_ab.json: medians and spreads (max - min), and the ratio sparse / narrow.

    python scripts/exact_narrow_ab.py [--out profiles/exact_narrow_ab.json]
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEGS = [("c8", 8e6, 2476.5e6, 16384), ("16", 16e6, 2440e6, 8192)]
FORMS = {"sparse": 1, "narrow": 3}                               # btgpu_exact_form()


def child(fs, fc, S):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    synth = importlib.import_module("gr_bluetooth_amd.synth")
    laps = tuple((0x24D952 + 0x10101 * i) & 0xFFFFFF for i in range(8))
    out, seg = {}, None
    for name, extra in (("presence", 0), ("exact_all", pkg.FLAG_EXACT_ALL)):
        b = pkg.multi_sniffer(fs, fc, 10.0, False, device=0, max_batch_slots=S,
                              flags=pkg.FLAG_ASYNC | pkg.FLAG_LE | pkg.FLAG_HEADERS | pkg.FLAG_TIMING_BANK | extra)
        d = b.design
        if seg is None:
            seg, _ = synth.make_segment_torch(fs, fc, 0, S, "cuda:0", left_pad=d.history - 1 + d.left_margin, laps=laps, seed=1, snr_db=25.0,
                                              occupancy=0.3, cfo_hz=75e3, max_payload_bits=2745)
            seg = seg.to("cuda:0").contiguous()
            torch.cuda.synchronize()

        def step(last):
            b.process_device(seg.data_ptr(), seg.shape[0], 0, S, left_margin=d.left_margin)
            if last:
                b.flush()
            return len(b.poll_arrays())

        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.15:
            step(False)
        step(True)
        torch.cuda.synchronize()
        tm0, K, hits = b.timing(), 30, 0
        t0 = time.perf_counter()
        for i in range(K):
            hits += step(i == K - 1)
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
        tm1 = b.timing()
        out[name] = {"exact_form": b.exact_form(), "decimation": d.decimation, "channels": d.high_channel - d.low_channel + 1,
                     "ms_per_step": el / K * 1e3, "gsamples_per_s": S * d.samples_per_slot * K / el / 1e9,
                     "exact_ms": (tm1.kernel_ms[7] - tm0.kernel_ms[7]) / max(1, tm1.kernel_launches[7] - tm0.kernel_launches[7]),
                     "exact_rows_per_step": (tm1.verify_rows - tm0.verify_rows) / K, "hits_per_step": hits // K}
        b.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_narrow_ab.json"))
    ap.add_argument("--child", type=float, nargs=3, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], int(a.child[2]))
    runs = {}
    for _ in range(3):
        for leg, fs, fc, S in LEGS:
            for form in FORMS:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(fs), str(fc), str(S)],
                                   env=dict(os.environ, BTGPU_EXACT_FORM=form), capture_output=True, text=True, timeout=240)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    return 2                                     # nothing more is started on the device behind a failed run
                res = json.loads(r.stdout.strip().splitlines()[-1])
                sys.stderr.write("%s %s: %s\n" % (leg, form, {k: (round(v["ms_per_step"], 3), round(v["exact_ms"], 3)) for k, v in res.items()}))
                for name, v in res.items():
                    if v["exact_form"] != FORMS[form]:
                        sys.stderr.write("%s: asked for %s, the handle runs form %d\n" % (leg, form, v["exact_form"]))
                        return 2
                    runs.setdefault("%s_%s_%s" % (leg, name, form), []).append(v)
    out = {"legs": {leg: {"sample_rate": fs, "center_freq": fc, "slots_per_step": S} for leg, fs, fc, S in LEGS}, "runs": runs, "summary": {}}
    s = out["summary"]
    for key, rs in runs.items():
        s[key] = {}
        for k in ("ms_per_step", "exact_ms", "gsamples_per_s"):
            v = sorted(r[k] for r in rs)
            s[key][k + "_median"], s[key][k + "_spread"] = v[1], v[-1] - v[0]
        s[key]["exact_rows_per_step"] = rs[0]["exact_rows_per_step"]
    for leg, _, _, _ in LEGS:
        for name in ("presence", "exact_all"):
            sp, na = s["%s_%s_sparse" % (leg, name)], s["%s_%s_narrow" % (leg, name)]
            s["%s_%s_sparse_over_narrow" % (leg, name)] = {
                "step": sp["ms_per_step_median"] / na["ms_per_step_median"], "exact_kernel": sp["exact_ms_median"] / na["exact_ms_median"],
                "narrow_faster_beyond_spread": bool(sp["ms_per_step_median"] - na["ms_per_step_median"] > max(sp["ms_per_step_spread"], na["ms_per_step_spread"]))}
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(s, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
