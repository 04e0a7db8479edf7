#!/usr/bin/env python3
"""What the payload sweep (csrc/payload_sweep.hip.h, BTGPU_FLAG_PAYLOAD_SWEEP) costs and saves, on one MI355X, in the `c8`
configuration of bench.py's result line (8 channels at 8 Msps, 16384 slots per step, ASYNC | LE | HEADERS, a device-resident
synthetic capture with bench.py's generator settings):

  step      ms per step with and without the flag (driver-timed, no event flags), and with BTGPU_FLAG_TIMING the tail of a batch
            (finish -> nsym -> header sweep [-> payload sweep] -> record copies) with and without it: the difference is the new
            kernel's time where it runs, beside the next batches' kernels
  sweeps    the hit windows of one step: the device's time for all their sweeps (the tail difference above) against the host's for
            the same 64 crc_check calls per record through bt_host_crc_check on one thread (the cost of an empty call subtracted)

Every run is a fresh child process, the forms alternating, three runs each: medians and spreads.  Run it on the parent commit with
--parent (no flag exists there: the `off` form only) to get the reference for "the flag is free when off".
Writes profiles/payload_sweep_ab.json.

    python scripts/payload_sweep_ab.py [--slots 16384] [--out profiles/payload_sweep_ab.json] [--parent]
"""
import argparse
import ctypes
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


def load_pkg():
    d = os.path.join(ROOT, "gr-bluetooth_amd")
    spec = importlib.util.spec_from_file_location("gr_bluetooth_amd", os.path.join(d, "__init__.py"), submodule_search_locations=[d])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["gr_bluetooth_amd"] = mod
    spec.loader.exec_module(mod)
    return mod


def child(form, slots, timing, host):
    import numpy as np
    import torch
    pkg = load_pkg()
    synth = importlib.import_module("gr_bluetooth_amd.synth")
    flags = pkg.FLAG_ASYNC | pkg.FLAG_LE | pkg.FLAG_HEADERS | pkg.FLAG_EXACT_PAYLOAD | (pkg.FLAG_TIMING if timing else 0)
    if form == "on":
        flags |= pkg.FLAG_PAYLOAD_SWEEP
    blk = pkg.multi_sniffer(FS, FC, 10.0, False, device=0, max_batch_slots=slots, flags=flags)
    d = blk.design
    laps = tuple((0x24D952 + 0x10101 * i) & 0xFFFFFF for i in range(8))
    seg, _ = synth.make_segment_torch(FS, FC, 0, slots, "cuda:0", left_pad=d.history - 1 + d.left_margin, laps=laps, seed=1, snr_db=25.0,
                                      occupancy=0.3, cfo_hz=75e3, max_payload_bits=2745)
    seg = seg.contiguous()
    torch.cuda.synchronize()

    def step(last):
        blk.process_device(seg.data_ptr(), seg.shape[0], 0, slots, left_margin=d.left_margin)
        if last:
            blk.flush()
        return len(blk.poll_arrays())

    gc.collect()
    gc.disable()
    t_pre = time.perf_counter()
    while time.perf_counter() - t_pre < 0.15:                       # clocks up
        step(False)
    step(True)
    torch.cuda.synchronize()
    K = 20
    tm0 = blk.timing()
    t0 = time.perf_counter()
    n = 0
    for i in range(K):
        n += step(i == K - 1)
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    tm1 = blk.timing()
    r = {"form": form, "timing": bool(timing), "ms_per_step": el / K * 1e3, "records_per_step": n // K}
    if timing:
        k = pkg.K_FINISH if hasattr(pkg, "K_FINISH") else 5
        r["tail_ms"] = (tm1.kernel_ms[k] - tm0.kernel_ms[k]) / max(1, tm1.kernel_launches[k] - tm0.kernel_launches[k])
    if host:
        # one step's records with their symbols; the host's 64 crc_check calls per classic record whose header decodes
        blk.process_device(seg.data_ptr(), seg.shape[0], 0, slots, left_margin=d.left_margin)
        blk.flush()
        hits, hdrs, syms, lens = blk.poll_headers(sym_cap=3125)
        L = ctypes.CDLL(os.path.join(ROOT, "gr-bluetooth_amd", "libgnuradio-bluetooth-amd.so"))
        f = L.bt_host_crc_check
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        rows = [i for i in range(len(hits)) if hits[i]["kind"] == pkg.KIND_AC and hdrs[i]["fec13_ok"]]
        ty, ua = hdrs["type"].astype(int).tolist(), hdrs["uap"].astype(int).tolist()
        base = syms.ctypes.data
        t0 = time.perf_counter()
        for i in rows:
            p, ln, t, u = base + i * syms.shape[1], int(lens[i]), ty[i], ua[i]
            for c in range(64):
                f(p, ln, c, t[c], u[c])
        work = time.perf_counter() - t0
        t0 = time.perf_counter()
        for i in rows:
            p, t, u = base + i * syms.shape[1], ty[i], ua[i]
            for c in range(64):
                f(p, 0, c, 0, u[c])                                 # type 0, no symbols: the call and the packet object alone
        empty = time.perf_counter() - t0
        r.update(host_records=len(rows), host_ms=work * 1e3, host_empty_call_ms=empty * 1e3)
    gc.enable()
    print(json.dumps(r))
    blk.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "payload_sweep_ab.json"))
    ap.add_argument("--parent", action="store_true", help="the `off` form only (a tree without the flag)")
    ap.add_argument("--child", default="")
    ap.add_argument("--timing", type=int, default=0)
    ap.add_argument("--host", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.slots, a.timing, a.host)
    forms = ["off"] if a.parent else ["off", "on"]
    runs = {}
    for rep in range(3):
        for timing in (0, 1):
            for form in forms:
                host = int(rep == 0 and timing == 0 and form == "off")
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", form, "--slots", str(a.slots), "--timing", str(timing),
                                    "--host", str(host)], capture_output=True, text=True, timeout=280)
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    return 2                                     # nothing more is started on the device behind a failed run
                runs.setdefault(form + ("_timing" if timing else ""), []).append(json.loads(r.stdout.strip().splitlines()[-1]))
    out = {"slots_per_step": a.slots, "tree": "parent" if a.parent else "this", "runs": runs, "summary": {}}
    s = out["summary"]
    for name, rs in runs.items():
        v = sorted(r["ms_per_step"] for r in rs)
        s[name] = {"ms_per_step_median": v[1], "ms_per_step_spread": v[-1] - v[0], "records_per_step": rs[0]["records_per_step"]}
        if "tail_ms" in rs[0]:
            t = sorted(r["tail_ms"] for r in rs)
            s[name].update(tail_ms_median=t[1], tail_ms_spread=t[-1] - t[0])
    h = runs["off"][0]
    s["host"] = {"records": h["host_records"], "crc_check_ms": h["host_ms"] - h["host_empty_call_ms"], "empty_calls_ms": h["host_empty_call_ms"]}
    if not a.parent:
        dev = s["on_timing"]["tail_ms_median"] - s["off_timing"]["tail_ms_median"]
        s["device_sweeps_ms"] = dev
        s["host_over_device"] = s["host"]["crc_check_ms"] / dev if dev > 0 else None
        s["step_on_minus_off_ms"] = s["on"]["ms_per_step_median"] - s["off"]["ms_per_step_median"]
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(s, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
