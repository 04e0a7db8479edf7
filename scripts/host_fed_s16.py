#!/usr/bin/env python3
"""Host-fed and device-resident throughput of the float and the int16 input entries, back to back in one process.

The bench's `host_fed` leg (bench.py: C79, 2304 slots per batch, FLAG_ASYNC, a page-locked source, btgpu_process_host) on the
bench's capture quantised to int16 (peak 8000), fed once as float32 (the int16 values widened on the host, 8 bytes per sample)
and once as int16 (4 bytes per sample, widened in the kernels).  Per format: Gsamples/s host-fed, the host-to-device copy of
the same bytes alone, their ratio; and the device-resident step with the channel-bank and exact-rows kernel times
(FLAG_TIMING_BANK).  Every figure is the median of --repeats timed regions of --batches batches after a warm-up, with the
minimum and maximum beside it.  Prints one JSON line; --out writes it to a file as well.
--formats f32,s16,s8 picks the formats of this process (scripts/host_fed_formats.py runs one per process); with s8 among them the
capture is quantised to int8 (peak 127) and EVERY format carries those values."""
import argparse
import hashlib
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stat(xs, digits=3):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=2304)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--formats", default="f32,s16")
    ap.add_argument("--int8-values", action="store_true", help="quantise to peak 127 also when s8 is not among --formats")
    args = ap.parse_args()
    import torch
    from conftest import load_pkg
    pkg = load_pkg()
    synth = importlib.import_module("gr_bluetooth_amd.synth")
    fs, fc, S, hb = 100e6, 2441e6, args.slots, args.batches
    laps = tuple((0x24D952 + 0x10101 * i) & 0xFFFFFF for i in range(8))

    def block(flags):
        return pkg.multi_sniffer(fs, fc, 10.0, False, device=0, max_batch_slots=S, flags=pkg.FLAG_ASYNC | flags)
    b = block(0)
    H, slot, mg = b.design.history, b.design.samples_per_slot, b.design.left_margin
    b.close()
    seg, _ = synth.make_segment_torch(fs, fc, 0, S, "cuda", left_pad=H - 1 + mg, laps=laps, seed=1)
    f = torch.view_as_real(seg) if seg.is_complex() else seg.reshape(-1, 2)
    names = args.formats.split(",")
    peak = 127.0 if "s8" in names or args.int8_values else 8000.0
    q = torch.round(f * (peak / f.abs().max())).to(torch.int16).contiguous()
    n = q.shape[0]
    dev = {"f32": q.float().contiguous(), "s16": q, "s8": q.to(torch.int8).contiguous()}
    res = {"workload": "c79", "slots_per_batch": S, "batches": hb, "repeats": args.repeats, "samples_per_batch": S * slot,
           "build_id": hashlib.sha256(open(os.path.join(ROOT, "gr-bluetooth_amd", "libbtgpu.so"), "rb").read()).hexdigest()[:16]}
    res["peak"] = peak
    for name, fmt in ((nm, {"f32": pkg.FORMAT_F32, "s16": pkg.FORMAT_S16, "s8": getattr(pkg, "FORMAT_S8", None)}[nm]) for nm in names):
        pinned = dev[name].cpu().pin_memory()
        nbytes = pinned.numel() * pinned.element_size()
        # ---- host-fed ----
        b = block(0)
        for _ in range(2):
            b.process_host((pinned.data_ptr(), n), 0, S, left_margin=mg, fmt=fmt)
        b.flush(); b.poll_arrays()
        fed, nrec = [], 0
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(hb):
                b.process_host((pinned.data_ptr(), n), 0, S, left_margin=mg, fmt=fmt)
                nrec += len(b.poll_arrays())
            b.flush(); nrec += len(b.poll_arrays())
            torch.cuda.synchronize()
            fed.append(S * slot * hb / (time.perf_counter() - t0) / 1e9)
        b.close()
        # ---- the copy of the same bytes alone ----
        dst = torch.empty_like(dev[name])
        dst.copy_(pinned, non_blocking=True); torch.cuda.synchronize()
        cp = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(hb):
                dst.copy_(pinned, non_blocking=True)
            torch.cuda.synchronize()
            cp.append(S * slot * hb / (time.perf_counter() - t0) / 1e9)
        del dst
        # ---- device-resident step, bank and exact-rows kernel times ----
        b = block(pkg.FLAG_TIMING_BANK)
        ptr = dev[name].data_ptr()
        for _ in range(3):
            b.process_device(ptr, n, 0, S, left_margin=mg, fmt=fmt)
        b.flush(); b.poll_arrays()
        step, bank, exact = [], [], []
        for _ in range(args.repeats):
            t_a = b.timing()
            t0 = time.perf_counter()
            for _ in range(hb):
                b.process_device(ptr, n, 0, S, left_margin=mg, fmt=fmt)
                b.poll_arrays()
            b.flush(); b.poll_arrays()
            torch.cuda.synchronize()
            step.append((time.perf_counter() - t0) / hb * 1e3)
            t_b = b.timing()
            bank.append((t_b.kernel_ms[0] - t_a.kernel_ms[0]) / hb)
            exact.append((t_b.kernel_ms[7] - t_a.kernel_ms[7]) / hb)
        b.close()
        res[name] = {"bytes_per_batch": nbytes, "records_host_fed": nrec,
                     "host_fed_Gsps": stat(fed), "h2d_alone_Gsps": stat(cp), "h2d_alone_GBps": round(statistics.median(cp) * nbytes / (S * slot), 2),
                     "frac_of_h2d_alone": round(statistics.median(fed) / statistics.median(cp), 3),
                     "device_step_ms": stat(step), "device_Gsps": round(S * slot / statistics.median(step) / 1e6, 2),
                     "bank_kernel_ms": stat(bank), "exact_rows_kernel_ms": stat(exact)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
