"""Complex int8 input (btgpu_work_s8 / btgpu_process_host_s8 / btgpu_process_device_s8): the samples are widened inside the
kernels with (float)int8, which is exact, so every output must be BIT FOR BIT what the float entries give for the same values.
(Every capture below holds classic records of the CPU oracle on its int8-rounded samples: 9, 8, 9, 9, 8, 9, 9 at 7, 8, 20, 25,
56, 80, 100 Msps with S = 4, seed 8.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

S = 4                                           # slots per case
LAPS = (0x24D952, 0x4831DD, 0x9E8B33)
_captures = {}


def _capture(synth, fs, fc):
    """A synth capture with packets in every slot, scaled so that its peak is 127, rounded to int8, a handful of samples
    overwritten with the extremes and -1 (even and odd samples, either byte: a sign or byte-order error cannot hide)."""
    if (fs, fc) not in _captures:
        iq, _ = synth.make_capture(fs, fc, S, laps=LAPS, seed=8, snr_db=25, occupancy=1.0)
        f = iq.view(np.float32).reshape(-1, 2)
        q = np.rint(f * (127.0 / np.abs(f).max())).astype(np.int8)
        n = len(q)
        for i, v in ((3, (-128, 127)), (4, (127, -128)), (1001, (-1, 0)), (1002, (0, -1)), (n // 2 | 1, (-1, -128)), (n - 1, (-128, -1))):
            q[i] = v
        _captures[(fs, fc)] = q
    return _captures[(fs, fc)]


def _outputs(pkg, fs, fc, samples, direct, **kw):
    """One stream through process_host from its start and through process_device on a segment cut out of it with ONE sample
    more than the design's margin in front (every tile and column start changes parity against the buffer's base); after each:
    every field of every record, the demodulated stream of the outermost channels, the window energies and, on the DIRECT
    cases, both banks' outputs -- as bytes."""
    import torch
    if direct:
        kw.update(channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT)
    blk = pkg.multi_LAP(fs, fc, 10.0, max_batch_slots=S, **kw)
    fmt = {np.dtype(np.int8): pkg.FORMAT_S8, np.dtype(np.int16): pkg.FORMAT_S16}.get(samples.dtype, pkg.FORMAT_F32)
    H, slot, d = blk.history(), blk.output_multiple(), blk.design
    nch = d.high_channel - d.low_channel + 1
    full = np.concatenate([np.zeros((H - 1, 2), samples.dtype), samples])
    out = []

    def snap(nslots):
        hits = blk.poll()
        out.append([(h.slot, h.channel, h.kind, h.offset, h.lap, h.ac_errors, h.nsym, np.float64(h.snr_db).tobytes()) for h in hits])
        out.append([blk.debug_fetch(1, c, 0, 1 << 22).tobytes() for c in (d.low_channel, d.high_channel)])
        out.append((blk.debug_fetch(2, 0, 0, nslots * nch).tobytes(), blk.debug_fetch(3, 0, 0, nslots * nch).tobytes()))
        if direct:                                                    # (segmented rates: every window has its own outputs)
            out.append([blk.debug_fetch(w, c, 0, per * nslots).tobytes() for w, per in ((0, d.ddc_out), (5, d.noise_out))
                        for c in (d.low_channel, d.high_channel)])

    blk.process_host(full, 0, S)
    snap(S)
    a, mg = 1, d.left_margin + 1
    seg = torch.from_numpy(full[a * slot - mg:].copy()).cuda()
    blk.process_device(seg.data_ptr(), len(seg), a, S - a, left_margin=mg, fmt=fmt)
    snap(S - a)
    if fmt == pkg.FORMAT_S8:                                          # one sample off the documented 4-byte alignment
        with pytest.raises(pkg.BtgpuError) as e:
            blk.process_device(seg.data_ptr() + 2, len(seg) - 1, a, S - a, left_margin=mg - 1, fmt=fmt)
        assert e.value.code == pkg.EINVAL
    blk.close()
    return out


def _compare(pkg, synth, fs, fc, direct=False, **kw):
    q = _capture(synth, fs, fc)
    want = _outputs(pkg, fs, fc, q.astype(np.float32), direct, **kw)
    assert any(r[2] == pkg.KIND_AC for r in want[0]), "the float path gave no classic record to compare"
    got = _outputs(pkg, fs, fc, q, direct, **kw)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "output %d differs" % i
    assert len(got) == len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,fc,direct,flags", [
    (8e6, 2476.5e6, False, 0),                  # 8 channels: pfbm F8 with the fused squelch stage, exact rows D = 4
    (20e6, 2441e6, False, 0),                   # pfbm, exact rows D = 10
    (7e6, 2441e6, True, 0),                     # segmented, odd seg_stride (4375): ddc_direct
    (25e6, 2441e6, True, 0),                    # segmented, odd seg_stride (15625), D = 12
    (7e6, 2441e6, True, "DIRECT_MFMA"),         # ... the same on the matrix pipe: D = 3, one padded group
    (25e6, 2441e6, True, "DIRECT_MFMA"),
    (56e6, 2441e6, False, 0),                   # pfbm, DIRECT squelch, dense exact rows (D = 28)
    (80e6, 2441e6, False, 0),                   # pfbg, channel and noise forms
    (100e6, 2441e6, False, 0),                  # pfb100f fused, exact rows D = 50
    (100e6, 2441e6, False, "EXACT_ALL"),        # exact rows, every channel marked
    (8e6, 2476.5e6, False, "EXACT_DENSE"),      # the dense form at D = 4: half a row block
], ids=["8M", "20M", "7M-seg", "25M-seg", "7M-seg-mfma", "25M-seg-mfma", "56M", "80M", "100M", "100M-exact-all", "8M-dense"])
def test_int8_entries_equal_float_entries_bit_for_bit(pkg, synth, fs, fc, direct, flags):
    _compare(pkg, synth, fs, fc, direct, flags=getattr(pkg, "FLAG_" + flags) if flags else 0)


@pytest.mark.gpu
def test_int8_on_the_one_tile_100_bin_bank():
    """pfb100_kernel_s8: BTGPU_BANK is read once per process, so this case runs the comparison above in a process of its own."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, BTGPU_BANK="legacy"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.mark.gpu
def test_formats_mixed_from_call_to_call_give_the_float_records(pkg, synth):
    """float, int8, int16 chunks of one stream through btgpu_work*: the capture is int8-valued, so narrowing the carried margin
    changes nothing and the records are those of the all-float run."""
    fs, fc = 8e6, 2476.5e6
    q = _capture(synth, fs, fc)
    recs = {}
    for name, dtypes in (("float", (np.float32,) * 3), ("mixed", (np.float32, np.int8, np.int16))):
        blk = pkg.multi_LAP(fs, fc, 10.0)
        H, slot = blk.history(), blk.output_multiple()
        full = np.concatenate([np.zeros((H - 1, 2), np.int8), q])
        cuts = [0, slot, 3 * slot, S * slot]
        for dt, lo, hi in zip(dtypes, cuts, cuts[1:]):
            assert blk.work(full[lo:hi + H - 1].astype(dt).reshape(-1)) == hi - lo
        recs[name] = [(h.key(), np.float64(h.snr_db).tobytes()) for h in blk.poll()]
        blk.close()
    assert len(recs["float"]) > 2 and recs["mixed"] == recs["float"]


@pytest.mark.gpu
def test_btrx_amd_s8_prints_what_the_float_capture_prints(synth, tmp_path):
    btrx = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gr-bluetooth_amd", "host", "btrx_amd")
    q = _capture(synth, 8e6, 2476.5e6)
    q.tofile(str(tmp_path / "cap.s8"))
    q.astype(np.float32).tofile(str(tmp_path / "cap.cfile"))
    base = [btrx, "-f", "2476.5M", "-r", "8M", "-c", "2"]
    s8 = subprocess.run(base + ["-i", str(tmp_path / "cap.s8"), "--s8"], capture_output=True, text=True, timeout=120)
    floats = subprocess.run(base + ["-i", str(tmp_path / "cap.cfile")], capture_output=True, text=True, timeout=120)
    assert s8.returncode == 0 and floats.returncode == 0, (s8.stderr, floats.stderr)
    assert s8.stdout.count("GOT PACKET") > 2 and s8.stdout == floats.stdout


if __name__ == "__main__":                       # the child of test_int8_on_the_one_tile_100_bin_bank
    import importlib
    from conftest import load_pkg
    _pkg = load_pkg()
    _compare(_pkg, importlib.import_module("gr_bluetooth_amd.synth"), 100e6, 2441e6)
