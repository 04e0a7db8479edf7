"""The general-M polyphase bank with its DFT on the matrix pipe (csrc/pfbg.hip.h) on the MI355X: 66 .. 98 Msps on the fast path
(AUTO = POLYPHASE + STAGED + dense exact rows) against the bit-exact DIRECT path and the oracle, with the tolerances of the other
polyphase banks (test_gpu_parity.test_fast_path_small_rates_vs_oracle_and_direct)."""
import os

import numpy as np
import pytest

import paritylib

LAPS = (0x24D952, 0x4831DD, 0x9E8B33)
FC = 2441e6


def _int16(iq):
    f = np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)
    return np.rint(f * (8000.0 / np.abs(f).max())).astype(np.int16)


def _work(blk, samples, nsl, zeros_in_front=True):
    """The last nsl slots of `samples` through work(): behind a history of zeros, or of the samples in front of them."""
    full = np.concatenate([np.zeros((blk.history() - 1, 2), samples.dtype), samples]) if zeros_in_front else samples
    full = full[len(full) - (blk.history() - 1) - nsl * blk.design.samples_per_slot:]
    assert blk.work(full.reshape(-1)) == nsl * blk.design.samples_per_slot
    return blk.poll()


@pytest.mark.gpu
@pytest.mark.parametrize("fs,s16,staged_only", [(66e6, False, False),     # M = 66, 65 channels: the last row block holds 2 rows, K = 132 (BTGPU_BANK_FORM, below)
                                                (80e6, True, False),      # the full band, 158 of 160 rows, int16 input
                                                (98e6, False, False),     # D = 49, K = 196 (no multiple of 8), the largest LDS
                                                (56e6, False, True)])     # explicit STAGED beside pfbm_kernel: 55 channels, four row blocks
def test_bank_and_squelch_against_the_direct_path(pkg, synth, monkeypatch, fs, s16, staged_only):
    """Three slots in one batch: Y of EVERY channel rel-L2 <= 1e-5, E_on / E_off <= 1e-5, SNR <= 1e-4 dB against DIRECT (fed the
    same values); 56 Msps, where only the noise form is new: E_off and SNR.  At 66 Msps pfbm_kernel's channel form still fits the
    LDS and stays the default: the knob puts the new kernel there, the resolution asserted is AUTO's either way."""
    nsl = 3
    if fs == 66e6:
        monkeypatch.setenv("BTGPU_BANK_FORM", "mfma")
    # (seven slots in front, the sniffer's history: the windows' noise spans lie in the capture, not in zeros -- E_off > 0)
    iq, _ = synth.make_capture(fs, FC, nsl + 7, laps=LAPS, seed=11, snr_db=22, occupancy=0.6, cfo_hz=60e3)
    samples = _int16(iq) if s16 else np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)
    fast = pkg.multi_sniffer(fs, FC, 10.0, False, flags=pkg.FLAG_DEBUG_Y, max_batch_slots=nsl,
                             **(dict(squelch=pkg.SQUELCH_STAGED) if staged_only else {}))
    direct = pkg.multi_sniffer(fs, FC, 10.0, False, flags=pkg.FLAG_DEBUG_Y, channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT,
                               max_batch_slots=nsl)
    d = fast.design
    assert (d.channelizer, d.squelch) == (pkg.CHANNELIZER_POLYPHASE, pkg.SQUELCH_STAGED)
    nch = d.high_channel - d.low_channel + 1
    out = {}
    for name, blk, x in (("fast", fast, samples), ("direct", direct, samples.astype(np.float32))):
        _work(blk, x, nsl, zeros_in_front=False)
        out[name] = dict(Y={c: blk.debug_fetch(0, c, 0, 1 << 22) for c in range(d.low_channel, d.high_channel + 1)},
                         eon=blk.debug_fetch(2, 0, 0, nsl * nch), eoff=blk.debug_fetch(3, 0, 0, nsl * nch), snr=blk.debug_fetch(4, 0, 0, nsl * nch))
        blk.close()
    f, r = out["fast"], out["direct"]
    if not staged_only:
        for c in range(d.low_channel, d.high_channel + 1):
            n = min(len(f["Y"][c]), len(r["Y"][c]))
            err = np.linalg.norm(f["Y"][c][1:n] - r["Y"][c][1:n]) / np.linalg.norm(r["Y"][c][1:n])
            assert n > 1250 * (nsl - 1) and err <= 1e-5, (c, n, err)
    m = np.isfinite(r["snr"]) & (r["eoff"] > 0)
    assert 2 * m.sum() >= m.size == nsl * nch
    for key in ("eoff",) if staged_only else ("eon", "eoff"):
        err = np.max(np.abs(f[key][m] - r[key][m]) / r[key][m])
        print(fs, key, err)
        assert err <= 1e-5, (key, err)
    err = np.max(np.abs(f["snr"][m] - r["snr"][m]))
    print(fs, "snr", err)
    assert err <= 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("fs", [70e6, 98e6])                     # D = 35, 49: the dense exact rows' first decimations above 32, both odd
def test_exact_rows_equal_the_direct_path(pkg, synth, fs):
    """EVERY demodulated row of every channel under EXACT_ALL against the DIRECT path's stream, bit for bit (the loop of
    test_gpu_exact_dense.test_dense_rows_equal_the_direct_path)."""
    nsl = 3
    iq, _ = synth.make_capture(fs, FC, nsl, laps=LAPS, seed=11, snr_db=22, occupancy=0.6, cfo_hz=60e3)
    samples = np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)
    exact = pkg.multi_sniffer(fs, FC, 10.0, False, flags=pkg.FLAG_EXACT_ALL, max_batch_slots=nsl)
    direct = pkg.multi_sniffer(fs, FC, 10.0, False, channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT, max_batch_slots=nsl)
    d = exact.design
    assert (d.channelizer, d.squelch) == (pkg.CHANNELIZER_POLYPHASE, pkg.SQUELCH_STAGED) and exact.exact_form() == pkg.EXACT_DENSE
    G = d.samples_per_slot // d.decimation * (nsl - 1) + d.ddc_out
    for blk in (exact, direct):
        _work(blk, samples, nsl)
    for ch in range(d.low_channel, d.high_channel + 1):
        a, b = exact.debug_fetch(1, ch, 0, G), direct.debug_fetch(1, ch, 0, G)
        assert len(a) == G and np.array_equal(a[1:G], b[1:G]), ch
    exact.close(); direct.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fs,nsl,seed", [(80e6, 9, 23)])         # (the oracle alone: 6 records)
def test_records_at_80_msps(pkg, po, synth, fs, nsl, seed):
    """Across a batch seam (max_batch_slots about half the capture): EXACT_ALL -- every field of every record is the oracle's;
    default flags -- the planted records identical on six fields through presence + exact rows; int16 input -- its float twin's records."""
    iq, truth = synth.make_capture(fs, FC, nsl, laps=LAPS, seed=seed, snr_db=20, occupancy=0.6, cfo_hz=30e3, max_payload_bits=1500)
    want, _ = po.Oracle(fs, FC, 10.0, po.MODE_SNIFFER, le=True).run_stream(iq, threads=os.cpu_count() or 1)
    samples = np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)
    key = lambda hs: np.array([h.key() for h in hs], np.int64).reshape(-1, 7)

    def run(x, flags=0):
        blk = pkg.multi_sniffer(fs, FC, 10.0, False, le=True, flags=flags, max_batch_slots=(nsl + 1) // 2)
        assert (blk.design.channelizer, blk.design.squelch) == (pkg.CHANNELIZER_POLYPHASE, pkg.SQUELCH_STAGED)
        got = _work(blk, x, nsl)
        tm = blk.timing()
        blk.close()
        return got, tm

    got, _ = run(samples, pkg.FLAG_EXACT_ALL)
    assert len(want) >= 6 and [h.key() for h in got] == [h.key() for h in want]
    got, tm = run(samples)
    assert tm.verify_rows > 0
    d = paritylib.differential(key(got), key(want), truth, lag=6)
    assert d["planted_ref"] > 0 and d["planted_identical"] and d["planted_only_gpu"] == 0 and d["planted_only_ref"] == 0 and d["planted_offset_differs"] == 0, d
    q = _int16(iq)
    a, _ = run(q)
    b, _ = run(q.astype(np.float32))
    assert len(a) > 0 and [h.key() for h in a] == [h.key() for h in b]
