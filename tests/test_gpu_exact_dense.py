"""The dense form of the exact rows' kernel (csrc/exact_dense.hip.h: channels as the matrix rows, the decimation a run-time argument)
on the MI355X: bit for bit the DIRECT path's rows and the oracle's records, also at 56 / 60 Msps, where no sparse kernel exists."""
import os

import numpy as np
import pytest

import paritylib

LAPS = (0x24D952, 0x4831DD, 0x9E8B33)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,fc,nsl,s16", [(8e6, 2476.5e6, 3, False),      # D = 4, 8 channels: half a row block
                                            (20e6, 2441e6, 3, True),        # D = 10 (D % 4 != 0), second row block partial, int16 input
                                            (56e6, 2441e6, 3, False),       # D = 28: no sparse kernel
                                            (100e6, 2441e6, 3, False)])     # D = 50, five row blocks, the last with 14 channels
def test_dense_rows_equal_the_direct_path(pkg, synth, fs, fc, nsl, s16):
    """EVERY demodulated row of every channel (EXACT_ALL | EXACT_DENSE) against the bit-exact DIRECT path's stream: three slots in one
    batch -- two slot-last 111-output tiles, the clamped head of the stream, the batch's partial last tile."""
    iq, _ = synth.make_capture(fs, fc, nsl, laps=LAPS, seed=11, snr_db=22, occupancy=0.6, cfo_hz=60e3)
    samples = np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)
    if s16:
        samples = np.rint(samples * (8000.0 / np.abs(samples).max())).astype(np.int16)
    dense = pkg.multi_sniffer(fs, fc, 10.0, False, flags=pkg.FLAG_EXACT_ALL | pkg.FLAG_EXACT_DENSE, max_batch_slots=nsl)
    direct = pkg.multi_sniffer(fs, fc, 10.0, False, channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT, max_batch_slots=nsl)
    assert dense.design.channelizer == pkg.CHANNELIZER_POLYPHASE and dense.exact_form() == pkg.EXACT_DENSE
    d = dense.design
    G = d.samples_per_slot // d.decimation * (nsl - 1) + d.ddc_out
    for blk, x in ((dense, samples), (direct, samples.astype(np.float32))):
        full = np.concatenate([np.zeros((blk.history() - 1, 2), x.dtype), x])
        assert blk.work(full.reshape(-1)) == nsl * d.samples_per_slot
        blk.poll()
    for ch in range(d.low_channel, d.high_channel + 1):
        a, b = dense.debug_fetch(1, ch, 0, G), direct.debug_fetch(1, ch, 0, G)
        assert len(a) == G and np.array_equal(a[1:G], b[1:G]), ch
    dense.close(); direct.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fs,fc,nsl", [(8e6, 2476.5e6, 12), (56e6, 2441e6, 10), (60e6, 2441e6, 10), (100e6, 2441e6, 10)])   # (the oracle alone: 12, 9, 11, 11 records)
def test_dense_records_equal_the_oracle(pkg, po, synth, fs, fc, nsl):
    """EXACT_ALL | EXACT_DENSE on an explicit POLYPHASE request, across batch seams: every field of every record is the oracle's.  At
    56 / 60 Msps also the default flags: presence's marks on the dense kernel, whose stores are masked by the bitmap."""
    iq, truth = synth.make_capture(fs, fc, nsl, laps=LAPS, seed=23, snr_db=20, occupancy=0.6, cfo_hz=30e3, max_payload_bits=1500)
    want, _ = po.Oracle(fs, fc, 10.0, po.MODE_SNIFFER, le=True).run_stream(iq, threads=os.cpu_count() or 1)
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, le=True, flags=pkg.FLAG_EXACT_ALL | pkg.FLAG_EXACT_DENSE,
                            channelizer=pkg.CHANNELIZER_POLYPHASE, max_batch_slots=5)
    assert blk.exact_form() == pkg.EXACT_DENSE
    blk.push(iq)
    got = blk.poll()
    tm = blk.timing()
    blk.close()
    assert len(want) >= 6 and [h.key() for h in got] == [h.key() for h in want]
    assert tm.long_tasks == 0                                   # nothing left for a second run: every row was exact already
    if fs in (56e6, 60e6):
        # (test_gpu_parity._differential_of's own comparison; the helper itself insists on the staged squelch, which these rates lack)
        blk = pkg.multi_sniffer(fs, fc, 10.0, False, le=True)
        assert blk.design.channelizer == pkg.CHANNELIZER_POLYPHASE and blk.exact_form() == pkg.EXACT_DENSE
        blk.push(iq)
        got = blk.poll()
        tm = blk.timing()
        blk.close()
        assert tm.verify_rows > 0
        key = lambda hs: np.array([h.key() for h in hs], np.int64).reshape(-1, 7)
        d = paritylib.differential(key(got), key(want), truth, lag=6)
        assert d["planted_ref"] > 0 and d["planted_identical"] and d["planted_only_gpu"] == 0 and d["planted_only_ref"] == 0 and d["planted_offset_differs"] == 0, d
