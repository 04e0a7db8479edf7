"""The narrow form of the exact rows' kernel (csrc/exact_narrow.hip.h: eight channels x (re, im) as the 16 rows of
v_mfma_f32_16x16x4_f32, decimation <= 8) on the MI355X: bit for bit the DIRECT path's rows and the oracle's records."""
import os

import numpy as np
import pytest

import paritylib

LAPS = (0x24D952, 0x4831DD, 0x9E8B33)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,fc,dtype", [(4e6, 2476e6, np.int8),        # D = 2: one matrix instruction per tap block
                                          (8e6, 2476.5e6, np.float32),   # D = 4: one full row block
                                          (10e6, 2450e6, np.int16),      # D = 5: the K pad, second row block with two channels
                                          (16e6, 2440e6, np.float32)])   # D = 8: two full row blocks
def test_narrow_rows_equal_the_direct_path(pkg, synth, fs, fc, dtype):
    """EVERY demodulated row of every channel (EXACT_ALL | EXACT_NARROW) against the bit-exact DIRECT path's stream: three slots in one
    batch -- two slot-last 111-output tiles, the clamped head of the stream, the batch's partial last tile."""
    nsl = 3
    iq, _ = synth.make_capture(fs, fc, nsl, laps=LAPS, seed=11, snr_db=22, occupancy=0.6, cfo_hz=60e3)
    samples = np.ascontiguousarray(iq).view(np.float32).reshape(-1, 2)
    if dtype is not np.float32:
        samples = np.rint(samples * ((127.0 if dtype is np.int8 else 8000.0) / np.abs(samples).max())).astype(dtype)
    narrow = pkg.multi_sniffer(fs, fc, 10.0, False, flags=pkg.FLAG_EXACT_ALL | pkg.FLAG_EXACT_NARROW, max_batch_slots=nsl)
    direct = pkg.multi_sniffer(fs, fc, 10.0, False, channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT, max_batch_slots=nsl)
    assert narrow.design.channelizer == pkg.CHANNELIZER_POLYPHASE and narrow.exact_form() == pkg.EXACT_NARROW
    d = narrow.design
    G = d.samples_per_slot // d.decimation * (nsl - 1) + d.ddc_out
    for blk, x in ((narrow, samples), (direct, samples.astype(np.float32))):
        full = np.concatenate([np.zeros((blk.history() - 1, 2), x.dtype), x])
        assert blk.work(full.reshape(-1)) == nsl * d.samples_per_slot
        blk.poll()
    for ch in range(d.low_channel, d.high_channel + 1):
        a, b = narrow.debug_fetch(1, ch, 0, G), direct.debug_fetch(1, ch, 0, G)
        assert len(a) == G and np.array_equal(a[1:G], b[1:G]), ch
    narrow.close(); direct.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fs,fc,nsl", [(8e6, 2476.5e6, 12), (10e6, 2450e6, 12)])     # (the oracle alone: 12 and 8 records)
def test_narrow_records_equal_the_oracle(pkg, po, synth, fs, fc, nsl):
    """Across batch seams.  EXACT_ALL | EXACT_NARROW: every field of every record is the oracle's.  EXACT_NARROW alone: presence's
    marks on the narrow kernel, whose stores are masked by the bitmap, and the second run."""
    iq, truth = synth.make_capture(fs, fc, nsl, laps=LAPS, seed=23, snr_db=20, occupancy=0.6, cfo_hz=30e3, max_payload_bits=1500)
    want, _ = po.Oracle(fs, fc, 10.0, po.MODE_SNIFFER, le=True).run_stream(iq, threads=os.cpu_count() or 1)
    assert len(want) >= 6
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, le=True, flags=pkg.FLAG_EXACT_ALL | pkg.FLAG_EXACT_NARROW, max_batch_slots=5)
    assert blk.design.channelizer == pkg.CHANNELIZER_POLYPHASE and blk.exact_form() == pkg.EXACT_NARROW
    blk.push(iq)
    got = blk.poll()
    tm = blk.timing()
    blk.close()
    assert [h.key() for h in got] == [h.key() for h in want]
    assert tm.long_tasks == 0                                   # nothing left for a second run: every row was exact already
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, le=True, flags=pkg.FLAG_EXACT_NARROW, max_batch_slots=5)
    assert blk.exact_form() == pkg.EXACT_NARROW
    blk.push(iq)
    got = blk.poll()
    blk.close()
    key = lambda hs: np.array([h.key() for h in hs], np.int64).reshape(-1, 7)
    r = paritylib.differential(key(got), key(want), truth, lag=6)
    assert r["planted_ref"] > 0 and r["planted_identical"] and r["planted_only_gpu"] == 0 and r["planted_only_ref"] == 0, r


def test_narrow_gate(pkg):
    """The form exists on the polyphase channelizer up to a decimation of 8."""
    for kw in (dict(sample_rate=100e6, center_freq=2441e6), dict(sample_rate=8e6, center_freq=2476.5e6, channelizer=pkg.CHANNELIZER_DIRECT)):
        with pytest.raises(pkg.BtgpuError) as e:
            pkg.design_query(flags=pkg.FLAG_EXACT_NARROW, **kw)
        assert e.value.code == pkg.EUNSUPPORTED
    assert pkg.design_query(8e6, 2476.5e6, flags=pkg.FLAG_EXACT_NARROW).decimation == 4
