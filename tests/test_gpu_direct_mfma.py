"""The direct-form banks on the matrix pipe (csrc/ddc_mfma.hip.h, BTGPU_FLAG_DIRECT_MFMA) on the MI355X: bit for bit the vector-ALU
form's channel and noise bank outputs, within 1e-5 of a float64 evaluation, and the oracle's records at the segmented rates."""
import numpy as np
import pytest

FC, NSL, NCAP = 2441e6, 3, 12      # three slots per batch; four batches, so that the last one's windows lie in the capture, not in the history's zeros
LAPS = (0x24D952, 0x4831DD, 0x9E8B33)


@pytest.mark.gpu
@pytest.mark.parametrize("fs,s16", [(7e6, False),      # segmented; D = 3: one padded 16-byte group; a partial row block
                                    (8e6, False),      # shared grid; D = 4; C8
                                    (25e6, True),      # segmented; D = 12; a full row block + a partial one; int16 input
                                    (100e6, False)])   # shared grid; D = 50; 79 channels; the noise bank's NB not a multiple of the chunk
def test_direct_mfma_equals_the_valu_form(pkg, po, synth, fs, s16):
    iq, _ = synth.make_capture(fs, FC, NCAP, laps=LAPS, seed=11, snr_db=25, occupancy=0.9, cfo_hz=40e3)
    kw = dict(channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT, max_batch_slots=NSL)
    mfma = pkg.multi_sniffer(fs, FC, 10.0, False, le=True, flags=pkg.FLAG_DIRECT_MFMA, **kw)
    valu = pkg.multi_sniffer(fs, FC, 10.0, False, le=True, **kw)
    assert mfma.direct_form() == pkg.DIRECT_MFMA and valu.direct_form() == pkg.DIRECT_VALU
    d = mfma.design
    seg = d.samples_per_slot % d.decimation != 0              # every window on its own decimation phase
    # the capture cut so that the last window's span ends at the end of the input (the clamped and zeroed loads)
    x = np.ascontiguousarray(iq[:NCAP * d.samples_per_slot]).view(np.float32).reshape(-1, 2)
    if s16:
        x = np.rint(x * (8000.0 / np.abs(x).max())).astype(np.int16)
    full = np.concatenate([np.zeros((d.history - 1, 2), x.dtype), x])
    for blk in (mfma, valu):
        assert blk.work(full.reshape(-1)) == NCAP * d.samples_per_slot
    got = [h.key() for h in mfma.poll()]
    G = d.ddc_out * NSL if seg else d.samples_per_slot // d.decimation * (NSL - 1) + d.ddc_out
    Gn = (d.noise_out if seg else d.samples_per_slot // d.decimation) * NSL
    # ---- the last batch's outputs; float64 reference of the channel bank: NCO mix, FIR, decimate; a unit phase per rotator restart ----
    h = pkg.filter_taps(fs, 0).astype(np.float64)
    xc = full.astype(np.float64) @ np.array([1.0, 1j])
    nn = np.arange(len(xc))
    starts = [k * d.samples_per_slot for k in range(NCAP - NSL, NCAP)] if seg else [(NCAP - NSL) * d.samples_per_slot]   # the last batch
    per = d.ddc_out if seg else G
    for ch in range(d.low_channel, d.high_channel + 1):
        for what, cnt in ((0, G), (5, Gn)):
            a, b = mfma.debug_fetch(what, ch, 0, cnt), valu.debug_fetch(what, ch, 0, cnt)
            assert len(a) == cnt and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (ch, what)
        Y = mfma.debug_fetch(0, ch, 0, G).astype(np.complex128)
        win = np.lib.stride_tricks.sliding_window_view(xc * np.exp(-2j * np.pi * (2402e6 + ch * 1e6 - FC) / fs * nn), len(h))
        err = ref2 = 0.0
        for k, s0 in enumerate(starts):
            ref = win[d.first_channel_sample + s0 + np.arange(per) * d.decimation] @ h[::-1]
            y = Y[k * per:(k + 1) * per]
            e = np.vdot(ref, ref).real                          # (0: a first window that lies in the history's zeros)
            c = np.vdot(ref, y) / e if e > 0 else 1.0
            assert abs(abs(c) - 1) < 1e-5
            err += np.linalg.norm(y - c * ref) ** 2
            ref2 += np.linalg.norm(ref) ** 2
        assert np.sqrt(err / ref2) <= 1e-5, ch
    mfma.close(); valu.close()
    if seg:                                                       # the DIRECT contract, end to end through the window kernel
        want, _ = po.Oracle(fs, FC, 10.0, po.MODE_SNIFFER, le=True).run_stream((x.astype(np.float32) @ np.array([1.0, 1j])).astype(np.complex64))
        assert len(want) > 0 and got == [h.key() for h in want]
