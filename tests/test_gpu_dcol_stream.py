"""The 100-bin bank's handles keep ONE demodulated stream, tile-blocked dcol[tile][80][25]: the bank writes it, the exact rows
are recomputed in it, the window kernel stages from it (WinLayoutTiled), finish / verify-fill read it.  BTGPU_NO_DCOL=1 (read
when a handle is created) is the reference layout: time-major d[g][80] only, every consumer on d.  Nothing a user can see may
depend on the layout: the stream itself (debug_fetch gathers it from the tiles), every record, every exported symbol.
All cases: 100 Msps, 2441 MHz, 79 channels, multi_sniffer with LE."""
import os
import re

import numpy as np
import pytest

FS, FC = 100e6, 2441e6
SMAX = 7
LAPS = (0x24D952, 0x4831DD, 0x9E8B33)
_cap = {}


def _capture(synth, pkg):
    """One capture for all cases: SMAX + 6 slots with a handful of bursts, no zeros in front -- its first history() - 1 samples
    serve as the history of slot 0, so that the detection span of every window holds samples.  Float, and the same rounded to int16."""
    if not _cap:
        iq, truth = synth.make_capture(FS, FC, SMAX + 6, laps=LAPS, seed=41, snr_db=24, occupancy=0.8)
        f = iq.astype(np.complex64).view(np.float32).reshape(-1, 2)
        q = np.rint(f * (8000.0 / np.abs(f).max())).astype(np.int16)
        _cap["f32"] = q.astype(np.float32)              # (the same values in both formats)
        _cap["s16"] = q
    return _cap


class _layout:
    """A handle created with the default layout (reference=False) or with BTGPU_NO_DCOL=1."""
    def __init__(self, pkg, reference, **kw):
        self.pkg, self.reference, self.kw = pkg, reference, kw

    def __enter__(self):
        old = os.environ.pop("BTGPU_NO_DCOL", None)
        if self.reference:
            os.environ["BTGPU_NO_DCOL"] = "1"
        try:
            self.blk = self.pkg.multi_sniffer(FS, FC, 10.0, False, le=True, max_batch_slots=SMAX, **self.kw)
        finally:
            os.environ.pop("BTGPU_NO_DCOL", None)
            if old is not None:
                os.environ["BTGPU_NO_DCOL"] = old
        return self.blk

    def __exit__(self, *a):
        self.blk.close()


def _segment(blk, samples, first, n):
    """Slots [first, first + n) of the capture on the device: (tensor, left margin)."""
    import torch
    H, slot, mg = blk.history(), blk.output_multiple(), blk.design.left_margin
    lo = first * slot - (mg if first else 0)
    seg = torch.from_numpy(samples[lo:(first + n) * slot + H - 1].copy()).cuda()
    return seg, (mg if first else 0)


def _process(blk, pkg, samples, first, n):
    seg, mg = _segment(blk, samples, first, n)
    fmt = pkg.FORMAT_S16 if samples.dtype == np.int16 else pkg.FORMAT_F32
    blk.process_device(seg.data_ptr(), len(seg), first, n, left_margin=mg, fmt=fmt)


def _stream(blk, G):
    d = blk.design
    out = [blk.debug_fetch(1, c, 0, 1 << 22) for c in range(d.low_channel, d.high_channel + 1)]
    assert all(len(a) == G for a in out)
    return np.stack(out)


@pytest.mark.gpu
def test_layouts_give_the_same_stream_records_and_symbols(pkg, synth):
    """S = 1 (G = ddc_out, no multiple of 25: a partial last tile), 2, and 7 (no multiple of the window kernel's 3 slots per
    workgroup; crosses the slot-end exact tile of 110 rows and 25- and 114-row boundaries), float and int16 input, flags
    LE | HEADERS | EXACT_PAYLOAD: the whole demodulated stream of every channel bit for bit, every record in all seven fields and
    snr_db as a double, the header sweeps and the exported symbols of every hit."""
    cap = _capture(synth, pkg)
    flags = pkg.FLAG_HEADERS | pkg.FLAG_EXACT_PAYLOAD
    res = {}
    for reference in (False, True):
        with _layout(pkg, reference, flags=flags) as blk:
            d = blk.design
            assert d.channelizer == pkg.CHANNELIZER_POLYPHASE and d.high_channel - d.low_channel + 1 == 79
            ops = d.samples_per_slot // d.decimation
            for fmt in ("f32", "s16"):
                for S in (1, 2, SMAX):
                    G = ops * (S - 1) + d.ddc_out
                    _process(blk, pkg, cap[fmt], 0, S)
                    hits, hdrs, syms, lens = blk.poll_headers()
                    res[(reference, fmt, S)] = (_stream(blk, G), hits, hdrs, syms, lens)
            assert d.ddc_out % 25 != 0
    nrec = 0
    for fmt in ("f32", "s16"):
        for S in (1, 2, SMAX):
            (da, ha, hda, sa, la), (db, hb, hdb, sb, lb) = res[(False, fmt, S)], res[(True, fmt, S)]
            assert da.shape == db.shape and da.tobytes() == db.tobytes(), (fmt, S, int((da.view(np.uint32) != db.view(np.uint32)).sum()))
            assert len(ha) == len(hb) and ha.tobytes() == hb.tobytes(), (fmt, S)       # seven fields + snr_db as a double
            assert hda.tobytes() == hdb.tobytes() and la.tobytes() == lb.tobytes() and sa.tobytes() == sb.tobytes(), (fmt, S)
            nrec += len(ha)
        assert len(res[(False, fmt, SMAX)][1]) >= 4, "too few records to compare"
    print("layout A/B: %d records identical" % nrec)


@pytest.mark.gpu
def test_batch_seam_with_the_single_stream(pkg, synth):
    """The capture as two calls (4 + 3 slots) with the default layout and as one call with BTGPU_NO_DCOL=1: the six key fields
    of every record (nsym is documented as partition-dependent)."""
    cap = _capture(synth, pkg)["f32"]
    with _layout(pkg, False) as blk:
        _process(blk, pkg, cap, 0, 4)
        _process(blk, pkg, cap, 4, 3)
        two = sorted(h.key()[:6] for h in blk.poll())
    with _layout(pkg, True) as blk:
        _process(blk, pkg, cap, 0, SMAX)
        one = sorted(h.key()[:6] for h in blk.poll())
    assert len(one) >= 4 and two == one


@pytest.mark.gpu
@pytest.mark.parametrize("dense", [False, True], ids=["sparse", "dense"])
def test_exact_rows_land_in_the_single_stream(pkg, synth, dense):
    """EXACT_ALL, S = 3: every row of every channel, read back from the tiles, is bit for bit the DIRECT channelizer's (the
    pattern of test_exact_stage_rows_equal_the_direct_path) -- with the sparse form of the exact rows' kernel and the dense one."""
    cap = _capture(synth, pkg)["f32"]
    S = 3
    with _layout(pkg, False, flags=pkg.FLAG_EXACT_ALL | (pkg.FLAG_EXACT_DENSE if dense else 0)) as blk:
        assert blk.exact_form() == (pkg.EXACT_DENSE if dense else pkg.EXACT_SPARSE)
        d = blk.design
        G = (d.samples_per_slot // d.decimation) * (S - 1) + d.ddc_out
        _process(blk, pkg, cap, 0, S)
        blk.poll()
        fast = _stream(blk, G)
    with _layout(pkg, False, channelizer=pkg.CHANNELIZER_DIRECT, squelch=pkg.SQUELCH_DIRECT) as blk:
        _process(blk, pkg, cap, 0, S)
        blk.poll()
        exact = _stream(blk, G)
    assert fast[:, 1:].tobytes() == exact[:, 1:].tobytes(), int((fast[:, 1:].view(np.uint32) != exact[:, 1:].view(np.uint32)).sum())


@pytest.mark.gpu
def test_default_handle_allocates_no_time_major_stream(pkg, capfd, monkeypatch):
    """What btgpu_create reports with BTGPU_VERBOSE=1: the default handle has a tile-blocked stream and no time-major one, the
    reference layout the reverse; a handle's device memory differs by exactly that exchange, per context."""
    monkeypatch.setenv("BTGPU_VERBOSE", "1")
    got = {}
    for reference in (False, True):
        capfd.readouterr()
        with _layout(pkg, reference):
            pass
        m = re.search(r"btgpu_create: (\d+) contexts.*device memory (\d+) bytes, per context: time-major stream (\d+), tile-blocked stream (\d+)",
                      capfd.readouterr().err)
        assert m, "btgpu_create printed no memory figure"
        got[reference] = [int(v) for v in m.groups()]
    (nctx, total, tm, tb), (nctx_r, total_r, tm_r, tb_r) = got[False], got[True]
    assert tm == 0 and tb > 0 and tm_r > 0 and tb_r == 0 and nctx == nctx_r
    assert total_r - total == nctx * (tm_r - tb)
    assert abs(tm_r - tb) <= 3 * 8000 + 64 * 320            # the two layouts of one stream: equal but for the tile rounding
