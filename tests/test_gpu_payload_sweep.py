"""payload_sweep_kernel (csrc/payload_sweep.hip.h): classic_packet::crc_check under the 64 CLK1-6 candidates on the GPU, integer
for integer against the oracle's (oracle/bt_uap.c bto_crc_check) with the type and UAP of the header sweep for the same clock."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAP, UAP = 0x4831DD, 0x6B
# kind -> (builder of (bits), body lengths from the smallest to the type's maximum, symbols of the payload header, FEC 2/3)
KINDS = {
    "POLL": (lambda sy, clk, n, rng: sy.classic_poll_bits(LAP, UAP, clk), (0,), 0, False),
    "DM1": (lambda sy, clk, n, rng: sy.classic_dm1_bits(LAP, UAP, clk, rng.bytes(n)), (0, 17), 15, True),
    "FHS": (lambda sy, clk, n, rng: sy.classic_fhs_bits(LAP, UAP, clk, 0xABCDEF, 0x47, 0x1234, int(rng.integers(0, 1 << 26))), (0,), 0, True),
    "DH1": (lambda sy, clk, n, rng: sy.classic_dh1_bits(LAP, UAP, clk, rng.bytes(n)), (0, 27), 8, False),
    "DH3": (lambda sy, clk, n, rng: sy.classic_dh_multislot_bits(LAP, UAP, clk, rng.bytes(n), ptype=11), (0, 183), 16, False),
    "DH5": (lambda sy, clk, n, rng: sy.classic_dh_multislot_bits(LAP, UAP, clk, rng.bytes(n), ptype=15), (1, 339), 16, False),
    "DM3": (lambda sy, clk, n, rng: sy.classic_dm_multislot_bits(LAP, UAP, clk, rng.bytes(n), ptype=10), (0, 121), 30, True),
    "DM5": (lambda sy, clk, n, rng: sy.classic_dm_multislot_bits(LAP, UAP, clk, rng.bytes(n), ptype=14), (0, 80, 224), 30, True),
}


def _capture(synth, fs, fc):
    # (8 of the 79 channels are in an 8 Msps band: 320 slots of a hopping master leave a few dozen visible packets)
    return synth.make_hopping_capture(fs, fc, 320, LAP, UAP, 0x2A5F3C1, seed=9, dh1_fraction=0.8)


def _compare(pkg, po, packets, to_header):
    """Every packet (symbols from the preamble on) through the parity entry; with to_header = 68 the device gets them from the
    sync word on, as libbtbb's offset would.  Returns the oracle's verdicts [n][64] (-1 where try_clock fails)."""
    skip = 72 - to_header
    hdrs, crcs = pkg.debug_payload_sweep([s[skip:] for s in packets], to_header=to_header)
    want = np.full((len(packets), 64), -1, np.int64)
    for i, s in enumerate(packets):
        assert bool(hdrs[i]["fec13_ok"]) == po.try_clock(s, 0)[2]
        if hdrs[i]["fec13_ok"]:
            want[i] = [po.crc_check(s, c, int(hdrs[i]["type"][c]), int(hdrs[i]["uap"][c])) for c in range(64)]
        assert crcs[i]["length"] == len(s) - skip
        assert crcs[i]["verdict"].tolist() == want[i].tolist(), (i, len(s), hdrs[i]["type"].tolist(), want[i].tolist())
    return want


@pytest.mark.parametrize("kind", list(KINDS))
def test_built_packets_whole_damaged_and_truncated(pkg, po, synth, kind):
    build, lengths, ph_syms, fec = KINDS[kind]
    rng = np.random.default_rng(sorted(KINDS).index(kind))
    packets, whole = [], []
    for n in lengths:
        for clk6 in (0, 21, 37, 63):                           # CLK1-6 below and above 32 (FHS retries 32 .. 63)
            clk = clk6 | (int(rng.integers(0, 1 << 20)) << 6)
            bits = build(synth, clk, n, rng)
            s = np.concatenate([bits, rng.integers(0, 2, 40, dtype=np.uint8)])       # noise behind the packet
            whole.append((len(packets), clk6))
            packets.append(s)
            if len(bits) > 126:
                one, two = s.copy(), s.copy()
                one[int(rng.integers(126, len(bits)))] ^= 1                               # one flipped payload symbol
                cw = 126 + 15 * int(rng.integers(0, max(1, (len(bits) - 126) // 15)))     # two flipped in one codeword
                a, b = rng.choice(min(15, len(bits) - cw), 2, replace=False)
                two[cw + a] ^= 1
                two[cw + b] ^= 1
                packets += [one, two]
            # where a guard changes its answer: no payload, the payload header's last symbol +-1, the body's last symbol +-1,
            # and (FEC types) the length the reference compares the DATA bit count with
            data_bits = (len(bits) - 126) * 2 // 3 if fec else len(bits) - 126
            cuts = {126, 126 + ph_syms - 1, 126 + ph_syms, 126 + ph_syms + 1, len(bits) - 1, len(bits), len(bits) + 1,
                    126 + data_bits - 1, 126 + data_bits}
            packets += [s[:c] for c in sorted(cuts) if 72 < c <= len(s)]
    for to_header in (72, 68):
        want = _compare(pkg, po, packets, to_header)
        # (on the oracle's side, so that a sweep of constants cannot pass) the true clock confirms the CRC; POLL has none
        for i, clk6 in whole:
            assert want[i][clk6] == {"POLL": 1, "FHS": 1000}.get(kind, 10)


def test_random_streams_reach_every_type(pkg, po, synth):
    """3000 random symbols: under the 64 clocks a random header takes every type (DV, HV1, EV3 / EV4 / EV5, AUX1, the refuted
    branches).  A random codeword passes the (15,10) check one time in five, so a third of the streams carry FEC-2/3-encoded random
    data from the payload's first symbol or from the DV data field on: the EV4, DM and DV parsers then run deep."""
    rng = np.random.default_rng(5)
    packets = []
    for k in range(300):
        s = rng.integers(0, 2, 3000, dtype=np.uint8)
        if k % 3 == 1:
            at = 126 if k % 2 else 206
            s[at:] = synth.fec23_encode(rng.integers(0, 2, 1920, dtype=np.uint8))[:3000 - at]
        if k % 3:
            s[72:126] = np.repeat(rng.integers(0, 2, 18, dtype=np.uint8), 3)          # a clean header: fec13_ok certain
        packets.append(s)
    want = _compare(pkg, po, packets, 72)
    assert {-1, 0, 1}.issubset(set(want.ravel().tolist()))


@pytest.mark.parametrize("eager_cap", [None, "3"])
def test_through_a_handle(pkg, po, synth, monkeypatch, eager_cap):
    """poll_payloads on a small hopping capture: the oracle's verdicts for the polled symbols, `length` as defined; hits, headers
    and symbols are those of a handle without the flag -- also where the records leave by the spill path (BTGPU_EAGER_CAP)."""
    fs, fc = 8e6, 2476.5e6
    iq, _ = _capture(synth, fs, fc)
    if eager_cap:
        monkeypatch.setenv("BTGPU_EAGER_CAP", eager_cap)
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, flags=pkg.FLAG_HEADERS | pkg.FLAG_LE, max_batch_slots=16)
    blk.push(iq)
    with pytest.raises(pkg.BtgpuError) as e:
        blk.poll_payloads()
    assert e.value.code == pkg.EUNSUPPORTED
    base = blk.poll_headers(sym_cap=3840)
    blk.close()
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, flags=pkg.FLAG_PAYLOAD_SWEEP | pkg.FLAG_LE, max_batch_slots=16)
    blk.push(iq)
    hits, hdrs, crcs, syms, lens = blk.poll_payloads(sym_cap=3840)
    blk.close()
    assert len(hits) > 8
    for a, b in zip((hits, hdrs, syms, lens), base):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    confirmed = 0
    for h, hd, cr, s, n in zip(hits, hdrs, crcs, syms, lens):
        assert cr["length"] == max(0, min(int(h["nsym"]), 3840 - int(h["offset"]))) == n
        want = [-1] * 64
        if h["kind"] == pkg.KIND_AC and hd["fec13_ok"]:
            want = [po.crc_check(s[:n], c, int(hd["type"][c]), int(hd["uap"][c])) for c in range(64)]
            confirmed += 10 in want
        assert cr["verdict"].tolist() == want
    assert confirmed > 4


def test_btrx_amd_prints_the_same_with_the_sweep(synth, tmp_path):
    """btrx_amd -S with BTGPU_PAYLOAD_SWEEP=1 (crc_check served from the GPU's verdicts): character for character what it prints
    without."""
    fs, fc = 8e6, 2476.5e6
    iq, _ = _capture(synth, fs, fc)
    path = tmp_path / "hop.cfile"
    iq.astype(np.complex64).tofile(path)
    btrx = os.path.join(ROOT, "gr-bluetooth_amd", "host", "btrx_amd")
    cmd = [btrx, "-f", "2476.5M", "-r", "8M", "-i", str(path), "-S"]
    env = {k: v for k, v in os.environ.items() if k != "BTGPU_PAYLOAD_SWEEP"}
    off = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120, check=True).stdout
    on = subprocess.run(cmd, env=dict(env, BTGPU_PAYLOAD_SWEEP="1"), capture_output=True, text=True, timeout=120, check=True).stdout
    assert "Correct CRC!" in off
    assert on == off
