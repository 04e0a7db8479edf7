"""le_sweep_kernel (csrc/le_sweep.hip.h): the dewhitened PDU header, the CRC-24 at the header's length and at every other length,
and the CRCInit a packet implies, field for field against a bit-at-a-time register written from the Core specification
(Vol 6 Part B 3.1.1: the CRC, 3.2: the whitening) in its own, unreflected form."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 3, 4, 5, 6, 37, 254, 255)      # around the five-byte lane chunks, their last lane, the 6-bit mask of the reference
INDICES = (0, 36, 37, 39)
ADV = 0x555555


def whitening(index, n):
    reg, out = [1] + [(index >> (5 - i)) & 1 for i in range(6)], []       # position 0 = 1, 1 .. 6 = the index, MSB first
    for _ in range(n):
        o = reg[6]
        out.append(o)
        reg = [o] + reg[:6]
        reg[4] ^= o
    return out


def crc_states(bits, init):
    """The register (bit p = position p) in front of every bit of `bits`, and behind the last."""
    reg, out = init, []
    for b in bits:
        out.append(reg)
        fb = (reg >> 23) ^ b
        reg = ((reg << 1) & 0xFFFFFF) ^ (0x00065B if fb else 0)           # x^10 + x^9 + x^6 + x^4 + x^3 + x + 1
    return out + [reg]


def crc_backwards(bits, reg):
    for b in reversed(bits):
        fb = reg & 1
        reg = ((reg ^ (0x00065B if fb else 0)) >> 1) | ((fb ^ b) << 23)
    return reg


def as_sent(reg):
    return sum(((reg >> (23 - k)) & 1) << k for k in range(24))           # position 23 first = bit 0


@functools.lru_cache(None)
def carried(d):
    """What changing the PDU's second byte by d adds to the register 0 .. 255 bytes behind it (the register is linear)."""
    return crc_states([(d >> k) & 1 for k in range(8)] + [0] * (8 * 255), 0)[8::8]


def reference(sym, index):
    """What btgpu_le_sweep defines, on the symbols from the preamble on."""
    length = min(len(sym), 3840)
    size = length - 40
    raw = [int(b) for b in sym[40:length]] + [0] * (8 * 262 - max(size, 0))
    pdu = [a ^ b for a, b in zip(raw, whitening(index, len(raw)))]
    word = lambda at, n: sum(pdu[at + k] << k for k in range(n))
    header = word(0, 16)
    states = crc_states(pdu[:8 * 258], ADV)
    # the CRC at payload length m - 2 is that of the PDU whose length byte reads m - 2
    hold = [m for m in range(2, 258) if 8 * m + 24 <= size
            and as_sent(states[8 * m] ^ carried((header >> 8) ^ (m - 2))[m - 2]) == word(8 * m, 24)]
    m = 2 + (header >> 8)
    rec = dict(header=header, length=length, crc_rx=word(8 * m, 24), match_len=hold[0] - 2 if hold else -1, verdict=-1, crc_init=0xFFFFFFFF)
    if 8 * m + 24 <= size:
        rec["verdict"] = int(m in hold)
        rec["crc_init"] = crc_backwards(pdu[:8 * m], as_sent(rec["crc_rx"]))       # (as_sent is its own inverse)
    return rec


def check(pkg, packets, indices):
    got = pkg.debug_le_sweep(packets, indices)
    want = [reference(p, i) for p, i in zip(packets, indices)]
    for g, w in zip(got, want):
        assert {k: int(g[k]) for k in w} == w
    return want


def test_the_two_registers_agree(synth):
    rng = np.random.default_rng(1)
    msg = [int(b) for b in rng.integers(0, 2, 8 * 39)]
    crc = synth.le_crc24(msg, 0x1A2B3C).tolist()
    assert [(as_sent(crc_states(msg, 0x1A2B3C)[-1]) >> k) & 1 for k in range(24)] == crc
    assert crc_states(msg + crc, 0x1A2B3C)[-1] == 0
    assert crc_backwards(msg, crc_states(msg, 0x1A2B3C)[-1]) == 0x1A2B3C
    other = msg[:8] + [(21 >> k) & 1 for k in range(8)] + msg[16:]         # the same PDU with 21 in its second byte
    d = 21 ^ sum(b << k for k, b in enumerate(msg[8:16]))
    assert crc_states(other, ADV)[-1] == crc_states(msg, ADV)[-1] ^ carried(d)[37]


@pytest.mark.parametrize("case", ["whole", "cut", "payload_bit", "length_bit", "data_channel"])
def test_built_packets(pkg, synth, case):
    rng = np.random.default_rng(5)
    packets, indices, inits = [], [], []
    for n in LENGTHS:
        for index in INDICES:
            init = int(rng.integers(1, 1 << 24)) if case == "data_channel" else ADV
            p = synth.le_advert_bits(index, rng, payload_bytes=n, crc=True, crc_init=init)
            if case == "cut":
                p = p[:-1]
            elif case == "payload_bit":
                p[40 + (16 + 4 * n if n else 0)] ^= 1                      # (an empty payload: a bit of the PDU type)
            elif case == "length_bit":
                p[40 + 8] ^= 1
            if case in ("payload_bit", "length_bit"):                      # noise behind the packet: a longer claim is still checked
                p = np.concatenate([p, rng.integers(0, 2, 40 + 8 * 260 - len(p), dtype=np.uint8)])
            packets.append(p), indices.append(index), inits.append(init)
    want = check(pkg, packets, indices)
    true_len = [n for n in LENGTHS for _ in INDICES]
    for w, n, init in zip(want, true_len, inits):
        if case == "whole":
            assert (w["verdict"], w["crc_init"], w["match_len"], w["header"] >> 8) == (1, ADV, n, n)
        elif case == "cut":
            assert (w["verdict"], w["crc_init"], w["match_len"]) == (-1, 0xFFFFFFFF, -1)
        elif case == "payload_bit":
            assert w["verdict"] == 0 and w["crc_init"] != ADV
        elif case == "length_bit":
            assert (w["verdict"], w["match_len"]) == (0, n)
        else:
            assert (w["verdict"], w["crc_init"]) == (0, init)


def test_random_symbols(pkg):
    rng = np.random.default_rng(7)
    check(pkg, list(rng.integers(0, 2, (256, 40 + 8 * 260), dtype=np.uint8)), rng.integers(0, 40, 256).tolist())


def test_through_a_handle(pkg, synth):
    """poll_le on a capture with CRC-bearing adverts on channel 39: every sweep equals the reference on the symbols the same call
    returned; the records are those of a handle without the flag."""
    fs, fc, slots = 8e6, 2476.5e6, 48
    iq, _ = synth.make_capture(fs, fc, slots, laps=(0x24D952, 0x4831DD), seed=3, snr_db=25, occupancy=0.3)
    rng = np.random.default_rng(11)
    assert synth.visible_channels(fs, fc)[1] >= 78
    for k in range(2, slots - 2, 4):
        synth.add_burst(iq, synth.le_advert_bits(39, rng, payload_bytes=int(rng.integers(6, 38)), crc=True), k * 5000 + 90, fs, fc, 78, rng)
    key = lambda hits: [(int(h["slot"]), int(h["channel"]), int(h["kind"]), int(h["offset"]), int(h["lap"])) for h in hits]
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, flags=pkg.FLAG_LE | pkg.FLAG_SYMBOLS, max_batch_slots=16)
    blk.push(iq)
    with pytest.raises(pkg.BtgpuError) as e:
        blk.poll_le()
    assert e.value.code == pkg.EUNSUPPORTED
    base = key(blk.poll_symbols()[0])
    blk.close()
    blk = pkg.multi_sniffer(fs, fc, 10.0, False, flags=pkg.FLAG_LE | pkg.FLAG_LE_SWEEP, max_batch_slots=16)
    blk.push(iq)
    hits, les, syms, lens = blk.poll_le(sym_cap=3840)
    blk.close()
    assert key(hits) == base
    good = 0
    for h, le, s, n in zip(hits, les, syms, lens):
        if h["kind"] == pkg.KIND_AA:
            ch = int(h["channel"]) // 2
            index = {0: 37, 12: 38, 39: 39}.get(ch, ch - 1 if ch < 12 else ch - 2)
            want = reference(s[:n], index)
            good += want["verdict"] == 1
        else:
            want = dict(header=0, verdict=-1, length=0, crc_rx=0, crc_init=0xFFFFFFFF, match_len=-1)
        assert {k: int(le[k]) for k in want} == want
    assert good >= 1 and any(h["kind"] == pkg.KIND_AC for h in hits)
