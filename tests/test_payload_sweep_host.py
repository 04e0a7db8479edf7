"""Host side of the payload sweep (no GPU): classic_packet serves crc_check from a btgpu_crc_sweep only where that was computed
on exactly the symbols it was handed (host/classic.cc), and the flag's rule in btgpu_design_query / btgpu_create."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gr-bluetooth_amd", "libgnuradio-bluetooth-amd.so")


@pytest.fixture(scope="module")
def swept(pkg):
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "gr-bluetooth_amd", "host")])
    import torch  # noqa: F401  (libbtgpu's HIP runtime: the one torch bundles)
    L = ctypes.CDLL(LIB)
    L.bt_host_crc_check_swept.restype = ctypes.c_int
    L.bt_host_crc_check_swept.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]

    def call(s, clock, hdr, crc):
        return L.bt_host_crc_check_swept(np.ascontiguousarray(s, np.uint8).tobytes(), len(s), clock, hdr.ctypes.data, crc.ctypes.data)
    return call


def _sweeps(pkg, po, s):
    hdr, crc = np.zeros(1, pkg.HEADER_DTYPE), np.zeros(1, pkg.CRC_SWEEP_DTYPE)
    tc = [po.try_clock(s, c) for c in range(64)]
    hdr["uap"][0], hdr["type"][0], hdr["fec13_ok"][0] = [t[0] for t in tc], [t[1] for t in tc], 1
    crc["verdict"][0] = [po.crc_check(s, c, tc[c][1], tc[c][0]) for c in range(64)]
    crc["length"][0] = len(s)
    return hdr, crc


def test_crc_check_is_served_from_a_sweep_of_the_same_symbols_only(pkg, po, synth, swept):
    clk = 0x1234567
    s = synth.classic_dm1_bits(0x4831DD, 0x6B, clk, b"payload sweep")
    hdr, crc = _sweeps(pkg, po, s)
    want = crc["verdict"][0].copy()
    assert want[clk & 63] == 10
    # a mark the parsers cannot produce: what comes back is the sweep's entry, not a computation
    crc["verdict"][0] = want + 7
    assert [swept(s, c, hdr, crc) for c in range(64)] == (want + 7).tolist()
    crc["verdict"][0][5] = -1                                  # not computed for this clock: the parsers answer
    assert swept(s, 5, hdr, crc) == want[5]
    crc["length"][0] = len(s) - 1                              # computed on another symbol count: ignored throughout
    assert [swept(s, c, hdr, crc) for c in range(64)] == want.tolist()
    assert [swept(s[:-1], c, hdr, crc) for c in (0, clk & 63)] == [want[0] + 7, want[clk & 63] + 7]
    crc["length"][0], hdr["fec13_ok"][0] = len(s), 0           # try_clock fails: type and UAP stay 0, crc_check gives 1
    assert swept(s, clk & 63, hdr, crc) == 1


def test_the_flag_is_for_the_sniffer_mode(pkg):
    flags = pkg.FLAG_PAYLOAD_SWEEP
    assert flags == 0x2000
    assert pkg.design_query(8e6, 2476.5e6, 10.0, mode=pkg.MODE_SNIFFER, flags=flags).history > 0
    with pytest.raises(pkg.BtgpuError) as e:
        pkg.design_query(8e6, 2476.5e6, 10.0, mode=pkg.MODE_LAP, flags=flags)
    assert e.value.code == pkg.EUNSUPPORTED
    # btgpu_create refuses it by the same rule, before it looks for a device
    cfg, h = pkg.make_config(8e6, 2476.5e6, 10.0, pkg.MODE_LAP, flags=flags), ctypes.c_void_p()
    assert pkg.lib().btgpu_create(ctypes.byref(cfg), ctypes.byref(h)) == pkg.EUNSUPPORTED and not h.value
