"""The window kernel's staging from the tile-blocked stream dcol[tile][80][25] (WinLayoutTiled, kernels.hip.h), compiled for the
HOST in a translation unit of its own (tests/emu_dcol_window.cc) and run under the HIP emulator of tests/emu: the 100-bin bank
writes both layouts of the demodulated stream, window_kernel runs once on each, and everything it leaves -- window lengths,
hits, continuation records, packed symbols -- must be the same bytes.  No GPU: staging index errors are found here."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
EMU = os.path.join(TESTS, "emu")
SRC = os.path.join(ROOT, "gr-bluetooth_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("emu_dcol") / "libemu_dcol_window.so")
    cxx = os.environ.get("CXX", "/opt/rocm/lib/llvm/bin/clang++")
    if not os.path.exists(cxx):
        cxx = "c++"
    subprocess.check_call([cxx, "-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                           "-I" + EMU, "-I" + SRC, "-I" + os.path.join(ROOT, "include"), "-I" + TESTS, "-shared", "-o", out,
                           os.path.join(TESTS, "emu_dcol_window.cc"), os.path.join(EMU, "emu.cc"),
                           os.path.join(SRC, "design.cc"), os.path.join(SRC, "design_fast.cc")])
    L = ctypes.CDLL(out)
    L.emu_dcol_window_ab.restype = ctypes.c_int
    L.emu_dcol_window_ab.argtypes = [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_float),
                                     ctypes.c_longlong, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    return L


@pytest.mark.parametrize("mode,le,S", [(0, 0, 4), (1, 1, 8)])
def test_window_kernel_from_dcol_equals_from_d(lib, po, synth, mode, le, S):
    """100 Msps, 79 channels.  multi_LAP, 4 slots: two workgroups of 3 slots, the second with one live slot.  multi_sniffer with LE,
    8 slots (its windows begin 3125 symbols back: window 6 is the first that holds the capture).  G = 1250 (S - 1) + ddc_out is
    no multiple of 25 in either: the last tile is a partial one, its rows past the stream are set to NaN.  A negative return
    names what differs (emu_dcol_window.cc)."""
    fs, fc = 100e6, 2441e6
    iq, _ = synth.make_capture(fs, fc, S, laps=(0x24D952, 0x4831DD, 0x9E8B33), seed=5, snr_db=25, occupancy=0.9)
    H = po.Oracle(fs, fc, 10.0, mode).history
    x = np.concatenate([np.zeros(H - 1, np.complex64), iq.astype(np.complex64)])
    xf = np.ascontiguousarray(x).view(np.float32)
    counts = (ctypes.c_int * 2)()
    n = lib.emu_dcol_window_ab(fs, fc, mode, le, 10.0, xf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), len(x), S, counts)
    assert n >= 0, "the two staging forms differ (code %d; hits %d, continuation records %d)" % (n, counts[0], counts[1])
    assert n > 0 and counts[1] > 0, "the capture gave the kernel nothing to find: %d hits, %d continuation records" % (counts[0], counts[1])
