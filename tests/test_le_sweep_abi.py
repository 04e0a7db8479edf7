"""BTGPU_FLAG_LE_SWEEP at the C ABI, without a device: where the flag is refused, what the entry points say to null arguments,
and the size of the record."""
import ctypes

import pytest


@pytest.mark.parametrize("mode, flags", [("MODE_LAP", 0x8001), ("MODE_SNIFFER", 0x8000)])      # LAP mode with FLAG_LE; the sniffer without
def test_the_flag_needs_the_le_pass_of_the_sniffer(pkg, mode, flags):
    assert pkg.FLAG_LE_SWEEP == 0x8000 and pkg.FLAG_LE == 1
    assert pkg.design_query(8e6, 2476.5e6, 10.0, mode=pkg.MODE_SNIFFER, flags=pkg.FLAG_LE | pkg.FLAG_LE_SWEEP).history > 0
    with pytest.raises(pkg.BtgpuError) as e:
        pkg.design_query(8e6, 2476.5e6, 10.0, mode=getattr(pkg, mode), flags=flags)
    assert e.value.code == pkg.EUNSUPPORTED
    # btgpu_create refuses it by the same rule, before it looks for a device
    cfg, h = pkg.make_config(8e6, 2476.5e6, 10.0, getattr(pkg, mode), flags=flags), ctypes.c_void_p()
    assert pkg.lib().btgpu_create(ctypes.byref(cfg), ctypes.byref(h)) == pkg.EUNSUPPORTED and not h.value


def test_null_arguments_and_the_record(pkg):
    L = pkg.lib()
    assert L.btgpu_poll_le(None, None, None, None, 0, None, 0) == pkg.EINVAL
    assert L.btgpu_debug_le_sweep(None, None, None, 0, 1, -1, None) == pkg.EINVAL
    assert ctypes.sizeof(pkg.LeSweep) == 20 == pkg.LE_SWEEP_DTYPE.itemsize
