"""The complex int8 entries of the C ABI without a GPU: exported by libbtgpu.so, bound by the Python mirror, declared in the
header, and loud on null arguments."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S8_ENTRIES = {"btgpu_work_s8": 4, "btgpu_process_host_s8": 6, "btgpu_process_device_s8": 7}


@pytest.mark.parametrize("name", sorted(S8_ENTRIES))
def test_s8_entry_is_exported_bound_and_declared(pkg, name):
    assert hasattr(ctypes.CDLL(os.path.join(ROOT, "gr-bluetooth_amd", "libbtgpu.so")), name)
    assert name in pkg.EXPORTS
    assert len(getattr(pkg.lib(), name).argtypes) == S8_ENTRIES[name]
    with open(os.path.join(ROOT, "include", "btgpu.h")) as f:
        assert "int %s(btgpu_handle *h, " % name in f.read()


def test_s8_null_handle_or_pointer_is_einval(pkg):
    L = pkg.lib()
    buf = (ctypes.c_int8 * 8)()
    fake = ctypes.c_void_p(ctypes.addressof(buf))          # a non-null "handle" is never reached: the pointer check comes first
    assert L.btgpu_work_s8(None, buf, 4, None) == pkg.EINVAL
    assert L.btgpu_work_s8(fake, None, 4, None) == pkg.EINVAL
    assert L.btgpu_process_host_s8(None, buf, 4, 0, 0, 1) == pkg.EINVAL
    assert L.btgpu_process_host_s8(fake, None, 4, 0, 0, 1) == pkg.EINVAL
    assert L.btgpu_process_device_s8(None, fake, 4, 0, 0, 1, None) == pkg.EINVAL
    assert L.btgpu_process_device_s8(fake, None, 4, 0, 0, 1, None) == pkg.EINVAL
