"""The complex int16 entries of the C ABI without a GPU: bound by the Python mirror, and loud on null arguments.
(btrx_amd needs a device for either input format: its `-s` against its float text is in tests/test_gpu_s16.py.)"""
import pytest

S16_ENTRIES = ["btgpu_work_s16", "btgpu_process_host_s16", "btgpu_process_device_s16"]


@pytest.mark.parametrize("name", S16_ENTRIES)
def test_s16_entry_is_bound(pkg, name):
    assert name in pkg.EXPORTS
    f = getattr(pkg.lib(), name)
    assert f.argtypes is not None and len(f.argtypes) == {"btgpu_work_s16": 4, "btgpu_process_host_s16": 6, "btgpu_process_device_s16": 7}[name]


def test_s16_null_handle_or_pointer_is_einval(pkg):
    import ctypes
    L = pkg.lib()
    buf = (ctypes.c_int16 * 8)()
    fake = ctypes.c_void_p(ctypes.addressof(buf))          # a non-null "handle" is never reached: the pointer check comes first
    assert L.btgpu_work_s16(None, buf, 4, None) == pkg.EINVAL
    assert L.btgpu_work_s16(fake, None, 4, None) == pkg.EINVAL
    assert L.btgpu_process_host_s16(None, buf, 4, 0, 0, 1) == pkg.EINVAL
    assert L.btgpu_process_host_s16(fake, None, 4, 0, 0, 1) == pkg.EINVAL
    assert L.btgpu_process_device_s16(None, fake, 4, 0, 0, 1, None) == pkg.EINVAL
    assert L.btgpu_process_device_s16(fake, None, 4, 0, 0, 1, None) == pkg.EINVAL
