"""CPU tests of the x4 up-sampling / subsampling entry points (main_class.cpp:32-33, 58-70 on the GPU): the C-ABI exports
them, the Python layer validates its arguments, and without a device nothing falls back to the CPU."""
import ctypes as C
import os

import numpy as np
import pytest

NEW_SYMBOLS = ["bbme_set_frames_host_x4", "bbme_set_frames_host_x4_async", "bbme_set_frames_device_x4",
               "bbme_subsampled_flow_device", "bbme_get_subsampled_flow_host"]


def test_x4_symbols_are_exported_and_bound(bbme):
    from blockbasedmotionestimation_amd import _capi
    lib = C.CDLL(_capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _capi.SIGNATURES, name
    L = _capi.lib()
    # a null context is refused before anything touches a device
    z = np.zeros(16, np.uint8)
    assert L.bbme_set_frames_host_x4(None, 0, z.ctypes.data, z.ctypes.data, 4) == _capi.ERR_INVALID
    assert L.bbme_set_frames_device_x4(None, 0, z.ctypes.data, z.ctypes.data, 4) == _capi.ERR_INVALID
    out = np.zeros(16, np.float32)
    assert L.bbme_get_subsampled_flow_host(None, 0, 4, out.ctypes.data) == _capi.ERR_INVALID
    assert L.bbme_subsampled_flow_device(None, 0, 4, out.ctypes.data, 4, None) == _capi.ERR_INVALID


def test_cli_still_prints_its_usage(bbme):
    import subprocess
    from blockbasedmotionestimation_amd import build as _build
    r = subprocess.run([_build.CLI], capture_output=True, text=True)
    assert r.returncode == 2 and "usage: bbme_cli" in r.stderr and "--no-upsample" in r.stderr


def test_upsample_factor_is_validated(bbme):
    z = np.zeros((40, 48), np.uint8)
    for bad in (0, 2, 3):
        with pytest.raises(bbme.BbmeError) as e:
            bbme.MF(z, z, [30, 30], [16, 16], upsample=bad)
        assert e.value.status == -1
        with pytest.raises(bbme.BbmeError) as e:
            bbme.MFBatch([(z, z)], [30, 30], [16, 16], upsample=bad)
        assert e.value.status == -1


def test_x4_mf_has_no_cpu_fallback_without_device(bbme):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    z = np.zeros((40, 48), np.uint8)
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MF(z, z, [30, 30], [16, 16], upsample=4)
    assert e.value.status == -5 and "no CPU fallback" in e.value.message
    with pytest.raises(bbme.BbmeError) as e:
        bbme.MFBatch([(z, z), (z, z)], [30, 30], [16, 16], upsample=4)
    assert e.value.status == -5
