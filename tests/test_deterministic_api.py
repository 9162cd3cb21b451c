"""The deterministic backward's host-side surface (no GPU compute): the C
ABI's scratch size and exported entries (include/gsplat_amd.h), the torch
extension's thread-local flag, and the package-level ``set_deterministic``.
"""
import ctypes
import os
import threading

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsplat_amd.h")
LIB = os.path.join(ROOT, "gaussian_splatting_with_eye_tracking_amd", "libgsplat_amd.so")
ENTRIES = ("gs_backward_deterministic_scratch_bytes", "gs_rasterizer_backward_deterministic",
           "gs_rasterizer_backward_view_grads_deterministic")


def _scratch_bytes():
    lib = ctypes.CDLL(LIB)
    f = lib.gs_backward_deterministic_scratch_bytes
    f.argtypes = [ctypes.c_int, ctypes.c_int]
    f.restype = ctypes.c_size_t
    return f


def test_entries_declared_and_exported():
    lib = ctypes.CDLL(LIB)
    hdr = open(HDR).read()
    for n in ENTRIES:
        assert n + "(" in hdr, n
        assert hasattr(lib, n), n
    # additive: no layout moved
    lib.gs_abi_version.restype = ctypes.c_int
    assert lib.gs_abi_version() == 7


def test_scratch_bytes_monotone_zero_safe_aligned():
    f = _scratch_bytes()
    for P in (0, 1, 10_000):
        assert f(P, 0) == 0
        assert f(P, -1) == 0
    assert f(0, 0) == 0
    prev = 0
    for R in (1, 2, 7, 8, 63, 64, 65, 1000, 4_400_000, 50_000_000, 2**31 - 1):
        n = f(10_000, R)
        assert n % 256 == 0, R
        assert n >= 36 * R, R  # one row of nine floats per sorted instance
        assert n < 36 * R + 256, R
        assert n >= prev, R
        prev = n
    # the formula the documents give does not depend on P
    assert f(1, 12345) == f(5_000_000, 12345)


def test_short_or_null_scratch_is_refused_before_any_device_call():
    """R > 0 with a NULL or too small scratch: a negative return and a message,
    nothing launched (so no device pointer is ever looked at: none is valid here)."""
    lib = ctypes.CDLL(LIB)
    lib.gs_last_error.restype = ctypes.c_char_p
    VP, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.gs_rasterizer_backward_deterministic.argtypes = (
        [I, I, I, I, VP, I, I, VP, VP, VP, VP, F, VP, VP, VP, VP, VP, F, F, VP, VP, VP, VP, VP] + [VP] * 9 +
        [VP, ctypes.c_size_t, I, VP])
    lib.gs_rasterizer_backward_view_grads_deterministic.argtypes = (
        [I, I, VP, I, I, VP, VP, VP, VP, F, F, VP, VP, VP, VP, VP, VP, VP, ctypes.c_size_t, I, VP])
    need = _scratch_bytes()(100, 1000)
    z = VP(0)
    for scratch, nbytes, word in ((z, need, "NULL"), (VP(256), need - 1, str(need))):
        rc = lib.gs_rasterizer_backward_deterministic(
            100, 3, 16, 1000, z, 64, 64, z, z, z, z, F(1.0), z, z, z, z, z, F(1.0), F(1.0), z, z, z, z, z,
            z, z, z, z, z, z, z, z, z, scratch, nbytes, 0, z)
        assert rc < 0
        assert word in lib.gs_last_error().decode()
        rc = lib.gs_rasterizer_backward_view_grads_deterministic(
            100, 1000, z, 64, 64, z, z, z, z, F(1.0), F(1.0), z, z, z, z, z, z, scratch, nbytes, 0, z)
        assert rc < 0
        assert word in lib.gs_last_error().decode()


def test_native_flag_is_thread_local_and_persistent():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    assert C.get_deterministic_backward() is False
    C.set_deterministic_backward(True)
    try:
        assert C.get_deterministic_backward() is True
        seen = []
        th = threading.Thread(target=lambda: seen.append(C.get_deterministic_backward()))
        th.start()
        th.join()
        assert seen == [False]
        assert C.get_deterministic_backward() is True
    finally:
        C.set_deterministic_backward(False)
    assert C.backward_deterministic_scratch_bytes(5, 1000) == _scratch_bytes()(5, 1000)


def test_set_deterministic_accepts_only_none_true_false():
    import gaussian_splatting_with_eye_tracking_amd as pkg
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import rasterization as R
    assert "set_deterministic" in pkg.__all__
    for bad in (1, 0, "yes", "True", 1.0, [], object()):
        with pytest.raises(ValueError):
            pkg.set_deterministic(bad)
    try:
        pkg.set_deterministic(True)
        assert R.deterministic_requested() is True and C.get_deterministic_backward() is True
        pkg.set_deterministic(False)
        assert R.deterministic_requested() is False and C.get_deterministic_backward() is False
        pkg.set_deterministic(None)
        import torch
        assert R.deterministic_requested() == torch.are_deterministic_algorithms_enabled()
        assert C.get_deterministic_backward() is False
    finally:
        pkg.set_deterministic(None)


def test_dropin_packages_export_the_switch():
    import diff_gaussian_rasterization as base
    import diff_gaussian_rasterization_amr as amr
    import gaussian_splatting_with_eye_tracking_amd as pkg
    assert base.set_deterministic is pkg.set_deterministic
    assert amr.set_deterministic is pkg.set_deterministic
