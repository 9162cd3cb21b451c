"""The C ABI through ctypes, as a host without the pybind module would bind it
(include/gsplat_amd.h): the library handle, gs_buffer
resize callbacks over torch byte tensors, and pointer / return-code helpers,
shared by the tests that call C entries directly."""
import ctypes
import os

VP = ctypes.c_void_p
I = ctypes.c_int
F = ctypes.c_float
RESIZE = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t)


class GsBuffer(ctypes.Structure):
    _fields_ = [("resize", RESIZE), ("ctx", ctypes.c_void_p)]


def lib():
    """libgsplat_amd.so with the argument types of the base forward / backward and the AMR forward set."""
    import gaussian_splatting_with_eye_tracking_amd as pkg
    lib = ctypes.CDLL(os.path.join(os.path.dirname(pkg.__file__), "libgsplat_amd.so"))
    fwd = [GsBuffer, GsBuffer, GsBuffer, I, I, I, VP, I, I, VP, VP, VP, VP, VP, F, VP, VP, VP, VP, VP, F, F, I]
    lib.gs_rasterizer_forward.argtypes = fwd + [VP, VP, I, VP]
    lib.gs_rasterizer_backward.argtypes = ([I, I, I, I, VP, I, I, VP, VP, VP, VP, F, VP, VP, VP, VP, VP, F, F, VP,
                                            VP, VP, VP, VP] + [VP] * 9 + [I, VP])
    lib.gs_amr_rasterizer_forward.argtypes = fwd + [I, VP, VP, VP, VP, VP, VP, I, I, VP]
    lib.gs_last_error.restype = ctypes.c_char_p
    for f in (lib.gs_rasterizer_forward, lib.gs_rasterizer_backward, lib.gs_amr_rasterizer_forward):
        f.restype = I
    return lib


class Buffers:
    """Caller-owned byte buffers behind gs_buffer callbacks (the reference's
    resizeFunctional, base/rasterize_points.cu:27-33): each resize allocates a
    torch uint8 device tensor and returns its pointer."""

    def __init__(self, device):
        self.t = {}
        self.cb = {}
        self.device = device

    def buf(self, key):
        import torch

        def _resize(_ctx, n):
            self.t[key] = torch.empty(max(int(n), 1), dtype=torch.uint8, device=self.device)
            return self.t[key].data_ptr()
        self.cb[key] = RESIZE(_resize)  # (kept alive as long as the buffers)
        return GsBuffer(self.cb[key], None)


def ptr(t):
    return VP(t.data_ptr()) if t is not None and t.numel() else VP(0)


def check(lib, rc, what):
    assert rc >= 0, f"{what}: {lib.gs_last_error().decode()}"
    return rc
