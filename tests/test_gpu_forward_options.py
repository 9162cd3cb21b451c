"""The per-call forward options (gs_set_thread_option) as a forward sees them:
the one-shot forward-only hint is consumed by exactly one forward entry --
also by one that returns early at P == 0 -- and store_cov3d holds until set
again.  Observed on the buffers the forward returns: the header flag kHdrDrgb
(gs_layout.h) and the geometry buffer's optional tail (parse_buffers' "cov3D").

Everything goes through `_C` except the P == 0 forward: the binding returns
its empty result without calling the C entry when P == 0, so that one call is
made on gs_rasterizer_forward itself through ctypes (the same library and
thread, hence the same thread options as `_C`).
"""
import os
import re

import pytest

import gs_helpers as G
from capi_helpers import GsBuffer, lib as _lib

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _hdr_word(name):
    import gaussian_splatting_with_eye_tracking_amd as pkg
    with open(os.path.join(os.path.dirname(pkg.__file__), "csrc", "gs_layout.h")) as f:
        return int(re.search(r"\b%s\s*=\s*(\d+)" % name, f.read()).group(1))


def test_forward_options_are_consumed_once():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    P, W, H = 2000, 96, 80
    sc, cam = G.scene_and_camera(P, W, H, 0)
    s = G.torch_settings(cam)
    t = G.scene_tensors(sc)
    e = torch.Tensor([])
    drgb = _hdr_word("kHdrDrgb")

    def forward(colors=e):
        K, _c, _r, gb, bb, ib = G.native_forward(sc, cam, colors if colors.numel() else None, settings=s,
                                                 tensors=t)[2]
        return C.parse_buffers(gb, bb, ib, P, K, W, H, 16)

    try:
        assert int(forward()["hdr"][drgb]) == 1
        C.set_thread_option("fwd_no_grad", 1)
        assert int(forward()["hdr"][drgb]) == 0
        assert int(forward()["hdr"][drgb]) == 1
        # a forward entry that returns at once (P == 0) consumes the hint too
        C.set_thread_option("fwd_no_grad", 1)
        none = GsBuffer()  # (no resize callback: P == 0 asks for no buffer)
        rc = _lib().gs_rasterizer_forward(none, none, none, 0, 3, 16, None, W, H, None, None, None, None, None, 1.0,
                                          None, None, None, None, None, s.tanfovx, s.tanfovy, 0, None, None, 0, None)
        assert rc == 0
        assert int(forward()["hdr"][drgb]) == 1
        # store_cov3d (precomputed colours: no SH-derivative rows ask for the tail)
        cols = torch.rand(P, 3, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
        C.set_thread_option("store_cov3d", 1)
        assert "cov3D" in forward(cols)
        C.set_thread_option("store_cov3d", 0)
        assert "cov3D" not in forward(cols)
    finally:
        C.set_thread_option("fwd_no_grad", 0)
        C.set_thread_option("store_cov3d", 0)
