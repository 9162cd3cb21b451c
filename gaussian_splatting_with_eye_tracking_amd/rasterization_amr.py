"""Autograd wrapper of the AMR / foveated rasterizer -- the drop-in for
``submodules/diff-gaussian-rasterization-amr/diff_gaussian_rasterization_amr/__init__.py``.

Public surface identical to the reference (``amr/.../__init__.py:21-367``):

* ``rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities,
  scales, rotations, cov3Ds_precomp, foveaStep, out_color_precomp,
  geomBuffer_precomp, binningBuffer_precomp, imageBuffer_precomp,
  interpolate_image, raster_settings)``;
* ``_RasterizeGaussians.apply(...) -> (color, radii, geomBuffer,
  binningBuffer, imgBuffer)`` -- imported directly by
  ``gaussian_renderer_amr/__init__.py:19``;
* ``GaussianRasterizer.forward(..., foveaStep=0, out_color_precomp=None,
  geomBuffer_precomp=None, binningBuffer_precomp=None,
  imageBuffer_precomp=None, interpolate_image=True)``.

foveaStep semantics (amr/cr/rasterizer_impl.cu:296-694): 0 = preprocess,
binning and per-tile AMR levels only (blank image); 1..4 = render round k of
every tile whose level reaches k, reusing the step-0 buffers (the image
buffer is updated in place); < 0 = render every round up to each tile's level
in one call (``render_once``).

The reference's AMR backward is unreachable (its autograd forward has 15
inputs/5 outputs while its backward takes 2 grads and returns 9, and its
kernel misindexes the 2x render grid -- SURVEY §8(a) row B-AMR).  Here the
backward works (an extension): each call's image is
differentiated through the pixels it rendered (see
_RasterizeGaussians.backward), so a 5-step foveated frame or a render_once
frame can be trained on.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _C
from .rasterization import GaussianRasterizationSettings, _check_exactly_one, _clear_hint, _hint_forward_only, _or_empty  # noqa: F401
from .rasterization import _DeterministicScope, set_deterministic  # noqa: F401


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        foveaStep, out_color_precomp, geomBuffer_precomp, binningBuffer_precomp,
                        imageBuffer_precomp, interpolate_image, raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, foveaStep, out_color_precomp, geomBuffer_precomp,
                                     binningBuffer_precomp, imageBuffer_precomp, interpolate_image, raster_settings)


class _RasterizeGaussians(torch.autograd.Function):
    @classmethod
    def apply(cls, *args):
        # the settings tuple is the base rasterizer's; its antialiasing switch has
        # no AMR form: refused rather than rendered without the filter
        if getattr(args[14], "antialiasing", False):
            raise NotImplementedError("the AMR (foveated) rasterizer has no antialiased form: use the base "
                                      "rasterizer, or build the settings with antialiasing=False")
        # the copies of the foveaStep >= 1 interpolation (the reference's racy
        # precomp-copy path) have no backward here: refuse at the call that
        # would record them (grad mode on, an input requiring grad), not at
        # loss.backward()
        if int(args[8]) > 0 and bool(args[13]) and torch.is_grad_enabled() and any(
                isinstance(a, torch.Tensor) and a.requires_grad for a in args[:8]):
            raise RuntimeError("the AMR backward differentiates interpolate_image only for render_once "
                               "(foveaStep < 0); run foveaStep >= 1 with interpolate_image=False or under "
                               "torch.no_grad()")
        hinted = int(args[8]) <= 0 and _hint_forward_only(args[:8])  # (the steps >= 1 run no preprocess)
        try:
            return super().apply(*args)
        finally:
            _clear_hint(hinted)

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, foveaStep,
                out_color_precomp, geomBuffer_precomp, binningBuffer_precomp, imageBuffer_precomp,
                interpolate_image, raster_settings):
        s = raster_settings
        num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = _C.amr_rasterize_gaussians(
            s.bg, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, sh, s.sh_degree,
            s.campos, s.prefiltered, int(foveaStep), out_color_precomp, geomBuffer_precomp, binningBuffer_precomp,
            imageBuffer_precomp, bool(interpolate_image), s.debug)
        ctx.num_rendered = num_rendered
        ctx.raster_settings = s
        ctx.fovea_step = int(foveaStep)
        ctx.interpolate = bool(interpolate_image)
        # steps >= 1 return zero radii (as the reference); the backward then
        # reads the radii the step-0 preprocess left in the geometry buffer
        ctx.save_for_backward(colors_precomp, means3D, scales, rotations, cov3Ds_precomp,
                              radii if int(foveaStep) < 0 else torch.empty(0, dtype=torch.int32, device=radii.device),
                              sh, geomBuffer, binningBuffer, imgBuffer)
        ctx.mark_non_differentiable(radii, geomBuffer, binningBuffer, imgBuffer)
        # no zero cotangents materialised for the radii and the byte buffers
        ctx.set_materialize_grads(False)
        return color, radii, geomBuffer, binningBuffer, imgBuffer

    @staticmethod
    def backward(ctx, grad_color, *_):
        """Extension beyond parity: the reference's AMR
        backward is unreachable (15 inputs / 2 grads in, 9 out), and its kernel
        misindexes the 2x render grid (SURVEY §8(a) B-AMR bwd).  Here the
        image of one AMR call is differentiated exactly: foveaStep k in 1..4
        renders round k of the tiles with level >= k, render_once (k < 0)
        every round <= level, through the interpolation copies when
        interpolate_image; the gradient flows only through the rendered
        pixels, with the 32-px tile lists the forward blended (same 8 outputs
        as diff_gaussian_rasterization's backward).  foveaStep 0 renders a
        blank image: no gradient.  Interpolation at foveaStep >= 1 (the
        reference's racy precomp-copy path) is not differentiated."""
        step = ctx.fovea_step
        nones = (None,) * 7
        if step == 0 or grad_color is None:
            return (None,) * 8 + nones
        if ctx.interpolate and step > 0:
            raise RuntimeError("the AMR backward differentiates interpolate_image only for render_once "
                               "(foveaStep < 0)")
        s = ctx.raster_settings
        (colors_precomp, means3D, scales, rotations, cov3Ds_precomp, radii, sh, geomBuffer, binningBuffer,
         imgBuffer) = ctx.saved_tensors
        # (the AMR blend backward keeps its float atomics: with determinism
        # requested the binding raises -- or warns, warn_only -- under
        # torch.use_deterministic_algorithms, as torch's own such ops do)
        with _DeterministicScope():
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = _C.amr_rasterize_gaussians_backward(
                s.bg, means3D, radii, colors_precomp, scales, rotations, s.scale_modifier, cov3Ds_precomp,
                s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, grad_color, sh, s.sh_degree, s.campos, geomBuffer,
                ctx.num_rendered, binningBuffer, imgBuffer, step, ctx.interpolate, s.debug)
        return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
                grad_rotations, grad_cov3Ds_precomp) + nones


def _empty_u8():
    return torch.Tensor([]).to(torch.uint8)


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions):
        with torch.no_grad():
            s = self.raster_settings
            visible = _C.mark_visible(positions, s.viewmatrix, s.projmatrix)
        return visible

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, foveaStep=int(0), out_color_precomp=None, geomBuffer_precomp=None,
                binningBuffer_precomp=None, imageBuffer_precomp=None, interpolate_image=True):
        _check_exactly_one(shs, colors_precomp, scales, rotations, cov3D_precomp)
        return rasterize_gaussians(
            means3D, means2D, _or_empty(shs), _or_empty(colors_precomp), opacities, _or_empty(scales),
            _or_empty(rotations), _or_empty(cov3D_precomp), foveaStep, _or_empty(out_color_precomp),
            _empty_u8() if geomBuffer_precomp is None else geomBuffer_precomp,
            _empty_u8() if binningBuffer_precomp is None else binningBuffer_precomp,
            _empty_u8() if imageBuffer_precomp is None else imageBuffer_precomp, interpolate_image,
            self.raster_settings)


# --------------------------------------------------------- 5-step driver ---
AMR_STEPS_1_TO_4 = 14  # include/gsplat_amd.h GSPLAT_AMD_AMR_STEPS_1_TO_4: foveaStep 1..4 in one launch
AMR_STEPS_1_TO_4_FILL = 15  # ... storing every pixel into an unfilled step-0 image (GSPLAT_AMD_AMR_STEPS_1_TO_4_FILL)
def render_steps(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                 raster_settings, interpolate_image: bool = False, fused: Optional[bool] = None,
                 starters=None, enders=None, after_step0=None, one_launch: Optional[bool] = None):
    """The rasterizer sequence of ``gaussian_renderer_amr.render``
    (gaussian_renderer_amr/__init__.py:126-594): foveaStep 0 (buffers and a
    zero image), then foveaStep 1..4 on step 0's buffers, the caller summing
    ``out_color_precomp = out_color_precomp + rendered_image_k`` (step 4
    with ``interpolate_image``, steps 1..3 without).  Operands as
    ``_RasterizeGaussians.apply`` (empty tensors for absent ones).  Returns
    (image, radii, geomBuffer, binningBuffer, imageBuffer): the reference's
    ``render`` image and step 0's radii.

    ``fused`` (default: whenever no autograd graph is recorded, step 4 does
    not interpolate and the library runs the default AMR variant -- the
    fused step exists for the region-list form only): steps 1..4 add the pixels they render straight into the
    running image (``_C.amr_accumulate_step``, gs_amr_accumulate_step) --
    the same fp32 adds, so the same bits -- instead of writing a full step
    image each that the caller then adds (four full-image reads and writes
    per frame).  ``fused=False`` is the literal apply-and-add sequence.
    ``one_launch`` (fused only; default: whenever no per-step events are
    asked for): steps 1..4 as ONE launch (GSPLAT_AMD_AMR_STEPS_1_TO_4_FILL)
    -- each (tile, quadrant) unit renders its rounds 1..min(level, 4) in
    turn, so the steps' tails overlap instead of each step waiting for its
    heaviest tile, and stores its whole quadrant into step 0's image, which
    is therefore not zero-filled first; same frame, final T, n_contrib,
    radii and level state as the four launches (each pixel belongs to one
    round).
    ``after_step0(imageBuffer)`` runs between step 0 and step 1 (e.g.
    apply_fovea_levels).  ``starters`` / ``enders``: CUDA events recorded
    around each step, as the reference's fps harness passes them."""
    s = raster_settings
    args = (means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
    grad = torch.is_grad_enabled() and any(isinstance(a, torch.Tensor) and a.requires_grad for a in args)
    if fused is None:
        fused = not grad and not interpolate_image and _C.get_tuning("amr_variant") == 4
    elif fused and (grad or interpolate_image):
        raise RuntimeError("render_steps(fused=True) is forward-only without interpolation: run it under "
                           "torch.no_grad() with interpolate_image=False")
    if one_launch is None:
        one_launch = fused and starters is None and enders is None
    elif one_launch and not fused:
        raise RuntimeError("render_steps(one_launch=True) needs the fused steps")
    e = torch.empty(0, device=means3D.device)
    u8 = torch.empty(0, dtype=torch.uint8, device=means3D.device)

    def mark(evs, k):
        if evs is not None:
            evs[k].record()

    mark(starters, 0)
    unfilled = one_launch and means3D.shape[0] > 0
    if unfilled:
        # step 0's zero image is never read before the one launch below stores
        # every pixel of it: skip the fill (one-shot option, consumed by this call)
        _C.set_thread_option("amr_step0_unfilled", 1)
    try:
        acc, radii, gb, bb, ib = _RasterizeGaussians.apply(*args, 0, e, u8, u8, u8, False, s)
    finally:
        if unfilled:
            _C.set_thread_option("amr_step0_unfilled", 0)  # (in case the call never reached the library)
    mark(enders, 0)
    if after_step0 is not None:
        after_step0(ib)
    if one_launch:
        _C.amr_accumulate_step(s.bg, colors_precomp, int(s.image_height), int(s.image_width),
                               int(means3D.shape[0]), AMR_STEPS_1_TO_4_FILL if unfilled else AMR_STEPS_1_TO_4,
                               acc, gb, bb, ib, bool(s.debug))
        return acc, radii, gb, bb, ib
    for k in range(1, 5):
        mark(starters, k)
        if fused:
            _C.amr_accumulate_step(s.bg, colors_precomp, int(s.image_height), int(s.image_width),
                                   int(means3D.shape[0]), k, acc, gb, bb, ib, bool(s.debug))
        else:
            c, _, gb, bb, ib = _RasterizeGaussians.apply(*args, k, acc, gb, bb, ib,
                                                          bool(interpolate_image) if k == 4 else False, s)
            acc = acc + c
        mark(enders, k)
    return acc, radii, gb, bb, ib


# ------------------------------------------------ fovea-driven levels (ext.) ---
def reference_foveae(width: int, height: int, centre: Optional[Tuple[float, float]] = None):
    """The fovea discs the reference builds and leaves unused
    (gaussian_renderer_amr/__init__.py:98-106): four centres (the image
    centre there; the tracked fovea centre here when given) and radii
    W/2, W/4, W/8, W/16."""
    c = (width / 2, height / 2) if centre is None else (float(centre[0]), float(centre[1]))
    return [c] * 4, [width / 2, width / 4, width / 8, width / 16]


def apply_fovea_levels(imageBuffer: torch.Tensor, width: int, height: int, centres: Sequence[Tuple[float, float]],
                       radii: Sequence[float], min_level: int = 1, replace: bool = False) -> None:
    """Extension beyond parity: implement the
    reference's TODO "if outside the current fovea, set to same as last step"
    (gaussian_renderer_amr/__init__.py:244) on the tile levels foveaStep 0
    left in ``imageBuffer`` (mutated in place, on the device): a tile keeps
    round k only while its rectangle meets foveae 1..k; ``replace`` makes the
    fovea alone decide the level (pure eccentricity foveation).  Call it
    between step 0 and steps 1..4; see csrc/amr.hip fovea_override_kernel."""
    flat = [float(v) for c in centres for v in c]
    _C.amr_fovea_levels(imageBuffer, int(width), int(height), flat, [float(r) for r in radii], int(min_level),
                        bool(replace))
    # the levels changed in place: a backward that saved this buffer before
    # the call must fail loudly rather than use the new levels
    torch.autograd.graph.increment_version(imageBuffer)
