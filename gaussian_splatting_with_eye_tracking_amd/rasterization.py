"""Autograd wrapper of the base rasterizer -- the drop-in for
``submodules/diff-gaussian-rasterization/diff_gaussian_rasterization/__init__.py``.

Same public names, argument order, return values and error behaviour as the
reference (``base/.../__init__.py:21-221``):

* ``rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities,
  scales, rotations, cov3Ds_precomp, raster_settings)``;
* ``_RasterizeGaussians.forward -> (color [3,H,W], radii [P] int32)`` and a
  backward returning gradients in input order, ``means2D``'s gradient being
  dL/d(NDC xy) with a zero third column;
* ``GaussianRasterizationSettings`` (NamedTuple) and ``GaussianRasterizer``
  (nn.Module) with ``markVisible`` and the "exactly one of" checks raising
  ``Exception``.

The native calls go to the MI355X extension ``_C`` (C ABI underneath).
"""
from __future__ import annotations

from typing import NamedTuple

import torch
import torch.nn as nn

from . import _C


def cpu_deep_copy_tuple(input_tuple):
    return tuple(item.cpu().clone() if isinstance(item, torch.Tensor) else item for item in input_tuple)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings):
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                     cov3Ds_precomp, raster_settings)


def rasterize_gaussians_aux(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                            raster_settings):
    """``rasterize_gaussians`` plus the differentiable depth and alpha maps:
    ``(color [3,H,W], radii [P], depth [1,H,W], alpha [1,H,W])`` with
    ``depth = sum z_i alpha_i T_i`` (view-space z, no background term, NOT
    normalised: divide by ``alpha`` yourself) and ``alpha = sum alpha_i T_i``
    over the colour blend's contributors (INTEGRATION.md "Depth and alpha
    maps").  ``color`` and ``radii`` are the plain call's bits."""
    return _RasterizeGaussiansAux.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                        cov3Ds_precomp, raster_settings)


def rasterize_gaussians_invdepth(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                                 raster_settings):
    """``rasterize_gaussians`` plus the differentiable inverse-depth and alpha
    maps: ``(color [3,H,W], radii [P], invdepth [1,H,W], alpha [1,H,W])`` with
    ``invdepth = sum (1 / z_i) alpha_i T_i`` (view-space z, one correctly rounded
    float division, no background term, not normalised) and ``alpha = sum
    alpha_i T_i`` over the colour blend's contributors: the upstream
    rasterizer's third output, which its depth regularisation reads
    (INTEGRATION.md §4g).  ``color`` and ``radii`` are the plain call's bits,
    ``alpha`` is ``rasterize_gaussians_aux``'s."""
    return _RasterizeGaussiansInvDepth.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                                             cov3Ds_precomp, raster_settings)


def _call(fn, args, debug: bool, dump: str, what: str):
    """debug mode: snapshot the arguments and re-raise (base/.../__init__.py:83-90)."""
    if not debug:
        return fn(*args)
    cpu_args = cpu_deep_copy_tuple(args)
    try:
        return fn(*args)
    except Exception as ex:
        torch.save(cpu_args, dump)
        print(f"\nAn error occured in {what}. Please forward {dump} for debugging.")
        raise ex


def _hint_forward_only(tensors) -> bool:
    """No backward can follow this call (grad mode off, or no input requires a
    gradient): tell the next native forward, which then skips what only the
    backward reads (the SH-derivative rows).  Returns whether
    the one-shot hint was set; the caller clears it once the call is over
    (_clear_hint), so a forward that raised before consuming it cannot hand
    it to a later training forward."""
    if not (torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)):
        _C.set_thread_option("fwd_no_grad", 1)
        return True
    return False


def _clear_hint(hinted: bool) -> None:
    if hinted:
        _C.set_thread_option("fwd_no_grad", 0)


# Deterministic backward (INTEGRATION.md "Deterministic backward"): None
# follows torch.are_deterministic_algorithms_enabled() at each backward.
_deterministic = None


def set_deterministic(mode) -> None:
    """Choose the blend backward's summation: ``True`` -- the fixed-order one
    (ascending tile index, float64, one rounding: bit-reproducible), ``False``
    -- the default float atomics, ``None`` (the default) -- whatever
    ``torch.are_deterministic_algorithms_enabled()`` says when a backward
    runs.  The autograd wrappers apply the choice around their native call;
    ``True`` / ``False`` also set the calling thread's native flag
    (``_C.set_deterministic_backward``), which direct users of the ``_C``
    backward bindings -- ``training.py``'s native sequence -- run under
    (``None`` clears it).  The AMR backward has no deterministic form."""
    global _deterministic
    if mode is not None and not isinstance(mode, bool):
        raise ValueError(f"set_deterministic: mode must be None, True or False, not {mode!r}")
    _deterministic = mode
    _C.set_deterministic_backward(bool(mode))


def deterministic_requested() -> bool:
    """What a backward that starts now runs as (set_deterministic)."""
    return torch.are_deterministic_algorithms_enabled() if _deterministic is None else _deterministic


class _DeterministicScope:
    """The calling thread's native flag set to the requested mode for one
    native call, and put back afterwards."""

    def __enter__(self):
        self.prev = _C.get_deterministic_backward()
        _C.set_deterministic_backward(deterministic_requested())

    def __exit__(self, *exc):
        _C.set_deterministic_backward(self.prev)
        return False


def native_forward_args(settings, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
    """The positional arguments of ``_C.rasterize_gaussians`` / ``_aux`` /
    ``_invdepth``: the one place that knows their order."""
    s = settings
    return (s.bg, means3D, colors_precomp, opacities, scales, rotations, s.scale_modifier, cov3Ds_precomp,
            s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width, sh, s.sh_degree,
            s.campos, s.prefiltered, s.debug, _antialiasing(s))


def native_backward_args(settings, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                         radii, geomBuffer, binningBuffer, imgBuffer, num_rendered, grad_color, grad_maps=None):
    """The positional arguments of ``_C.rasterize_gaussians_backward`` / ``_lean``
    or, with ``grad_maps = (dL_ddepth, dL_dalpha)``, of ``_aux`` / ``_aux_lean``
    (``(dL_dinvdepth, dL_dalpha)``: of ``_invdepth`` / ``_invdepth_lean``).
    ``opacities``: the forward's input, read by the antialiased backward only."""
    s = settings
    return ((s.bg, means3D, radii, colors_precomp, scales, rotations, s.scale_modifier, cov3Ds_precomp,
             s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, grad_color) + tuple(grad_maps or ()) +
            (sh, s.sh_degree, s.campos, geomBuffer, num_rendered, binningBuffer, imgBuffer, s.debug, opacities,
             _antialiasing(s)))


class _RasterizeBase(torch.autograd.Function):
    """What _RasterizeGaussians, _RasterizeGaussiansAux and
    _RasterizeGaussiansInvDepth share: the one-shot
    forward-only hint around ``apply``, the native forward with what the
    backward needs saved, and the lean native backward with its gradients put
    into input order."""

    @classmethod
    def apply(cls, *args):
        hinted = _hint_forward_only(args[:8])
        try:
            return super().apply(*args)
        finally:
            _clear_hint(hinted)

    @staticmethod
    def native_forward(ctx, fn, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, s):
        """Returns ``fn``'s outputs between num_rendered and the three buffers:
        (color, radii) or (color, depth, alpha, radii)."""
        operands = (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        num_rendered, *outs, geomBuffer, binningBuffer, imgBuffer = _call(
            fn, native_forward_args(s, *operands), s.debug, "snapshot_fw.dump", "forward")
        ctx.raster_settings = s
        ctx.num_rendered = num_rendered
        ctx.save_for_backward(*operands, outs[-1], geomBuffer, binningBuffer, imgBuffer)
        # radii (int32) never carries a gradient: without this autograd fills a
        # zero int tensor of P elements for it on every backward (~6 us at 1M)
        ctx.set_materialize_grads(False)
        return outs

    @staticmethod
    def native_backward(ctx, grad_out_color, grad_maps=None, inverse=False):
        s = ctx.raster_settings
        fn = (_C.rasterize_gaussians_backward_lean if grad_maps is None else
              _C.rasterize_gaussians_backward_invdepth_lean if inverse else _C.rasterize_gaussians_backward_aux_lean)
        args = native_backward_args(s, *ctx.saved_tensors, ctx.num_rendered, grad_out_color, grad_maps)
        with _DeterministicScope():
            (grad_means2D, grad_colors_precomp, grad_opacities, grad_means3D, grad_cov3Ds_precomp, grad_sh,
             grad_scales, grad_rotations) = _call(fn, args, s.debug, "snapshot_bw.dump", "backward")
        return (grad_means3D, grad_means2D, grad_sh, grad_colors_precomp, grad_opacities, grad_scales,
                grad_rotations, grad_cov3Ds_precomp, None)


class _RasterizeGaussians(_RasterizeBase):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        color, radii = _RasterizeBase.native_forward(
            ctx, _C.rasterize_gaussians, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
            raster_settings)
        return color, radii

    @staticmethod
    def backward(ctx, grad_out_color, _):
        if grad_out_color is None:  # the image took no part in the loss
            return (None,) * 9
        return _RasterizeBase.native_backward(ctx, grad_out_color)


def _maps_forward(ctx, fn, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings):
    """The forward of the two classes with maps: ``fn`` is ``_C.rasterize_gaussians_aux``
    or ``_C.rasterize_gaussians_invdepth``."""
    color, depth, alpha, radii = _RasterizeBase.native_forward(
        ctx, fn, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, raster_settings)
    ctx.mark_non_differentiable(radii)
    return color, radii, depth, alpha


def _maps_backward(ctx, grad_out_color, grad_depth, grad_alpha, inverse):
    """Their backward (``grad_depth``: the depth map's cotangent, or with
    ``inverse`` the inverse-depth map's)."""
    if grad_out_color is None and grad_depth is None and grad_alpha is None:
        return (None,) * 9
    aux = grad_depth is not None or grad_alpha is not None
    if aux and deterministic_requested():
        who, what = (("rasterize_gaussians_invdepth", "inverse-depth") if inverse else
                     ("rasterize_gaussians_aux", "depth"))
        raise RuntimeError(
            f"{who}: the deterministic backward has no form that takes {what} / alpha "
            "cotangents (a deterministic aux backward is not built); call set_deterministic(False) or keep "
            f"the {what} and alpha maps out of the loss")
    if grad_out_color is None:  # (the native call takes H and W from it)
        s, means3D = ctx.raster_settings, ctx.saved_tensors[0]
        grad_out_color = torch.zeros((3, s.image_height, s.image_width), dtype=means3D.dtype,
                                     device=means3D.device)
    if not aux:
        return _RasterizeBase.native_backward(ctx, grad_out_color)
    none = grad_out_color.new_empty(0)
    return _RasterizeBase.native_backward(
        ctx, grad_out_color, (none if grad_depth is None else grad_depth,
                              none if grad_alpha is None else grad_alpha), inverse=inverse)


class _RasterizeGaussiansAux(_RasterizeBase):
    """_RasterizeGaussians with the depth and alpha maps as two more
    differentiable outputs.  A backward that got neither map's cotangent is
    the plain lean backward; one that got either has no deterministic form
    and raises under the deterministic mode rather than use atomics."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        return _maps_forward(ctx, _C.rasterize_gaussians_aux, means3D, sh, colors_precomp, opacities, scales,
                             rotations, cov3Ds_precomp, raster_settings)

    @staticmethod
    def backward(ctx, grad_out_color, _, grad_depth, grad_alpha):
        return _maps_backward(ctx, grad_out_color, grad_depth, grad_alpha, inverse=False)


class _RasterizeGaussiansInvDepth(_RasterizeBase):
    """_RasterizeGaussiansAux on the inverse-depth map ``sum (1 / z) alpha T``:
    the same rules for absent cotangents and under the deterministic mode."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings):
        return _maps_forward(ctx, _C.rasterize_gaussians_invdepth, means3D, sh, colors_precomp, opacities, scales,
                             rotations, cov3Ds_precomp, raster_settings)

    @staticmethod
    def backward(ctx, grad_out_color, _, grad_invdepth, grad_alpha):
        return _maps_backward(ctx, grad_out_color, grad_invdepth, grad_alpha, inverse=True)


class _ReferenceSettings(NamedTuple):
    """The reference's settings tuple (base/.../__init__.py:157-169)."""
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


class GaussianRasterizationSettings(_ReferenceSettings):
    """The reference's settings tuple plus ``antialiasing`` (an extension: the
    reference predates the upstream rasterizer's switch), given as a trailing
    positional or a keyword argument, default ``False``.  With it each Gaussian
    is blended with ``opacity * sqrt(max(0.000025, det S / det (S + 0.3 I)))``,
    ``S`` its 2D covariance before the 0.3-px dilation: the Mip-Splatting 2D
    filter.

    The tuple itself stays the reference's twelve fields (``_fields``, ``len``,
    unpacking and ``tuple(settings)`` are unchanged, so it still drops into code
    written for the reference); the switch is an attribute beside it, kept by
    ``_replace``.  Code that reads it uses ``getattr(s, "antialiasing", False)``,
    so the reference's own tuple class is accepted as well."""
    antialiasing = False

    def __new__(cls, *args, **kw):
        n = len(_ReferenceSettings._fields)
        aa = kw.pop("antialiasing", False)
        if len(args) == n + 1:
            if "antialiasing" in kw or aa is not False:
                raise TypeError("GaussianRasterizationSettings: antialiasing given twice")
            *args, aa = args
        self = super().__new__(cls, *args, **kw)
        self.antialiasing = bool(aa)
        return self

    def _replace(self, **kw):
        aa = kw.pop("antialiasing", self.antialiasing)
        out = super()._replace(**kw)
        out.antialiasing = bool(aa)
        return out

    def __repr__(self):
        return super().__repr__()[:-1] + f", antialiasing={self.antialiasing!r})"


def _antialiasing(settings) -> bool:
    return bool(getattr(settings, "antialiasing", False))


def _check_exactly_one(shs, colors_precomp, scales, rotations, cov3D_precomp):
    """base/.../__init__.py:191-195"""
    if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
        raise Exception('Please provide excatly one of either SHs or precomputed colors!')
    if ((scales is None or rotations is None) and cov3D_precomp is None) or \
            ((scales is not None or rotations is not None) and cov3D_precomp is not None):
        raise Exception('Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!')


def _or_empty(t):
    return torch.Tensor([]) if t is None else t


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
                cov3D_precomp=None, return_aux=False, return_invdepth=False):
        """The reference's ``(color, radii)``; with ``return_aux=True`` (an
        extension) ``(color, radii, depth, alpha)`` -- rasterize_gaussians_aux;
        with ``return_invdepth=True`` (an extension) ``(color, radii, invdepth,
        alpha)`` -- rasterize_gaussians_invdepth.  Not both."""
        if return_aux and return_invdepth:
            raise ValueError("GaussianRasterizer: return_aux and return_invdepth are two different calls; give one")
        _check_exactly_one(shs, colors_precomp, scales, rotations, cov3D_precomp)
        fn = (rasterize_gaussians_invdepth if return_invdepth else
              rasterize_gaussians_aux if return_aux else rasterize_gaussians)
        return fn(means3D, means2D, _or_empty(shs), _or_empty(colors_precomp), opacities, _or_empty(scales),
                  _or_empty(rotations), _or_empty(cov3D_precomp), self.raster_settings)
