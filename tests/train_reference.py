"""Float64 restatements of the training-step kernels' element-wise math
(csrc/train.hip), from float32 inputs, in plain numpy:

* the activations of scene/gaussian_model.py:93-113 -- ``exp`` for the
  scales, ``sigmoid`` for the opacities, ``r / max(|r|, 1e-12)`` for the
  rotations (F.normalize, eps 1e-12), ``cat(dc, rest)`` for the SH rows;
* their backward as torch autograd defines it (ExpBackward,
  SigmoidBackward, div + clamp_min + norm backward -- the norm term only
  where ``|r| >= 1e-12`` --, CatBackward), and for every backward element
  the magnitude ``A``: the sum of the absolute values of the terms the
  element is formed from.  Where terms cancel (the rotation's two terms) a
  float32 evaluation errs by a multiple of 2^-24 A, not of the result;
* the densification statistics of train.py:111-113 /
  scene/gaussian_model.py:405-407.

Written from the formulas, not from the kernels: tests/test_train_reference.py
pins every function to float64 torch.autograd on the CPU.
"""
from __future__ import annotations

import numpy as np

NORM_EPS = 1e-12  # torch.nn.functional.normalize's default eps


def _f64(a) -> np.ndarray:
    return np.asarray(a, np.float64)


def sigmoid(x) -> np.ndarray:
    """1 / (1 + exp(-x)) without overflow at either end."""
    x = _f64(x)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def one_minus_sigmoid(x) -> np.ndarray:
    """1 - sigmoid(x) = sigmoid(-x), formed without the cancellation."""
    return sigmoid(-_f64(x))


def _norm(r: np.ndarray) -> np.ndarray:
    return np.sqrt((r * r).sum(axis=1, keepdims=True))


def activate(dc, rest, opacity, scaling, rotation) -> dict:
    """dc [P, 1, 3], rest [P, M-1, 3], opacity [P, 1], scaling [P, 3],
    rotation [P, 4] -> shs [P, M, 3], opacities, scales, rotations."""
    dc, rest, r = _f64(dc), _f64(rest), _f64(rotation)
    P = dc.shape[0]
    shs = np.concatenate([dc.reshape(P, 1, 3), rest.reshape(P, -1, 3)], axis=1)
    return {"shs": shs, "opacities": sigmoid(opacity), "scales": np.exp(_f64(scaling)),
            "rotations": r / np.maximum(_norm(r), NORM_EPS)}


def activation_backward(d_shs, d_opac, d_scales, d_rot, d_means3D, opacity, scaling, rotation):
    """The cotangents of the rasterizer's inputs pulled back to the raw
    groups.  Returns (grads, magnitudes): two dicts over xyz, f_dc, f_rest,
    opacity, scaling, rotation."""
    d_shs, d_opac, d_scales = _f64(d_shs), _f64(d_opac), _f64(d_scales)
    g, r = _f64(d_rot), _f64(rotation)
    P = d_shs.shape[0]
    d_shs = d_shs.reshape(P, -1, 3)
    grads = {"xyz": _f64(d_means3D).copy(), "f_dc": d_shs[:, :1].copy(), "f_rest": d_shs[:, 1:].copy()}
    s = sigmoid(opacity)
    grads["opacity"] = d_opac * one_minus_sigmoid(opacity) * s
    grads["scaling"] = d_scales * np.exp(_f64(scaling))
    n = _norm(r)
    d = np.maximum(n, NORM_EPS)
    first = g / d
    live = n >= NORM_EPS  # clamp_min passes the gradient on only where it did not clamp
    dot = (g * r).sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        second = np.where(live, r * dot / (d * d * n), 0.0)
        second_abs = np.where(live, np.abs(r) * np.abs(g * r).sum(axis=1, keepdims=True) / (d * d * n), 0.0)
    grads["rotation"] = first - second
    mags = {k: np.abs(v) for k, v in grads.items() if k != "rotation"}  # one term each
    mags["rotation"] = np.abs(first) + second_abs
    return grads, mags


def densify_stats(radii, grad_means2D, accum, denom, max_radii):
    """train.py:111-113 + gaussian_model.py:405-407 on the visible
    (radii > 0) rows; accum / denom [P, 1], max_radii [P].  Returns the
    three updated arrays in float64."""
    radii = np.asarray(radii).reshape(-1)
    g = _f64(grad_means2D)[:, :2]
    vis = radii > 0
    accum, denom, max_radii = _f64(accum).copy(), _f64(denom).copy(), _f64(max_radii).copy()
    accum[vis] += np.sqrt((g[vis] * g[vis]).sum(axis=1, keepdims=True))
    denom[vis] += 1.0
    max_radii[vis] = np.maximum(max_radii[vis], radii[vis].astype(np.float64))
    return accum, denom, max_radii


def edge_rotations() -> np.ndarray:
    """Rotation rows at the corners of F.normalize: an exact zero, a norm
    below the clamp (1e-13), and norms of 1e-6 and 1e+6 (float32 squares stay
    finite and normal within 1e+-15)."""
    u = np.array([0.5, -0.5, 0.1, 0.7]) / np.linalg.norm([0.5, -0.5, 0.1, 0.7])
    return np.stack([np.zeros(4), 1e-13 * u, 1e-6 * u, 1e6 * u]).astype(np.float32)


EDGE_OPACITIES = (30.0, -30.0, 100.0, -100.0)


def raw_inputs(P: int, M: int, seed: int) -> dict:
    """Float32 raw groups and cotangents for P Gaussians with M SH
    coefficients: scaling in [-15, 5], opacity in [-12, 12] plus rows at
    +-30 and +-100, rotations of norm 0.5 .. 2 plus edge_rotations() -- the
    edge rows are placed from the end backwards as far as P allows."""
    rng = np.random.default_rng(seed)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    rot = rng.standard_normal((P, 4))
    rot *= rng.uniform(0.5, 2.0, (P, 1)) / np.linalg.norm(rot, axis=1, keepdims=True)
    rot = f32(rot)
    opacity = f32(rng.uniform(-12, 12, (P, 1)))
    edge = edge_rotations()
    for k in range(min(P - 1, len(edge))):
        rot[P - 1 - k] = edge[k]
    for k in range(min(P - 1, len(EDGE_OPACITIES))):
        opacity[P - 1 - k] = EDGE_OPACITIES[k]
    raw = {"xyz": f32(rng.standard_normal((P, 3))), "f_dc": f32(rng.standard_normal((P, 1, 3))),
           "f_rest": f32(rng.standard_normal((P, M - 1, 3))), "opacity": opacity,
           "scaling": f32(rng.uniform(-15, 5, (P, 3))), "rotation": rot}
    cot = {"d_shs": f32(rng.standard_normal((P, M, 3))), "d_opac": f32(rng.standard_normal((P, 1))),
           "d_scales": f32(rng.standard_normal((P, 3))), "d_rot": f32(rng.standard_normal((P, 4))),
           "d_means3D": f32(rng.standard_normal((P, 3)))}
    return {"raw": raw, "cot": cot}
