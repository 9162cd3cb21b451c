"""References for the fused L1 + D-SSIM loss (csrc/loss.hip) that are cheap
enough for whole images, and the inputs its edge tests share.  Test
infrastructure only.

* ``separable_loss_and_grad``: the float64 loss and analytic gradient of
  oracle/loss_oracle.py with the 11 x 11 window applied as two 1-D passes, so
  that a 3 x 1080 x 1920 reference costs seconds where the oracle's 121
  shifts cost the better part of a minute.  The reference's 2-D window is the
  *float32* outer product of the 1-D one, which no pair of 1-D passes
  reproduces below 5e-8; its rounding residual E = w2d - w (x) w (exact in
  float64, |E| <= 2^-24 w2d) is applied on top as one float32 11 x 11
  correlation, whose own error is 1e-7 of a 5e-8 term.  Pinned to the oracle
  at rtol 1e-11 by tests/test_loss_reference.py.
* ``float32_loss_and_grad``: the same loss in torch float32 on the CPU,
  conv2d(padding=5, groups=C) and autograd -- the arithmetic of the
  reference program.  Its only job is to be the yardstick for the constant
  of the element-wise bar (``bar_ratio`` below): what float32 conv2d needs, the
  kernel may need four times of.
"""
from __future__ import annotations

import numpy as np

import loss_oracle as L

RTOL = 1e-4  # relative part of the element-wise bar (the project's gradient tolerance)


# ------------------------------------------------------------- float64 ----
def _corr_sep(a: np.ndarray, w2d_residual=None) -> np.ndarray:
    """Per-plane 'same' correlation with zero padding of [..., H, W] float64
    planes: two 1-D passes with the float64 value of the float32 window, plus
    the 2-D window's rounding residual when given."""
    from concurrent.futures import ThreadPoolExecutor
    from scipy.ndimage import correlate1d
    g = L.window_1d().astype(np.float64)

    def one(p):
        return correlate1d(correlate1d(p, g, axis=-2, mode="constant", cval=0.0), g, axis=-1, mode="constant", cval=0.0)

    with ThreadPoolExecutor(8) as ex:  # (planes are independent; the filter releases the GIL)
        out = np.stack(list(ex.map(one, a.reshape(-1, *a.shape[-2:])))).reshape(a.shape)
    if w2d_residual is not None:
        import torch
        lead = a.shape[:-2]
        t = torch.from_numpy(np.ascontiguousarray(a, np.float32)).reshape(1, -1, *a.shape[-2:])
        k = torch.from_numpy(w2d_residual.astype(np.float32))[None, None].repeat(t.shape[1], 1, 1, 1)
        r = torch.nn.functional.conv2d(t, k, padding=L.WINDOW // 2, groups=t.shape[1])
        out = out + r.reshape(*lead, *a.shape[-2:]).numpy().astype(np.float64)
    return out


def window_residual() -> np.ndarray:
    """w2d - w (x) w in float64: what rounding the outer product to float32
    (utils/loss_utils.py:27-31) adds to the separable window."""
    g = L.window_1d().astype(np.float64)
    return L.window_2d().astype(np.float64) - np.outer(g, g)


def separable_loss_and_grad(img, gt, lam: float = 0.2):
    """(loss, l1, ssim, grad, abs_terms) in float64.  abs_terms[c, i, j] is
    the sum of the absolute values of the terms grad[c, i, j] is the sum of:
    the scale against which a float32 evaluation's rounding is to be read."""
    x = np.asarray(img, np.float64)
    y = np.asarray(gt, np.float64)
    n = x.size
    E = window_residual()
    mu1, mu2, e11, e22, e12 = _corr_sep(np.stack([x, y, x * x, y * y, x * y]), E)
    s11, s22, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A = 2 * mu1 * mu2 + L.C1
    B = 2 * s12 + L.C2
    Cd = mu1 * mu1 + mu2 * mu2 + L.C1
    D = s11 + s22 + L.C2
    m = A * B / (Cd * D)
    ssim = m.mean()
    l1 = np.abs(x - y).mean()
    loss = (1 - lam) * l1 + lam * (1 - ssim)
    c = -lam / n
    G = np.stack([c * ((2 * mu2 * B - 2 * mu2 * A) / (Cd * D) - m * (2 * mu1 / Cd - 2 * mu1 / D)),
                  c * (-m / D),
                  c * (2 * A / (Cd * D))])
    a1, a11, a12 = _corr_sep(G, E)
    l1_term = (1 - lam) * np.sign(x - y) / n
    grad = a1 + 2 * x * a11 + y * a12 + l1_term
    b1, b11, b12 = _corr_sep(np.abs(G))
    abs_terms = b1 + 2 * np.abs(x) * b11 + np.abs(y) * b12 + np.abs(l1_term)
    return float(loss), float(l1), float(ssim), grad, abs_terms


# ------------------------------------------------------------- float32 ----
def float32_loss_and_grad(img, gt, lam: float = 0.2):
    """(loss, l1, ssim, grad) as torch float32 on the CPU computes them."""
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(np.ascontiguousarray(img, np.float32)).clone().requires_grad_(True)
    y = torch.from_numpy(np.ascontiguousarray(gt, np.float32))
    C = x.shape[0]
    w1 = torch.from_numpy(L.window_1d()).unsqueeze(1)
    w = (w1 @ w1.t()).expand(C, 1, L.WINDOW, L.WINDOW).contiguous()
    pad = L.WINDOW // 2

    def blur(t):
        return F.conv2d(t.unsqueeze(0), w, padding=pad, groups=C).squeeze(0)

    mu1, mu2 = blur(x), blur(y)
    s11 = blur(x * x) - mu1 * mu1
    s22 = blur(y * y) - mu2 * mu2
    s12 = blur(x * y) - mu1 * mu2
    ssim = (((2 * mu1 * mu2 + L.C1) * (2 * s12 + L.C2)) /
            ((mu1 * mu1 + mu2 * mu2 + L.C1) * (s11 + s22 + L.C2))).mean()
    l1 = (x - y).abs().mean()
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    loss.backward()
    return float(loss.detach()), float(l1.detach()), float(ssim.detach()), x.grad.numpy()


# ------------------------------------------------------------- the bar ----
def needed_abs(g, r) -> float:
    """The smallest a with |g - r| <= RTOL |r| + a max|r| element-wise."""
    g = np.asarray(g, np.float64)
    scale = np.abs(r).max()
    if scale == 0.0:
        return 0.0 if not np.any(g) else float("inf")
    return float(np.maximum(np.abs(g - r) - RTOL * np.abs(r), 0.0).max() / scale)


# What float32_loss_and_grad needs, per case, is in DESIGN.md section 6 (the
# largest: 2.885e-5 at 3 x 289 x 321 with a constant block, where every
# pixel's E[x^2] - mu^2 is the same rounding residue of a flat image against
# C2 = 9e-4); four times that, because the kernel's three chained 11-tap
# passes round in another order than conv2d's 121-tap sums, and never below
# the project's 1e-6.
BAR_ABS = 1.16e-4


def bar_ratio(g, r, a: float = BAR_ABS) -> float:
    """max |g - r| / (RTOL |r| + a max|r|)."""
    g = np.asarray(g, np.float64)
    scale = np.abs(r).max()
    if scale == 0.0:
        return 0.0 if not np.any(g) else float("inf")
    return float((np.abs(g - r) / (RTOL * np.abs(r) + a * scale)).max())


# ------------------------------------------------------------ the cases ----
SHAPES = [(3, 1, 1), (1, 1, 97), (3, 32, 32), (3, 33, 33), (3, 64, 31), (3, 289, 321)]
EDGE_SHAPES = [(3, 33, 33), (3, 289, 321)]  # every content and every lambda runs on these two


def _block(H, W):
    """A 40 % block that crosses the 32-pixel tile boundaries where there are any."""
    bh, bw = max(1, int(round(H * 0.8))), max(1, int(round(W * 0.5)))
    r0, c0 = (H - bh) // 2, (W - bw) // 3
    return slice(r0, r0 + bh), slice(c0, c0 + bw)


def make_inputs(shape, content: str):
    """(img, gt) float32 [C, H, W] from a seed fixed by the shape and content."""
    C, H, W = shape
    rng = np.random.default_rng([C, H, W, sum(map(ord, content))])
    img = rng.uniform(0.0, 1.0, shape)
    gt = np.clip(img + rng.normal(0.0, 0.1, shape), 0.0, 1.0)
    rows, cols = _block(H, W)
    if content == "noise":
        pass
    elif content == "same_block":      # gt == img exactly: sign(x - y) = 0 there
        gt[:, rows, cols] = img[:, rows, cols]
    elif content == "const_block":     # flat in both: E[x^2] - mu^2 cancels to rounding against C2
        img[:, rows, cols] = 0.7
        gt[:, rows, cols] = 0.4
    elif content == "wide_range":      # rendered images are not clamped during training
        img = rng.uniform(-0.1, 1.3, shape)
        gt = rng.uniform(-0.1, 1.3, shape)
    else:
        raise ValueError(content)
    img, gt = img.astype(np.float32), gt.astype(np.float32)
    if content == "same_block":
        assert np.array_equal(img[:, rows, cols], gt[:, rows, cols])
    return img, gt


# (shape, content, lambda)
CASES = [(s, "noise", 0.2) for s in SHAPES]
CASES += [(s, c, 0.2) for s in EDGE_SHAPES for c in ("same_block", "const_block", "wide_range")]
CASES += [(s, "same_block", 1.0) for s in EDGE_SHAPES] + [(s, "same_block", 0.0) for s in EDGE_SHAPES]


def case_id(case) -> str:
    (C, H, W), content, lam = case
    return f"{C}x{H}x{W}-{content}-lam{lam:g}"
