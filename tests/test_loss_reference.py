"""tests/loss_reference.py on the CPU.

* separable_loss_and_grad against the oracle's 121-shift form at rtol 1e-11,
  values and every gradient element, on the five loss_pins.npz cases and on
  3 x 33 x 33.  The identical-images pin has no gradient to be relative to
  (the exact one is 0; both forms leave float64 rounding residue of terms
  that cancel): there both stay below 1e-12 of the largest abs_terms.
* float32_loss_and_grad is the same function: it meets the bar the kernel is
  held to on every case of the GPU edge tests.  The smallest constant it
  needs there is printed per case (pytest -s); BAR_ABS is four times the
  largest, see DESIGN.md section 6.
"""
import os

import numpy as np
import pytest

import loss_oracle as L
import loss_reference as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PINS = ["rand_3x37x53", "near_3x64x80", "same_3x16x16", "rand_1x20x30", "tiny_3x7x5"]


def _pin_inputs(name):
    if name == "edge_3x33x33":
        return R.make_inputs((3, 33, 33), "noise") + (0.2,)
    d = np.load(os.path.join(GOLD, "loss_pins.npz"))
    return d[name + "_img"], d[name + "_gt"], float(d["lambda_dssim"])


@pytest.mark.parametrize("name", PINS + ["edge_3x33x33"])
def test_separable_matches_the_121_shift_oracle(name):
    img, gt, lam = _pin_inputs(name)
    loss, l1, ssim, grad = L.loss_and_grad(img, gt, lam)
    s_loss, s_l1, s_ssim, s_grad, abs_terms = R.separable_loss_and_grad(img, gt, lam)
    for got, ref in ((s_loss, loss), (s_l1, l1), (s_ssim, ssim)):
        assert abs(got - ref) <= 1e-11 * abs(ref)
    assert s_grad.shape == grad.shape == abs_terms.shape and s_grad.dtype == np.float64
    assert np.all(abs_terms >= np.abs(s_grad) * (1 - 1e-6))  # (abs_terms leaves the 5e-8 window residual out)
    if np.abs(grad).max() < 1e-12:  # identical images: zero gradient
        assert max(np.abs(s_grad).max(), np.abs(grad).max()) <= 1e-12 * abs_terms.max()
        return
    err = np.abs(s_grad - grad)
    print(f"{name}: worst gradient error / (1e-11 |ref|) = {(err / (1e-11 * np.abs(grad))).max():.3f}")
    assert np.all(err <= 1e-11 * np.abs(grad))


def test_window_residual_is_the_float32_rounding_of_the_outer_product():
    E = R.window_residual()
    w2 = L.window_2d().astype(np.float64)
    assert np.abs(E).max() > 0.0 and np.all(np.abs(E) <= 2.0 ** -24 * w2)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_float32_yardstick_meets_the_bar(case):
    shape, content, lam = case
    img, gt = R.make_inputs(shape, content)
    assert img.shape == shape and img.dtype == gt.dtype == np.float32
    if content == "wide_range":
        assert img.min() < 0.0 and img.max() > 1.0
    ref = R.separable_loss_and_grad(img, gt, lam)
    f32 = R.float32_loss_and_grad(img, gt, lam)
    a = R.needed_abs(f32[3], ref[3])
    print(f"{R.case_id(case)}: float32 conv2d needs a = {a:.3e}; value errors "
          f"{abs(f32[0] - ref[0]):.1e} {abs(f32[1] - ref[1]):.1e} {abs(f32[2] - ref[2]):.1e}")
    assert R.bar_ratio(f32[3], ref[3]) <= 1.0
    assert abs(f32[1] - ref[1]) < 1e-5  # (loss and ssim: see the constant-block figures in DESIGN.md)
