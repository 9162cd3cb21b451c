"""The fused L1 + D-SSIM loss (csrc/loss.hip) at its edges, element by
element against the float64 reference of tests/loss_reference.py (pinned to
the 121-shift oracle by tests/test_loss_reference.py).

The bar on every gradient element is |g - r| <= 1e-4 |r| + a max|r|.  Its
constant cannot be derived -- where the images are flat the SSIM map's
E[x^2] - mu^2 cancels against C2 = 9e-4 -- so it is measured on the
reference's own float32 arithmetic (loss_reference.float32_loss_and_grad,
never on the kernel): a = loss_reference.BAR_ABS is four times the largest
constant that arithmetic needs over the cases below.  Loss, L1 and SSIM are
held to the project's 1e-5 absolute.

Shapes: one pixel; one row; exactly one 32 x 32 tile; one-pixel partial
tiles in both axes (33 x 33); a partial tile in x only (64 x 31); and
3 x 289 x 321 = 330 workgroups, the smallest comfortable shape at which
l1_ssim_reduce_kernel's i += 256 loop takes a second round, again with
one-pixel partial tiles on both edges.  Contents (on 33 x 33 and 289 x 321):
noise; a 40 % block where gt == img exactly (sgn = 0: the L1 part of the
gradient is exactly 0 there); a constant block in both images; values in
[-0.1, 1.3].  lambda = 0.2, 1 and 0; at 0 the gradient is
float32(1 / n) sign(x - y) bit for bit and loss == l1.

Bit-identity: a CHW permutation of an HWC tensor against its contiguous
copy; two calls on the same inputs; and a NaN planted in one channel leaves
the other channels' gradients unchanged (one workgroup reads one channel).

Every test prints its worst error-to-bound ratio (pytest -s).

Found by these tests and fixed: with float32 accumulation of the five
correlations the two constant-block cases missed the SSIM value (1.6e-5 at
3 x 33 x 33, 4.9e-5 at 3 x 289 x 321 against 1e-5; the float32 yardstick
misses by 2.0e-5 and 5.9e-5).  The kernel now accumulates them in float64;
DESIGN.md section 6 has the record.
"""
import functools

import numpy as np
import pytest

import loss_reference as R

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _kernel(img, gt, lam):
    """(out3 [loss, l1, ssim], grad) as numpy, straight from the binding."""
    from gaussian_splatting_with_eye_tracking_amd import _C
    x = img if isinstance(img, torch.Tensor) else torch.from_numpy(img).cuda()
    y = gt if isinstance(gt, torch.Tensor) else torch.from_numpy(gt).cuda()
    out3, grad = _C.l1_ssim_loss(x, y, float(lam))
    return out3.cpu().numpy(), grad.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(case):
    shape, content, lam = case
    img, gt = R.make_inputs(shape, content)
    ref = R.separable_loss_and_grad(img, gt, lam)
    for a in (img, gt, ref[3], ref[4]):
        a.setflags(write=False)
    return img, gt, ref


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_values_and_every_gradient_element(case):
    shape, content, lam = case
    img, gt, (loss, l1, ssim, grad, abs_terms) = _case(case)
    out3, g = _kernel(img, gt, lam)
    assert g.shape == shape and g.dtype == np.float32 and np.all(np.isfinite(g))
    ratio = R.bar_ratio(g, grad)
    worst = np.unravel_index(np.argmax(np.abs(g - grad)), shape)
    print(f"{R.case_id(case)}: gradient worst error / bar = {ratio:.3f}; worst element {worst}: error "
          f"{abs(g[worst] - grad[worst]):.2e} = {abs(g[worst] - grad[worst]) / abs_terms[worst]:.1e} of its terms; "
          f"value errors loss {abs(out3[0] - loss):.1e} l1 {abs(out3[1] - l1):.1e} ssim {abs(out3[2] - ssim):.1e}")
    assert ratio <= 1.0
    assert abs(out3[0] - loss) < 1e-5
    assert abs(out3[1] - l1) < 1e-5
    assert abs(out3[2] - ssim) < 1e-5
    n = img.size
    if lam == 0.0:  # (these cases have the gt == img block: the gradient is exactly 0 there)
        want = np.float32(1.0 / n) * np.sign(img - gt)
        rows, cols = R._block(*shape[1:])
        assert not np.any(want[:, rows, cols]) and np.count_nonzero(want) > 0
        assert np.array_equal(_bits(g), _bits(want))
        assert _bits(out3[0:1])[0] == _bits(out3[1:2])[0]  # loss == l1


@pytest.mark.parametrize("shape", R.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_permuted_view_gives_the_contiguous_bits(shape):
    img, gt = R.make_inputs(shape, "noise")
    hwc_x = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 2, 0))).cuda()
    hwc_y = torch.from_numpy(np.ascontiguousarray(gt.transpose(1, 2, 0))).cuda()
    vx, vy = hwc_x.permute(2, 0, 1), hwc_y.permute(2, 0, 1)
    assert not vx.is_contiguous() and tuple(vx.shape) == shape
    o_v, g_v = _kernel(vx, vy, 0.2)
    o_c, g_c = _kernel(vx.contiguous(), vy.contiguous(), 0.2)
    assert np.array_equal(_bits(o_v), _bits(o_c)) and np.array_equal(_bits(g_v), _bits(g_c))
    o_n, g_n = _kernel(img, gt, 0.2)
    assert np.array_equal(_bits(o_v), _bits(o_n)) and np.array_equal(_bits(g_v), _bits(g_n))


@pytest.mark.parametrize("shape", R.EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_two_calls_give_the_same_bits(shape):
    img, gt = R.make_inputs(shape, "wide_range")
    x, y = torch.from_numpy(img).cuda(), torch.from_numpy(gt).cuda()
    o1, g1 = _kernel(x, y, 0.2)
    o2, g2 = _kernel(x, y, 0.2)
    assert np.array_equal(_bits(o1), _bits(o2)) and np.array_equal(_bits(g1), _bits(g2))


def test_nan_in_one_channel_leaves_the_others_alone():
    shape = (3, 33, 33)
    img, gt = R.make_inputs(shape, "noise")
    _, g = _kernel(img, gt, 0.2)
    bad = img.copy()
    bad[1, 16, 31:33] = np.nan  # across the tile boundary in x
    _, gb = _kernel(bad, gt, 0.2)  # no exception
    for ch in (0, 2):
        assert np.array_equal(_bits(gb[ch]), _bits(g[ch]))
