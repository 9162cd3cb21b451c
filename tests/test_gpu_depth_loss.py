"""The depth-regularisation term on the GPU (csrc/loss.hip depth_l1_kernel /
depth_l1_reduce_kernel, `_C.depth_l1_loss`, `losses.depth_l1_loss`):

    out1[0] = mean over H W of |(x - t) m|         grad = weight * sgn * m / (H W)

The value against a float64 torch reference (1e-5); the gradient bit for bit
against float32 ``weight * sgn * m / N`` evaluated in that order, ``sgn`` decided
by comparing x with t and taking the sign of m -- exactly 0 where the target
was copied from the input; two calls give the same bits (fixed-order
reduction); the autograd wrapper scales the saved gradient by the incoming one.

Shapes: one pixel; a 17 x 33 map (one workgroup, ragged); 130 x 250 (127
workgroups, the last one ragged, so the reduction kernel sums more partials
than one wave holds).
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (17, 33), (130, 250)]
MASKS = ["none", "zeros", "binary", "float"]


def _case(H, W, mask, seed=0):
    gen = torch.Generator().manual_seed(seed + 131 * H + W)
    x = torch.rand(1, H, W, generator=gen) * 2.0
    t = torch.rand(1, H, W, generator=gen) * 2.0
    copied = torch.rand(1, H, W, generator=gen) < 0.25  # sgn = 0 there
    if H * W == 1:
        copied[:] = False
    t = torch.where(copied, x, t)
    if mask == "none":
        m = None
    elif mask == "zeros":
        m = torch.zeros(1, H, W)
    elif mask == "binary":
        m = (torch.rand(1, H, W, generator=gen) < 0.6).float()
    else:
        m = torch.randn(1, H, W, generator=gen) * 3.0  # negatives included
        m[torch.rand(1, H, W, generator=gen) < 0.1] = 0.0
    return x, t, m, copied


def _expected(x, t, m, weight):
    """(float64 value, float32 gradient in the issue's order)."""
    N = x.numel()
    mm = torch.ones_like(x) if m is None else m
    value = float(((x.double() - t.double()) * mm.double()).abs().mean())
    f32 = torch.float32
    sgn = (x > t).to(f32) - (x < t).to(f32)
    sgn = sgn * ((mm > 0).to(f32) - (mm < 0).to(f32))
    grad = torch.tensor(weight, dtype=f32) * sgn * mm / torch.tensor(float(N), dtype=f32)
    return value, grad


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("mask", MASKS)
def test_value_and_gradient(H, W, mask):
    import gaussian_splatting_with_eye_tracking_amd._C as C
    weight = 0.37
    x, t, m, copied = _case(H, W, mask)
    want, want_grad = _expected(x, t, m, weight)
    xc, tc = x.cuda(), t.cuda()
    mc = None if m is None else m.cuda()
    out1, grad = C.depth_l1_loss(xc, tc, mc, weight)
    out1b, gradb = C.depth_l1_loss(xc, tc, mc, weight)
    torch.cuda.synchronize()
    assert out1.shape == (1,) and grad.shape == x.shape and grad.dtype == torch.float32
    got = float(out1[0])
    print(f"{H}x{W} mask={mask}: value {got!r} (float64 reference {want!r})")
    assert abs(got - want) < 1e-5
    g = grad.cpu()
    away = ~copied
    assert torch.equal(g.view(torch.int32)[away], want_grad.view(torch.int32)[away])  # bit for bit
    assert bool((g[copied] == 0).all())
    if mask == "zeros":
        assert got == 0.0 and bool((g == 0).all())
    # the same bits on a second call
    assert torch.equal(out1.view(torch.int32), out1b.view(torch.int32))
    assert torch.equal(grad.view(torch.int32), gradb.view(torch.int32))
    # an empty mask tensor means ones too
    if mask == "none":
        out1e, grade = C.depth_l1_loss(xc, tc, torch.empty(0, device="cuda"), weight)
        assert torch.equal(out1e, out1) and torch.equal(grade, grad)


def test_sign_comes_from_the_comparison_not_from_a_rounded_difference():
    """Inputs one denormal apart: the float32 difference is a denormal (zero
    once flushed), the comparison still says which is larger."""
    import gaussian_splatting_with_eye_tracking_amd._C as C
    tiny = np.float32(1e-45)  # the smallest denormal
    x = torch.tensor([[tiny, 0.0, 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))]], dtype=torch.float32)
    t = torch.tensor([[0.0, tiny, np.nextafter(np.float32(1.0), np.float32(2.0)), 1.0]], dtype=torch.float32)
    m = torch.tensor([[1.0, 1.0, -2.0, -2.0]], dtype=torch.float32)
    out1, grad = C.depth_l1_loss(x.cuda(), t.cuda(), m.cuda(), 1.0)
    want = torch.tensor([[1.0, -1.0, -2.0, 2.0]]) / 4.0  # sign(x - t) |m| / N
    assert torch.equal(grad.cpu(), want)
    assert torch.equal(grad.cpu(), _expected(x, t, m, 1.0)[1])
    assert abs(float(out1[0]) - float(((x.double() - t.double()) * m.double()).abs().mean())) < 1e-5


def test_autograd_wrapper_scales_by_the_incoming_gradient():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    from gaussian_splatting_with_eye_tracking_amd import losses
    H, W = 17, 33
    x, t, m, _ = _case(H, W, "float", seed=5)
    weight = 0.25
    out1, grad = C.depth_l1_loss(x.cuda(), t.cuda(), m.cuda(), weight)
    xr = x.cuda().requires_grad_(True)
    tr, mr = t.cuda().requires_grad_(True), m.cuda().requires_grad_(True)
    loss = losses.depth_l1_loss(xr, tr, mr, weight=weight)
    assert loss.shape == () and float(loss) == pytest.approx(weight * float(out1[0]), rel=1e-6)
    (3.0 * loss).backward()
    assert torch.equal(xr.grad, grad * 3.0)
    assert tr.grad is None and mr.grad is None  # data: no gradient
    # defaults: no mask, weight 1; a [H, W] map is taken as well
    x2 = x[0].cuda().requires_grad_(True)
    l2 = losses.depth_l1_loss(x2, t[0].cuda())
    l2.backward()
    want, want_grad = _expected(x, t, None, 1.0)
    assert abs(float(l2) - want) < 1e-5
    assert x2.grad.shape == (H, W) and torch.equal(x2.grad.cpu(), want_grad[0])
    weighted, plain = losses.depth_l1_loss_terms(x.cuda(), t.cuda(), None, 0.5)
    assert float(weighted) == pytest.approx(0.5 * float(plain), rel=1e-6) and abs(float(plain) - want) < 1e-5


def test_operand_checks():
    import gaussian_splatting_with_eye_tracking_amd._C as C
    x = torch.rand(1, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="target"):
        C.depth_l1_loss(x, torch.rand(1, 8, 7, device="cuda"), None, 1.0)
    with pytest.raises(RuntimeError, match="mask"):
        C.depth_l1_loss(x, x.clone(), torch.rand(1, 4, 8, device="cuda"), 1.0)
    with pytest.raises(RuntimeError, match="target"):
        C.depth_l1_loss(x, x.cpu(), None, 1.0)
