"""tests/sparse_adam_reference.py pinned on the CPU: bit for bit to an
independently written torch float32 restatement in the shape of upstream's
SparseGaussianAdam (per group: ``param[vis]``, ``exp_avg[vis]``,
``exp_avg_sq[vis]``), and to the float64 evaluation within the bounds derived
in ``step_f64``'s docstring, edge rows included."""
import numpy as np
import pytest
import torch

import sparse_adam_reference as SR

BETAS = (0.9, 0.999)
EPS = 1e-15
LRS = [1.6e-4, 2.5e-3, 1.25e-4, 5e-2, 5e-3, 1e-3]


def _torch_step(p, g, m, v, seg_end, lr, step, radii, beta1, beta2, eps):
    """Upstream's optimiser loop over param groups with masked tensor ops
    (float32, every operation its own tensor op), the formula of its
    adamUpdate kernel.  The square root is taken in float64 and rounded to
    float32: that is the correctly rounded float32 root (53 >= 2 * 24 + 2
    bits, so the double rounding is innocuous), which torch.sqrt on a float32
    CPU tensor is not in every build (test_torch_float32_sqrt_... below
    shows the input at which the vectorised one is 1 ulp off)."""
    f32 = torch.float32
    p, g, m, v = (torch.from_numpy(np.array(a, dtype=np.float32, copy=True)) for a in (p, g, m, v))
    P = int(np.asarray(radii).size)
    vis = torch.from_numpy(np.asarray(radii).reshape(-1) > 0)
    b1, b2 = torch.tensor(beta1, dtype=f32), torch.tensor(beta2, dtype=f32)
    omb1, omb2 = torch.tensor(1.0, dtype=f32) - b1, torch.tensor(1.0, dtype=f32) - b2
    e32 = torch.tensor(eps, dtype=f32)
    lo = 0
    for end, lr_s, t in zip(seg_end, lr, step):
        n = end - lo
        if t > 0 and n > 0:
            param, grad = p[lo:end].view(P, n // P), g[lo:end].view(P, n // P)
            exp_avg, exp_avg_sq = m[lo:end].view(P, n // P), v[lo:end].view(P, n // P)
            gv = grad[vis]
            exp_avg[vis] = torch.add(torch.mul(exp_avg[vis], b1), torch.mul(gv, omb1))
            exp_avg_sq[vis] = torch.add(torch.mul(exp_avg_sq[vis], b2), torch.mul(torch.mul(gv, omb2), gv))
            num = torch.mul(exp_avg[vis], -torch.tensor(lr_s, dtype=f32))
            den = torch.add(torch.sqrt(exp_avg_sq[vis].double()).float(), e32)
            param[vis] = torch.add(param[vis], torch.div(num, den))
        lo = end
    return p.numpy(), m.numpy(), v.numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


CASES = [(1, 16), (2, 1), (65, 4), (257, 16)]


@pytest.mark.parametrize("P,M", CASES, ids=[f"P{p}-M{m}" for p, m in CASES])
def test_numpy_reference_is_the_torch_restatement_bit_for_bit(P, M):
    p, g, m, v, ends = SR.make_state(P, M, seed=P + M)
    steps = [1, 2, 3, 0, 5, 6]  # the opacity segment is inactive
    for name, radii in SR.masks(P).items():
        g_nan = g.copy()
        lo = 0
        for e in ends:  # gradients of invisible rows are never read
            w = (e - lo) // P
            g_nan[lo:e].reshape(P, w)[radii <= 0] = np.nan
            lo = e
        got = SR.step(p, g_nan, m, v, ends, LRS, steps, radii, *BETAS, EPS)
        want = _torch_step(p, g, m, v, ends, LRS, steps, radii, *BETAS, EPS)
        for a, b, what in zip(got, want, "pmv"):
            assert np.array_equal(_bits(a), _bits(b)), (name, what)
        assert not any(np.isnan(a).any() for a in got), name
        # invisible rows and the inactive segment keep their bits
        keep = np.ones(ends[-1], bool)
        lo = 0
        for e, t in zip(ends, steps):
            w = (e - lo) // P
            if t > 0:
                keep[lo:e].reshape(P, w)[radii > 0] = False
            lo = e
        for a, b in zip(got, (p, m, v)):
            assert np.array_equal(_bits(a)[keep], _bits(b)[keep]), name
        if name == "all":
            changed = _bits(got[1]) != _bits(m)
            assert changed[~keep].mean() > 0.5  # and the visible ones do move


@pytest.mark.parametrize("P,M", CASES, ids=[f"P{p}-M{m}" for p, m in CASES])
def test_numpy_reference_is_within_the_derived_bound_of_float64(P, M):
    p, g, m, v, ends = SR.make_state(P, M, seed=7 * P + M)
    steps = [1] * 6
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for name in ("all", "random50", "signed"):
        radii = SR.masks(P)[name]
        got = SR.step(p, g, m, v, ends, LRS, steps, radii, *BETAS, EPS)
        p64, m64, v64, bp, bm, bv = SR.step_f64(p, g, m, v, ends, LRS, steps, radii, *BETAS, EPS)
        for what, a, r, b in (("p", got[0], p64, bp), ("m", got[1], m64, bm), ("v", got[2], v64, bv)):
            err = np.abs(a.astype(np.float64) - r)
            assert np.all(err <= b), (name, what, float((err - b).max()))
            live = b > 0
            if live.any():
                worst[what] = max(worst[what], float((err[live] / b[live]).max()))
    print(f"sparse adam f32 vs f64, P={P} M={M}: worst error/bound {worst}")
    assert worst["m"] > 0.05 and worst["v"] > 0.05 and worst["p"] > 0.05  # the bounds are not vacuous


def test_torch_float32_sqrt_is_why_the_restatement_roots_in_float64():
    """v' = 6.50675691105107e-09 (a float32) has a root 0.5016 ulp above the
    lower float32 neighbour: the correctly rounded result is the upper one,
    which numpy and the float64 route give.  (torch.sqrt on the float32
    tensor may give either; it is not asserted.)"""
    x = np.float32(6.50675691105107e-09)
    lo, hi = np.float32(8.06644675321877e-05), np.float32(8.066447480814531e-05)
    assert np.nextafter(lo, np.float32(1)) == hi
    exact = np.sqrt(np.float64(x))
    assert abs(np.float64(hi) - exact) < abs(np.float64(lo) - exact)
    assert np.sqrt(x) == hi
    assert torch.sqrt(torch.tensor([float(x)], dtype=torch.float32).double()).float().item() == float(hi)


def test_edge_rows_by_hand():
    """g = 0 leaves m' = b1 m and v' = b2 v; with v = 0 too the quotient is
    (-lr m') / eps; a subnormal g squares to zero; a large g stays finite."""
    ends, lr, radii = [len(SR.EDGE_ROWS)], [1e-3], np.ones(1, np.int32)
    g, m, v = (np.array(c, np.float32) for c in zip(*SR.EDGE_ROWS))
    p = np.ones_like(g)
    p1, m1, v1 = SR.step(p, g, m, v, ends, lr, [1], radii, *BETAS, EPS)
    f = np.float32
    b1, b2 = f(BETAS[0]), f(BETAS[1])
    assert m1[0] == b1 * f(0.25) and v1[0] == b2 * f(0.5)
    assert v1[1] == 0 and p1[1] == f(1) + (-f(1e-3) * (b1 * f(0.125))) / f(EPS)
    assert m1[2] == 0 and v1[2] == 0 and p1[2] == 1  # 0 / eps
    assert g[3] != 0 and g[3] < np.finfo(np.float32).tiny and v1[3] == 0 and m1[3] != 0
    assert np.isfinite(p1).all() and np.isfinite(v1).all() and v1[6] > 1e32


def test_reference_refuses_partial_rows_and_bad_segment_counts():
    z = np.zeros(10, np.float32)
    with pytest.raises(ValueError):
        SR.step(z, z, z, z, [5, 10], [1e-3] * 2, [1, 1], np.ones(3, np.int32), *BETAS, EPS)
    with pytest.raises(ValueError):
        SR.step(z, z, z, z, list(range(1, 10)) + [10], [1e-3] * 10, [1] * 10, np.ones(1, np.int32), *BETAS, EPS)
