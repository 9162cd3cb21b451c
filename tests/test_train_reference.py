"""CPU checks of tests/train_reference.py: the float64 numpy restatement of
the activations, their backward and the densification statistics against
torch (float64, autograd on the CPU), so the reference the GPU kernels are
held to is pinned independently of the kernels' own formulas."""
import numpy as np
import pytest
import torch

import train_reference as TR

RTOL = 1e-12


def _t64(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=grad)


def _torch_activations(raw):
    t = {k: _t64(v) for k, v in raw.items()}
    out = {"shs": torch.cat((t["f_dc"], t["f_rest"]), dim=1), "opacities": torch.sigmoid(t["opacity"]),
           "scales": torch.exp(t["scaling"]), "rotations": torch.nn.functional.normalize(t["rotation"])}
    return t, out


@pytest.mark.parametrize("P,M,seed", [(1, 16, 0), (64, 4, 1), (67, 1, 2), (130, 16, 3)])
def test_activations_match_torch_float64(P, M, seed):
    case = TR.raw_inputs(P, M, seed)
    raw = case["raw"]
    ref = TR.activate(raw["f_dc"], raw["f_rest"], raw["opacity"], raw["scaling"], raw["rotation"])
    _, out = _torch_activations(raw)
    assert ref["shs"].shape == (P, M, 3)
    np.testing.assert_array_equal(ref["shs"], out["shs"].detach().numpy())
    for k in ("opacities", "scales", "rotations"):
        np.testing.assert_allclose(ref[k], out[k].detach().numpy(), rtol=RTOL, atol=0, err_msg=k)


@pytest.mark.parametrize("P,M,seed", [(1, 16, 0), (64, 4, 1), (67, 1, 2), (130, 16, 3)])
def test_activation_backward_matches_autograd_float64(P, M, seed):
    """rtol 1e-12 everywhere.  Two additions, both far below anything a
    float32 kernel is asked for: the rotation's two terms may cancel, so its
    bound also carries 1e-12 of the magnitude A; and float64 torch forms
    1 - sigmoid by subtraction, which is off by up to 2^-53 absolute where
    the sigmoid saturates (the restatement forms sigmoid(-x) instead), so the
    opacity carries 2^-52 |cotangent|."""
    case = TR.raw_inputs(P, M, seed)
    raw, cot = case["raw"], case["cot"]
    g, mags = TR.activation_backward(cot["d_shs"], cot["d_opac"], cot["d_scales"], cot["d_rot"], cot["d_means3D"],
                                     raw["opacity"], raw["scaling"], raw["rotation"])
    t, out = _torch_activations(raw)
    loss = ((out["shs"] * _t64(cot["d_shs"], False)).sum() + (out["opacities"] * _t64(cot["d_opac"], False)).sum() +
            (out["scales"] * _t64(cot["d_scales"], False)).sum() + (out["rotations"] * _t64(cot["d_rot"], False)).sum() +
            (t["xyz"] * _t64(cot["d_means3D"], False)).sum())
    loss.backward()
    for k in ("xyz", "f_dc", "f_rest"):
        np.testing.assert_array_equal(g[k], t[k].grad.numpy(), err_msg=k)
    np.testing.assert_allclose(g["scaling"], t["scaling"].grad.numpy(), rtol=RTOL, atol=0)
    want = t["opacity"].grad.numpy()
    assert (np.abs(g["opacity"] - want) <= RTOL * np.abs(want) + 2.0 ** -52 * np.abs(cot["d_opac"])).all()
    want = t["rotation"].grad.numpy()
    assert np.isfinite(want).all() and np.isfinite(g["rotation"]).all()
    assert (np.abs(g["rotation"] - want) <= RTOL * np.abs(want) + RTOL * mags["rotation"]).all()
    # the magnitudes bound the values and equal them where there is one term
    for k in g:
        assert (np.abs(g[k]) <= mags[k] * (1 + 1e-15)).all(), k
    if P > 4:  # the edge rows (train_reference.edge_rotations, from the end backwards)
        gr, d_rot = g["rotation"], cot["d_rot"].astype(np.float64)
        np.testing.assert_allclose(gr[P - 1], d_rot[P - 1] / 1e-12, rtol=RTOL)  # zero quaternion: clamp only
        np.testing.assert_allclose(gr[P - 2], d_rot[P - 2] / 1e-12, rtol=RTOL)  # below the clamp: no norm term
        for row in (P - 3, P - 4):  # above it: the gradient is orthogonal to r
            r = raw["rotation"][row].astype(np.float64)
            assert abs(float(gr[row] @ r)) <= 1e-12 * float(mags["rotation"][row] @ np.abs(r))


def test_edge_rows_are_present():
    case = TR.raw_inputs(64, 4, 0)
    n = np.linalg.norm(case["raw"]["rotation"].astype(np.float64), axis=1)
    assert n[-1] == 0.0 and 0 < n[-2] < 1e-12 and abs(n[-3] / 1e-6 - 1) < 1e-6 and abs(n[-4] / 1e6 - 1) < 1e-6
    assert 0.5 - 1e-6 <= n[:-4].min() and n[:-4].max() <= 2.0 + 1e-6
    op = case["raw"]["opacity"].reshape(-1)
    assert sorted(op[-4:].tolist()) == [-100.0, -30.0, 30.0, 100.0]
    assert np.abs(op[:-4]).max() <= 12.0
    sc = case["raw"]["scaling"]
    assert -15.0 <= sc.min() and sc.max() <= 5.0


def test_sigmoid_is_stable_at_both_ends():
    x = np.array([-800.0, -100.0, -30.0, 0.0, 30.0, 100.0, 800.0])
    s, c = TR.sigmoid(x), TR.one_minus_sigmoid(x)
    assert np.isfinite(s).all() and np.isfinite(c).all()
    np.testing.assert_allclose(s[1], np.exp(-100.0), rtol=1e-15)
    np.testing.assert_allclose(c[5], np.exp(-100.0), rtol=1e-15)
    np.testing.assert_array_equal(s, c[::-1])


@pytest.mark.parametrize("width", [2, 3, 4])
def test_densify_stats_matches_the_torch_statements(width):
    """train.py:111-113 and gaussian_model.py:405-407 as the reference writes
    them (boolean-mask gather, torch.norm, in-place add), in float64."""
    rng = np.random.default_rng(width)
    P = 301
    radii = rng.choice(np.array([0, -3, 1, 5000], np.int32), P)
    g = rng.standard_normal((P, width)).astype(np.float32)
    g[7] = np.nan
    radii[7] = 1
    accum = rng.uniform(0, 2, (P, 1)).astype(np.float32)
    denom = rng.integers(0, 9, (P, 1)).astype(np.float32)
    mx = rng.choice(np.array([0.0, 3.0, 9000.0], np.float32), P)
    a, d, m = TR.densify_stats(radii, g, accum, denom, mx)
    ta, td, tm, tg = _t64(accum, False), _t64(denom, False), _t64(mx, False), _t64(g, False)
    tr = torch.from_numpy(radii)
    vis = tr > 0
    tm[vis] = torch.max(tm[vis], tr[vis].double())
    ta[vis] += torch.norm(tg[vis, :2], dim=-1, keepdim=True)
    td[vis] += 1
    np.testing.assert_allclose(a, ta.numpy(), rtol=RTOL, atol=0, equal_nan=True)
    np.testing.assert_array_equal(d, td.numpy())
    np.testing.assert_array_equal(m, tm.numpy())
    assert np.isnan(a[7, 0]) and int(np.isnan(a).sum()) == 1
    hidden = radii <= 0
    assert hidden.any() and np.array_equal(a[hidden], accum[hidden].astype(np.float64))
