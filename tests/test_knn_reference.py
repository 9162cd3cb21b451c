"""tests/knn_reference.py against the oracle, on the CPU.

orc_knn (oracle.dist_cuda2) restates the kernel's Morton / box / window
reject algorithm; brute_force_f32 and kdtree_f64 know nothing of it.  On
every small cloud the oracle equals the all-pairs search bit for bit
(compared as uint32, so the inf of P = 1, 2 and the FLT_MAX-dominated value
of P = 3 count), and the all-pairs search stays inside the k-d tree's derived
bound (knn_reference.KD_RTOL) wherever P >= 4.
"""
import numpy as np
import pytest

import knn_reference as K
import oracle as O


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", list(K.SMALL))
def test_oracle_equals_brute_force_and_kdtree_bounds_it(name):
    pts = K.SMALL[name]()
    assert pts.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] == 3 and pts.shape[0] <= 10_000
    bf = K.brute_force_f32(pts)
    np.testing.assert_array_equal(_bits(O.dist_cuda2(pts)), _bits(bf))
    if name in K.KNOWN:
        np.testing.assert_array_equal(bf, np.full(len(pts), K.KNOWN[name], np.float32))
    if len(pts) >= 4:
        ratio = K.kd_ratio(bf, K.kdtree_f64(pts))
        print(f"{name}: brute force vs k-d tree, worst error / bound = {ratio:.3f}")
        assert ratio <= 1.0


def test_fewer_than_three_neighbours():
    """The FLT_MAX slots reach the sum: inf at P = 1 and 2 (two slots
    overflow), a finite FLT_MAX-dominated value at P = 3."""
    for P in (1, 2):
        assert np.all(np.isposinf(K.brute_force_f32(K.SMALL[f"normal_P{P}"]())))
    v = K.brute_force_f32(K.SMALL["normal_P3"]())
    assert np.all(np.isfinite(v)) and np.all(v >= K.FLT_MAX / np.float32(3))


def test_brute_force_blocking_does_not_change_the_bits():
    pts = K.SMALL["normal_P1025"]()
    np.testing.assert_array_equal(_bits(K.brute_force_f32(pts, block=512)), _bits(K.brute_force_f32(pts, block=100)))


@pytest.mark.parametrize("shape", [(7,), (7, 2), (7, 4), (3, 7, 3)])
def test_binding_refuses_other_shapes_first(shape):
    """The shape is checked before the device: this needs no GPU (the same
    shapes as device tensors are in tests/test_gpu_knn.py)."""
    import torch
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match=r"points must be \[P, 3\]"):
        distCUDA2(torch.zeros(shape))
    assert tuple(distCUDA2(torch.zeros((0, 3))).shape) == (0,)
