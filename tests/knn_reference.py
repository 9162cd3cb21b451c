"""Independent references for simple-knn (distCUDA2: the mean of the squared
distances to the three nearest other points) and the point clouds its tests
share.  Test infrastructure only.

Neither reference knows about Morton codes, boxes or the window reject of
csrc/knn.hip and oracle/gs_oracle.c (orc_knn restates the kernel's algorithm
line by line): distCUDA2's result is an exact 3-NN whatever the Morton order
is, so an all-pairs search and a k-d tree pin it from outside.

* ``brute_force_f32``: all pairs in numpy float32 in the kernel's operation
  order; equal to the kernel bit for bit, P < 4 included.
* ``kdtree_f64``: scipy's cKDTree in float64, for sizes where all pairs cost
  too much.  ``KD_RTOL`` is its derived bound against a float32 evaluation.
"""
from __future__ import annotations

import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)

# A float32 evaluation against the float64 one, relative to the float64
# value, in units of 2^-24 (half an ulp): the coordinate subtraction rounds
# once and enters squared (2), the square (1), the two adds of the three
# squares (2), the two adds of the three neighbours (2), the division (1).
# Every term is non-negative, so the relative errors do not amplify; where
# the third neighbour is nearly tied the two candidates' distances differ by
# less than their own rounding, so either choice stays inside.  No absolute
# term: exact duplicates give exact zeros in both.
KD_RTOL = 8.0 * 2.0 ** -24


def brute_force_f32(pts, block: int = 512) -> np.ndarray:
    """[P] float32: (b0 + b1) + b2 over 3 of the three smallest of
    {|p_j - p_i|^2, j != i} and three FLT_MAX slots, every operation in
    float32 in the kernel's order: d = other - self, (d0*d0 + d1*d1) + d2*d2.
    The sums may overflow to inf (P < 3), as the kernel's do."""
    p = np.ascontiguousarray(pts, np.float32)
    P = p.shape[0]
    out = np.empty(P, np.float32)
    three = np.float32(3)
    with np.errstate(over="ignore"):
        for q0 in range(0, P, block):
            q = p[q0:q0 + block]
            d = p[None, :, :] - q[:, None, :]                               # other - self
            d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            d2[np.arange(q.shape[0]), q0 + np.arange(q.shape[0])] = FLT_MAX  # self is excluded
            d2 = np.minimum(d2, FLT_MAX)                                     # (an inf never displaces a slot)
            d2 = np.concatenate([d2, np.full((q.shape[0], 3), FLT_MAX, np.float32)], axis=1)
            b = np.sort(np.partition(d2, 2, axis=1)[:, :3], axis=1)
            out[q0:q0 + block] = ((b[:, 0] + b[:, 1]) + b[:, 2]) / three
    assert out.dtype == np.float32
    return out


def kdtree_f64(pts, workers: int = 16) -> np.ndarray:
    """[P] float64: the mean of the three smallest squared distances to the
    other points, P >= 4.  (With duplicates the query point itself need not
    be the first hit, but the first hit is at distance 0 either way.)"""
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(pts, np.float64)
    assert p.shape[0] >= 4
    d, _ = cKDTree(p).query(p, k=4, workers=workers)
    return (d[:, 1:4] ** 2).sum(axis=1) / 3.0


def kd_ratio(got, ref) -> float:
    """max |got - ref| / (KD_RTOL * ref); exact zeros must be met exactly."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    if np.any((ref == 0.0) & (err != 0.0)):
        return float("inf")
    nz = ref > 0.0
    return float((err[nz] / (KD_RTOL * ref[nz])).max()) if nz.any() else 0.0


# ----------------------------------------------------------------- the clouds
def _normal(P, seed, sigma=3.0):
    return np.random.default_rng(seed).normal(0.0, sigma, (P, 3)).astype(np.float32)


def _clusters(P, seed):
    rng = np.random.default_rng(seed)
    c = np.array([[0, 0, 0], [50, 0, 0], [0, -80, 3]], np.float64)
    return (c[rng.integers(0, 3, P)] + rng.normal(0.0, 0.01, (P, 3))).astype(np.float32)


def _lattice(n):
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    return np.random.default_rng(31).permutation(g.astype(np.float32))  # (shuffled: index order is no help)


def _flat(P, seed, axes):
    p = _normal(P, seed)
    p[:, axes] = 0.0
    return p


# name -> builder.  Every cloud comes from a fixed seed; P <= 10,000.
SMALL = {}
for _P in (1, 2, 3, 4, 1023, 1024, 1025, 4095, 4096, 4097, 8193):
    # fewer than three neighbours; the 1024-point box and 4096-item radix tile, one below / at / one above;
    # 8193 = two full radix tiles and one item, nine boxes
    SMALL[f"normal_P{_P}"] = (lambda P=_P: _normal(P, 100 + P))
SMALL["positive_P4097"] = lambda: np.random.default_rng(7).uniform(1.0, 2.0, (4097, 3)).astype(np.float32)
SMALL["negative_P4097"] = lambda: -SMALL["positive_P4097"]()
SMALL["flat_z_P3000"] = lambda: _flat(3000, 8, [2])
SMALL["line_P2000"] = lambda: _flat(2000, 9, [1, 2])
SMALL["identical_P1500"] = lambda: np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (1500, 1))
SMALL["duplicates_4x1024"] = lambda: np.random.default_rng(10).permutation(np.tile(_normal(1024, 11), (4, 1)))
SMALL["clusters_P8193"] = lambda: _clusters(8193, 12)
SMALL["scaled_1e4_P4097"] = lambda: _normal(4097, 13) * np.float32(1e4)
SMALL["scaled_1e-4_P4097"] = lambda: _normal(4097, 13) * np.float32(1e-4)
SMALL["lattice_20"] = lambda: _lattice(20)

# name -> the exact value of every element, where it is known without a reference
KNOWN = {"identical_P1500": 0.0, "duplicates_4x1024": 0.0, "lattice_20": 1.0}

LARGE = {
    "normal_P300001": lambda: _normal(300_001, 14),
    # 1026 boxes: the second staging round of knn_box_mean_dist holds two boxes, the last box one point
    "uniform_P1049601": lambda: np.random.default_rng(15).uniform(-1.0, 1.0, (1_049_601, 3)).astype(np.float32),
}
