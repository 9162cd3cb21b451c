"""The sparse Adam step (csrc/train.hip sparse_adam_kernel, the upstream
trainer's ``--optimizer_type sparse_adam``) restated in plain numpy over the
trainer's flat layout: one float32 buffer, ``seg_end`` exclusive segment ends,
segment ``s`` holding ``P = len(radii)`` rows of ``(end_s - end_{s-1}) / P``
floats.

For every segment with ``step > 0`` and every row with ``radii > 0``, per
element, in float32 with every operation rounded on its own::

    omb1 = 1 - b1;  omb2 = 1 - b2            (b1 = float32(beta1), b2 = float32(beta2))
    m' = b1 * m + omb1 * g
    v' = b2 * v + (omb2 * g) * g
    p' = p + (-float32(lr) * m') / (sqrt(v') + float32(eps))

No bias correction, no step count in the formula.  Every other row keeps
p, m, v, and its gradient is never read (the visible rows are gathered first,
so a NaN in an invisible row cannot reach a result).

``step`` is that formula with one float32 operation per statement;
``step_f64`` evaluates the same formula (same float32 constants and inputs) in
float64 and returns the magnitudes the float32 error bounds are stated in.
tests/test_sparse_adam_reference.py pins ``step`` bit for bit to a torch-CPU
restatement in upstream's shape and to ``step_f64`` within those bounds.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
U = 2.0 ** -24  # float32 unit roundoff


def segment_rows(n: int, seg_end, P: int):
    """[(lo, width)] per segment; refuses what the kernel's callers refuse."""
    ends = [int(e) for e in seg_end]
    if not 1 <= len(ends) <= 8:
        raise ValueError("1..8 segments")
    if ends[-1] != n or any(b < a for a, b in zip([0] + ends[:-1], ends)):
        raise ValueError("segments must be ordered and cover the buffer")
    out = []
    lo = 0
    for e in ends:
        if P > 0 and (e - lo) % P != 0:
            raise ValueError("a segment is not P whole rows")
        out.append((lo, (e - lo) // P if P > 0 else 0))
        lo = e
    return out


def step(p, g, m, v, seg_end, lr, step, radii, beta1, beta2, eps):
    """One sparse step on float32 arrays; returns new (p, m, v), inputs untouched."""
    p, m, v = (np.array(a, dtype=F32, copy=True) for a in (p, m, v))
    g = np.asarray(g, dtype=F32)
    radii = np.asarray(radii).reshape(-1)
    P = radii.size
    vis = np.nonzero(radii > 0)[0]
    b1 = F32(beta1)
    b2 = F32(beta2)
    one = F32(1.0)
    omb1 = one - b1
    omb2 = one - b2
    e32 = F32(eps)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for (lo, w), lr_s, t in zip(segment_rows(p.size, seg_end, P), lr, step):
            if t <= 0 or w == 0 or vis.size == 0:
                continue
            rows = lambda a: a[lo:lo + P * w].reshape(P, w)  # noqa: E731  (views)
            gv = rows(g)[vis]
            mv = rows(m)[vis]
            vv = rows(v)[vis]
            pv = rows(p)[vis]
            neg_lr = -F32(lr_s)
            a = b1 * mv
            b = omb1 * gv
            m1 = a + b
            c = b2 * vv
            d = omb2 * gv
            d = d * gv
            v1 = c + d
            num = neg_lr * m1
            den = np.sqrt(v1)
            den = den + e32
            q = num / den
            p1 = pv + q
            for arr in (a, b, m1, c, d, v1, num, den, q, p1):
                assert arr.dtype == F32
            rows(m)[vis] = m1
            rows(v)[vis] = v1
            rows(p)[vis] = p1
    return p, m, v


def step_f64(p, g, m, v, seg_end, lr, step, radii, beta1, beta2, eps):
    """The same formula from the same float32 inputs and float32 constants,
    evaluated in float64.  Returns (p, m, v, bound_p, bound_m, bound_v): the
    float64 results and, per element, the bound a float32 evaluation with one
    rounding per operation stays within (0 where the element is untouched).

    Derivation (u = 2^-24; each float32 operation errs by at most u times its
    exact result, or by 2^-150 where the result is subnormal; v >= 0):

    * m' = fl(fl(b1 m) + fl(omb1 g)).  With A_m = |b1 m| + |omb1 g| the two
      products err by u A_m together and the sum by u |m'| <= u A_m (1 + u):
      |dm| <= 2.01 u A_m + 3 * 2^-150.                       asserted: 2.5 u A_m + 2^-148
    * v' = fl(fl(b2 v) + fl(fl(omb2 g) g)): all terms are non-negative, so
      A_v = v'; three roundings deep: |dv| <= 3.01 u v' + 3 * 2^-150.
                                                              asserted: 3.5 u v' + 2^-148
    * den = fl(fl(sqrt(v')) + eps): the square root halves v's relative error
      (1.51 u) and adds one rounding, the sum (non-negative terms) another:
      3.51 u den; an absolute error of 2^-148 in v' moves sqrt(v') by at most
      2^-74, which is 0.89 u of den >= eps = 1e-15 (the bound assumes
      eps >= 1e-15): |dden| <= 4.4 u den.
    * num = fl(-lr m'): |dnum| <= (2.01 + 1.01) u lr A_m + lr 2^-148 + 2^-150.
    * q = fl(num / den): |dq| <= |dnum| / den + |num| 4.4 u / den + u |q|
      <= (3.02 + 4.4 + 1 + second order) u lr A_m / den + 2^-146 / den,
      using |m'| <= A_m.                                     asserted: 9 u lr A_m / den + 2^-146 / den
    * p' = fl(p + q): |dp| <= u |p'| + |dq| + 2^-150.
    """
    f64 = lambda a: np.array(a, dtype=F32).astype(np.float64)  # noqa: E731
    p, m, v, g = f64(p), f64(m), f64(v), np.asarray(g, dtype=F32)
    bp, bm, bv = np.zeros_like(p), np.zeros_like(p), np.zeros_like(p)
    radii = np.asarray(radii).reshape(-1)
    P = radii.size
    vis = np.nonzero(radii > 0)[0]
    b1 = np.float64(F32(beta1))
    b2 = np.float64(F32(beta2))
    omb1 = np.float64(F32(1.0) - F32(beta1))
    omb2 = np.float64(F32(1.0) - F32(beta2))
    e64 = np.float64(F32(eps))
    tiny = 2.0 ** -148
    for (lo, w), lr_s, t in zip(segment_rows(p.size, seg_end, P), lr, step):
        if t <= 0 or w == 0 or vis.size == 0:
            continue
        rows = lambda a: a[lo:lo + P * w].reshape(P, w)  # noqa: E731
        gv = rows(g)[vis].astype(np.float64)
        mv, vv, pv = rows(m)[vis], rows(v)[vis], rows(p)[vis]
        lr64 = np.float64(F32(lr_s))
        m1 = b1 * mv + omb1 * gv
        A_m = np.abs(b1 * mv) + np.abs(omb1 * gv)
        v1 = b2 * vv + (omb2 * gv) * gv
        den = np.sqrt(v1) + e64
        p1 = pv + (-lr64 * m1) / den
        rows(m)[vis] = m1
        rows(v)[vis] = v1
        rows(p)[vis] = p1
        rows(bm)[vis] = 2.5 * U * A_m + tiny
        rows(bv)[vis] = 3.5 * U * v1 + tiny
        rows(bp)[vis] = U * np.abs(p1) + 9.0 * U * lr64 * A_m / den + 4.0 * tiny / den + tiny
    return p, m, v, bp, bm, bv


# ------------------------------------------------------------- test inputs ---
GROUP_WIDTHS = lambda M: (3, 3, 3 * (M - 1), 1, 3, 4)  # noqa: E731  xyz, f_dc, f_rest, opacity, scaling, rotation


def flat_layout(P: int, M: int):
    """seg_end of the trainer's flat buffer for P Gaussians with M SH coefficients."""
    return [int(e) for e in np.cumsum([P * w for w in GROUP_WIDTHS(M)])]


# g, m, v of the edge rows: g = 0; v = 0 with g = 0 (the quotient is m' / eps
# alone); subnormal g; large g (its square, 1e36, is still finite in float32).
EDGE_ROWS = ((0.0, 0.25, 0.5), (0.0, 0.125, 0.0), (0.0, 0.0, 0.0), (1e-42, 0.0, 0.0), (-3e-41, 1e-3, 1e-6),
             (1e18, -2.0, 1e30), (-1e18, 0.0, 0.0))


def make_state(P: int, M: int, seed: int, edges: bool = True):
    """Float32 p, g, m (any sign), v >= 0 over flat_layout(P, M), with the
    EDGE_ROWS values written over the first elements of every segment."""
    rng = np.random.default_rng(seed)
    ends = flat_layout(P, M)
    n = ends[-1]
    p = rng.standard_normal(n).astype(F32)
    g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-8, 0, n)).astype(F32)
    m = (rng.standard_normal(n) * 1e-3).astype(F32)
    v = (rng.uniform(0, 1, n) ** 4 * 1e-4).astype(F32)
    if edges:
        lo = 0
        for e in ends:
            for k, (ge, me, ve) in enumerate(EDGE_ROWS[:max(0, e - lo)]):
                g[lo + k], m[lo + k], v[lo + k] = ge, me, ve
            lo = e
    return p, g, m, v, ends


def masks(P: int, seed: int = 0):
    """name -> int32 radii [P] (visible iff > 0), the masks of the GPU test."""
    rng = np.random.default_rng(1000 + seed)
    i = np.arange(P)
    big = rng.integers(1, 200, P).astype(np.int32)
    out = {"all": big.copy(), "none": np.zeros(P, np.int32)}
    out["first"] = np.where(i == 0, big, 0).astype(np.int32)
    out["last"] = np.where(i == P - 1, big, 0).astype(np.int32)
    out["alternating"] = np.where(i % 2 == 0, big, 0).astype(np.int32)
    out["runs64"] = np.where((i // 64) % 2 == 0, big, 0).astype(np.int32)
    out["runs65"] = np.where((i // 65) % 2 == 1, big, 0).astype(np.int32)
    out["random50"] = np.where(rng.random(P) < 0.5, big, 0).astype(np.int32)
    out["random10"] = np.where(rng.random(P) < 0.1, big, 0).astype(np.int32)
    out["signed"] = rng.integers(-3, 4, P).astype(np.int32)  # zeros and negatives are invisible
    return out
