"""simple-knn (csrc/knn.hip, distCUDA2) at its edges, against references that
do not share its algorithm (tests/knn_reference.py, pinned on the CPU by
tests/test_knn_reference.py).

distCUDA2's result is an exact 3-NN whatever the Morton order is.  The
{0,0,0} start of the bounding box and the 0/0 code of a flat axis therefore
change speed only and cannot be seen in the output.  These tests pin the
output; exposing the intermediates (codes, sorted indices, boxes) is out of
scope.

* Small clouds (P <= 10,000): the GPU's bits equal brute_force_f32's and
  oracle.dist_cuda2's, compared as uint32 so that inf counts.  The sizes sit
  on P < 4 (the FLT_MAX slots reach the sum), on the 1024-point box and the
  4096-item radix tile (one below, at, one above), and the clouds are
  one-sided, flat, collinear, identical, duplicated, clustered and scaled.
* Large clouds: element-wise within knn_reference.KD_RTOL (8 * 2^-24,
  derived there) of a float64 k-d tree.  P = 1,049,601 is 1026 boxes, the
  smallest size at which knn_box_mean_dist's staging loop takes a second
  round (two boxes in it, one point in the last).
* Through the C ABI with mean_dists pre-filled with NaN: no NaN is left, so
  every index survived the radix sort and was written where it belongs (the
  binding allocates the output with torch::empty; garbage could pass there).
* The binding refuses anything but [P, 3] on the host.

Every test prints its worst error-to-bound ratio (pytest -s).
"""
import ctypes
import functools

import numpy as np
import pytest

import knn_reference as K

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dist(pts):
    from simple_knn._C import distCUDA2
    return distCUDA2(pts if isinstance(pts, torch.Tensor) else torch.from_numpy(pts).cuda()).cpu().numpy()


@functools.lru_cache(maxsize=None)
def _large(name):
    pts = K.LARGE[name]()
    ref = K.kdtree_f64(pts)
    pts.setflags(write=False)
    ref.setflags(write=False)
    return pts, ref


def _assert_exact_zeros_and_known(name, got):
    if name in K.KNOWN:
        np.testing.assert_array_equal(got, np.full(got.shape, K.KNOWN[name], np.float32))


@pytest.mark.parametrize("name", list(K.SMALL))
def test_small_clouds_bit_exact(name):
    import oracle as O
    pts = K.SMALL[name]()
    assert len(pts) <= 10_000
    got = _dist(pts)
    assert got.dtype == np.float32 and got.shape == (len(pts),)
    np.testing.assert_array_equal(_bits(got), _bits(K.brute_force_f32(pts)))
    np.testing.assert_array_equal(_bits(got), _bits(O.dist_cuda2(pts)))
    _assert_exact_zeros_and_known(name, got)


@pytest.mark.parametrize("name", list(K.LARGE))
def test_large_clouds_within_the_kdtree_bound(name):
    pts, ref = _large(name)
    got = _dist(pts)
    ratio = K.kd_ratio(got, ref)
    print(f"{name}: GPU vs float64 k-d tree, worst error / (8 * 2^-24 * ref) = {ratio:.3f}")
    assert np.all(np.isfinite(got))
    assert ratio <= 1.0


def test_transposed_view_gives_the_contiguous_bits():
    pts = K.SMALL["normal_P4097"]()
    soa = torch.from_numpy(np.ascontiguousarray(pts.T)).cuda()  # [3, P]
    view = soa.t()                                             # [P, 3], strides (1, P)
    assert not view.is_contiguous() and tuple(view.shape) == (4097, 3)
    np.testing.assert_array_equal(_bits(_dist(view)), _bits(_dist(view.contiguous())))
    np.testing.assert_array_equal(_bits(_dist(view)), _bits(K.brute_force_f32(pts)))


# ------------------------------------------------------------- the C ABI ----
def _knn_capi(pts):
    """gs_simple_knn through ctypes into an output pre-filled with NaN."""
    import capi_helpers as CT
    lib = CT.lib()
    lib.gs_simple_knn.argtypes = [CT.I, CT.VP, CT.VP, CT.GsBuffer, CT.VP]
    lib.gs_simple_knn.restype = CT.I
    P = len(pts)
    dev = torch.from_numpy(pts).cuda()
    out = torch.full((P,), float("nan"), dtype=torch.float32, device="cuda")
    bufs = CT.Buffers(dev.device)
    stream = torch.cuda.current_stream()
    CT.check(lib, lib.gs_simple_knn(P, CT.ptr(dev), CT.ptr(out), bufs.buf("scratch"), ctypes.c_void_p(stream.cuda_stream)),
              "gs_simple_knn")
    stream.synchronize()
    return out.cpu().numpy()


def test_capi_writes_every_element_small():
    pts = K.SMALL["normal_P4097"]()
    got = _knn_capi(pts)
    assert not np.isnan(got).any()
    np.testing.assert_array_equal(_bits(got), _bits(K.brute_force_f32(pts)))


def test_capi_writes_every_element_large():
    pts, ref = _large("uniform_P1049601")
    got = _knn_capi(pts)
    assert not np.isnan(got).any()
    ratio = K.kd_ratio(got, ref)
    print(f"C ABI, uniform_P1049601: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


# ----------------------------------------------------------- shape check ----
@pytest.mark.parametrize("shape", [(7,), (7, 2), (7, 4), (3, 7, 3)])
def test_wrong_shapes_raise_on_the_host(shape):
    """[P] and [P, 2] would be read out of bounds, [P, 4] with the wrong
    stride: the binding raises before anything is launched."""
    from simple_knn._C import distCUDA2
    with pytest.raises(RuntimeError, match=r"points must be \[P, 3\]"):
        distCUDA2(torch.zeros(shape, dtype=torch.float32, device="cuda"))


def test_empty_and_views_are_still_accepted():
    from simple_knn._C import distCUDA2
    out = distCUDA2(torch.zeros((0, 3), dtype=torch.float32, device="cuda"))
    assert tuple(out.shape) == (0,) and out.dtype == torch.float32
    pts = K.SMALL["normal_P1025"]()
    wide = torch.zeros((1025, 5), dtype=torch.float32, device="cuda")
    wide[:, 1:4] = torch.from_numpy(pts).cuda()
    np.testing.assert_array_equal(_bits(_dist(wide[:, 1:4])), _bits(K.brute_force_f32(pts)))
