"""Host side of the sparse Adam option (training.py optimizer_type, the C
entry's declaration and export, reduce_visibility at world sizes 1 and 2 over
gloo).  The kernel itself is in tests/test_gpu_sparse_adam.py."""
import ctypes
import dataclasses
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from gaussian_splatting_with_eye_tracking_amd import training as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "gsplat_amd.h")
LIB = os.path.join(ROOT, "gaussian_splatting_with_eye_tracking_amd", "libgsplat_amd.so")


def _raw(P, sh_degree=3):
    g = torch.Generator().manual_seed(0)
    M = (sh_degree + 1) ** 2
    return {"xyz": torch.randn(P, 3, generator=g), "f_dc": torch.randn(P, 1, 3, generator=g),
            "f_rest": torch.randn(P, M - 1, 3, generator=g), "opacity": torch.randn(P, 1, generator=g),
            "scaling": torch.randn(P, 3, generator=g) - 4.0, "rotation": torch.randn(P, 4, generator=g)}


def test_optimizer_type_default_and_names():
    o = T.OptimizationParams()
    assert o.optimizer_type == "default"
    assert dataclasses.fields(T.OptimizationParams)[-1].name == "optimizer_type"
    assert T.OPTIMIZER_TYPES == ("default", "sparse_adam")
    for name in T.OPTIMIZER_TYPES:
        m = T.FlatGaussianModel(_raw(5), 3, 1.0, opt=T.OptimizationParams(optimizer_type=name), device="cpu")
        assert m.opt.optimizer_type == name


@pytest.mark.parametrize("bad", ["adam", "sparse", "", "SPARSE_ADAM", None])
def test_unknown_optimizer_type_is_refused_at_construction(bad):
    with pytest.raises(ValueError, match="optimizer_type"):
        T.FlatGaussianModel(_raw(5), 3, 1.0, opt=T.OptimizationParams(optimizer_type=bad), device="cpu")


def test_sparse_step_without_an_active_group_is_a_no_op_before_radii_are_looked_at():
    """After densify_and_prune no group has a gradient and the render
    package's radii still have the old length: nothing is launched (this runs
    without a GPU) and nothing is checked."""
    m = T.FlatGaussianModel(_raw(7), 3, 1.0, opt=T.OptimizationParams(optimizer_type="sparse_adam"), device="cpu")
    before = m.params.clone()
    assert not any(m.has_grad.values())
    m.optimizer_step(torch.ones(3, dtype=torch.int64))
    m.optimizer_step(None)
    assert torch.equal(m.params, before) and all(v == 0 for v in m.steps.values())
    m.mark_backward()
    with pytest.raises(ValueError, match="radii"):
        m.optimizer_step(None)


def test_header_declares_and_library_exports_the_entry():
    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    decl = re.search(r"int\s+gs_sparse_adam_step\s*\(([^;]*)\)\s*;", text)
    assert decl, "gs_sparse_adam_step is not declared"
    args = [a.strip() for a in " ".join(decl.group(1).split()).split(",")]
    assert args == ["float* params", "const float* grads", "float* exp_avg", "float* exp_avg_sq", "long long n",
                    "int nseg", "const long long* seg_end", "const double* lr", "const long long* step", "int P",
                    "const int* radii", "double beta1", "double beta2", "double eps", "void* stream"]
    assert re.search(r"#define GSPLAT_AMD_ABI_VERSION 7\b", text)  # an additive entry
    lib = ctypes.CDLL(LIB)
    assert hasattr(lib, "gs_sparse_adam_step") and hasattr(lib, "gs_adam_step")
    lib.gs_sparse_adam_rows_per_pass.restype = ctypes.c_longlong
    assert lib.gs_sparse_adam_rows_per_pass() > 0


def test_host_refusals_of_the_c_entry_need_no_device():
    """Segment-count, whole-rows and null-radii errors are raised before any
    launch; P == 0 and n == 0 return 0 without one."""
    lib = ctypes.CDLL(LIB)
    lib.gs_last_error.restype = ctypes.c_char_p
    LL, D = ctypes.c_longlong, ctypes.c_double
    f = lib.gs_sparse_adam_step
    f.argtypes = [ctypes.c_void_p] * 4 + [LL, ctypes.c_int, ctypes.POINTER(LL), ctypes.POINTER(D), ctypes.POINTER(LL),
                                          ctypes.c_int, ctypes.c_void_p, D, D, D, ctypes.c_void_p]
    f.restype = ctypes.c_int

    def call(ends, P, radii, n=None):
        k = len(ends)
        return f(None, None, None, None, ends[-1] if n is None else n, k, (LL * k)(*ends), (D * k)(*[1e-3] * k),
                 (LL * k)(*[1] * k), P, radii, 0.9, 0.999, 1e-15, None)

    assert call([12, 24], 4, None) < 0 and b"radii" in lib.gs_last_error()
    assert call([12, 25], 4, ctypes.c_void_p(16)) < 0 and b"whole rows" in lib.gs_last_error()
    assert call(list(range(4, 40, 4)), 4, ctypes.c_void_p(16)) < 0 and b"1..8" in lib.gs_last_error()
    assert call([12, 24], 0, None) == 0
    assert call([0, 0], 4, None, n=0) == 0


def test_reduce_visibility_is_the_identity_at_world_size_one():
    r = torch.tensor([3, 0, -1, 7], dtype=torch.int32)
    assert T.reduce_visibility(r) is r


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _radii_of(rank):
    return torch.from_numpy(np.random.default_rng(rank).integers(-2, 9, 101).astype(np.int32))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import sys
        sys.path.insert(0, ROOT)
        from gaussian_splatting_with_eye_tracking_amd import training
        mine = _radii_of(rank)
        keep = mine.clone()
        out = training.reduce_visibility(mine)
        q.put((rank, out.numpy().copy(), bool(torch.equal(mine, keep)), out.data_ptr() != mine.data_ptr()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_reduce_visibility_is_the_elementwise_maximum_at_world_size_two():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=240) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = torch.maximum(_radii_of(0), _radii_of(1)).numpy()
    assert ((want > 0) == ((_radii_of(0) > 0) | (_radii_of(1) > 0)).numpy()).all()  # the union of the views
    for _rank, out, input_kept, is_clone in got:
        assert out.dtype == np.int32
        np.testing.assert_array_equal(out, want)
        assert input_kept and is_clone
