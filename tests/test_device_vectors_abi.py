"""The device-resident vector calls (alfd_*_device) at the ABI level: declared in alfd.h, exported, mirrored by
solver.ABI_SYMBOLS with the expected argtypes, refused for a null context -- no GPU here.  What they compute is
checked on the GPU against the host-pointer calls (tests/test_gpu_device_vectors.py)."""
import ctypes as C
import os
import re

import pytest

from fictitious_domain_al_preconditioners_amd import _abi, solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PP, VP, RES = C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(_abi.Result)

# name -> (argtypes of the Python mirror, C parameter list in alfd.h with white space normalised)
DEVICE_CALLS = {
    "alfd_upload_rhs_device": ([VP, PP, PP, VP],
                               "alfd_ctx_t ctx, const double *const *rhs_blocks, const double *const *x0_blocks, "
                               "void *stream"),
    "alfd_download_solution_device": ([VP, PP, VP], "alfd_ctx_t ctx, double *const *x_blocks, void *stream"),
    "alfd_solve_device": ([VP, PP, PP, RES, VP],
                          "alfd_ctx_t ctx, const double *const *rhs_blocks, double *const *x_blocks, alfd_result *res, "
                          "void *stream"),
    "alfd_precond_apply_device": ([VP, PP, PP, RES, VP],
                                  "alfd_ctx_t ctx, const double *const *src_blocks, double *const *dst_blocks, "
                                  "alfd_result *res, void *stream"),
    "alfd_system_apply_device": ([VP, PP, PP, VP],
                                 "alfd_ctx_t ctx, const double *const *src_blocks, double *const *dst_blocks, "
                                 "void *stream"),
    "alfd_augment_rhs_device": ([VP, PP, VP], "alfd_ctx_t ctx, double *const *rhs_blocks, void *stream"),
}


@pytest.fixture(scope="module", autouse=True)
def _built(built):
    return built


def _header():
    txt = open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))


def test_declared_exported_and_mirrored():
    lib, hdr = solver.load_library(), _header()
    for name, (argtypes, params) in DEVICE_CALLS.items():
        assert f"int {name}({params});" in hdr, name
        assert hasattr(lib, name), name
        assert name in solver.ABI_SYMBOLS, name
        fn = getattr(lib, name)
        assert fn.restype == C.c_int and fn.argtypes == argtypes, (name, fn.argtypes)


def test_null_context_is_refused():
    lib = solver.load_library()
    tab = (C.c_void_p * _abi.ALFD_MAX_BLOCKS)()          # a block table of null pointers: never looked at
    res = _abi.Result()
    assert lib.alfd_upload_rhs_device(None, tab, tab, None) == _abi.E_INVALID
    assert lib.alfd_upload_rhs_device(None, tab, None, None) == _abi.E_INVALID
    assert lib.alfd_download_solution_device(None, tab, None) == _abi.E_INVALID
    assert lib.alfd_solve_device(None, tab, tab, C.byref(res), None) == _abi.E_INVALID
    assert lib.alfd_precond_apply_device(None, tab, tab, C.byref(res), None) == _abi.E_INVALID
    assert lib.alfd_precond_apply_device(None, tab, tab, None, None) == _abi.E_INVALID
    assert lib.alfd_system_apply_device(None, tab, tab, None) == _abi.E_INVALID
    assert lib.alfd_augment_rhs_device(None, tab, None) == _abi.E_INVALID


def test_abi_version_and_struct_sizes_unchanged():
    """The six symbols are additive: no version bump, same struct layouts."""
    lib = solver.load_library()
    assert lib.alfd_abi_version() == 12
    assert "#define ALFD_ABI_VERSION 12" in open(os.path.join(ROOT, "include", "alfd", "alfd.h")).read()
    assert C.sizeof(_abi.Config) == 264 and C.sizeof(_abi.Result) == 80


def test_python_front_end_checks_arguments_without_a_gpu():
    """Context.*_device validate before the library is called: an object without __cuda_array_interface__ (a numpy
    array), a wrong dtype, rank, length, stride or a read-only output raise ValueError."""
    class Fake:   # what a device array exposes; the address is never dereferenced here
        def __init__(self, n, typestr="<f8", strides=None, readonly=False, shape=None):
            self.__cuda_array_interface__ = dict(shape=shape or (n,), typestr=typestr, strides=strides,
                                                 data=(4096, readonly), version=2)
    import numpy as np
    ctx = solver.Context.__new__(solver.Context)          # no alfd_create: the checks need the block sizes only
    ctx._h, ctx.block_sizes = None, [5, 3]
    ok = [Fake(5), Fake(3)]
    tab = ctx._dev(ok, "x", writable=True)
    assert [tab[0], tab[1]] == [4096, 4096]
    assert ctx._dev([Fake(5, strides=(8,)), Fake(3)], "x")[0] == 4096
    for bad in ([np.zeros(5), np.zeros(3)], [Fake(5, "<f4"), Fake(3)], [Fake(4), Fake(3)], [Fake(5)],
                [Fake(5, strides=(16,)), Fake(3)], [Fake(5, shape=(5, 1)), Fake(3)]):
        with pytest.raises(ValueError):
            ctx._dev(bad, "x")
    with pytest.raises(ValueError):
        ctx._dev([Fake(5, readonly=True), Fake(3)], "x", writable=True)
    class Raises:   # a torch tensor that requires grad raises RuntimeError from the property
        @property
        def __cuda_array_interface__(self):
            raise RuntimeError("requires grad")
    with pytest.raises(ValueError):
        ctx._dev([Raises(), Fake(3)], "x")
    assert ctx._dev([Fake(5, readonly=True), Fake(3)], "x")[0] == 4096        # inputs may be read-only
    ctx.block_sizes = [5, 0]
    assert ctx._dev([Fake(5), Fake(0)], "x")[1] is None                       # an empty block travels as a null pointer
    # streams: an integer is a raw handle, 0 / None without torch tensors the null stream
    assert solver.Context._stream(0, ok).value is None
    assert solver.Context._stream(1234, ok).value == 1234
    assert solver.Context._stream(None, ok).value is None
