"""alfd_get_last_spmv_launch without a GPU: declared, exported, mirrored field by field, refused on null arguments."""
import ctypes as C
import os
import re

from fictitious_domain_al_preconditioners_amd import _abi, solver

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "alfd", "alfd.h")


def _header():
    with open(HEADER) as f:
        return f.read()


def test_last_spmv_launch_is_declared_exported_and_mirrored(built):
    lib = solver.load_library()
    assert "alfd_get_last_spmv_launch" in solver.ABI_SYMBOLS and hasattr(lib, "alfd_get_last_spmv_launch")
    assert re.search(r"int alfd_get_last_spmv_launch\(alfd_ctx_t ctx, alfd_spmv_launch \*out\);", _header())
    assert lib.alfd_get_last_spmv_launch.argtypes == [C.c_void_p, C.POINTER(_abi.SpmvLaunch)]
    assert hasattr(solver.Context, "last_spmv_launch")


def test_struct_and_enum_mirror_the_header():
    text = _header()
    body = re.search(r"typedef struct alfd_spmv_launch \{(.*?)\} alfd_spmv_launch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int32_t|int64_t) ([^;]+);", body):
        fields += [(n.strip(), {"int32_t": C.c_int32, "int64_t": C.c_int64}[ctype]) for n in names.split(",")]
    assert fields == list(_abi.SpmvLaunch._fields_)
    assert C.sizeof(_abi.SpmvLaunch) == 48
    enum = re.search(r"enum alfd_spmv_family \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"ALFD_SPMV_(\w+) = (\d+)", enum)
    assert [int(v) for _, v in names] == list(range(len(names)))
    assert names[-1][0] == "NFAMILIES" and int(names[-1][1]) == _abi.SPMV_NFAMILIES == len(_abi.SPMV_FAMILY_NAMES)
    for name, value in names[:-1]:
        assert getattr(_abi, "SPMV_" + name) == int(value)
        assert _abi.SPMV_FAMILY_NAMES[int(value)] == name.lower()


def test_last_spmv_launch_refuses_null_arguments(built):
    """A null context or a null record answers ALFD_E_INVALID before anything is read or written.  (ALFD_E_NOT_SETUP
    before the first launch and the records themselves need a live context: tests/test_gpu_launch_shapes.py.)"""
    lib = solver.load_library()
    rec = _abi.SpmvLaunch(family=-7, grid=-7)
    assert lib.alfd_get_last_spmv_launch(None, C.byref(rec)) == _abi.E_INVALID
    assert (rec.family, rec.grid) == (-7, -7)
