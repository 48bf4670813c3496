"""The sanity block of the drivers (elliptic_interface.cc:973-1009) through include/alfd/dealii_adapter.hpp:
System::constraint_residual and System::estimate_condition_number_CCt compiled against the mock deal.II classes
(tests/adapter/spectrum_demo.cpp) and driven once on the GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "fictitious_domain_al_preconditioners_amd", "lib")


@pytest.fixture(scope="module")
def demo(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter_spectrum") / "spectrum_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "adapter", "spectrum_demo.cpp"), "-L" + LIB, "-lalfd",
                           "-lalfd_synth", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_adapter_methods_compile_and_fail_loudly_without_gpu(demo):
    import torch
    p = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    if torch.cuda.is_available():
        assert p.returncode == 0, p.stderr
    else:
        assert p.returncode == 3, (p.returncode, p.stderr)      # alfd_create -> ALFD_E_HIP -> Error
        assert "alfd_create" in p.stderr


@pytest.mark.gpu
def test_adapter_sanity_block_on_the_gpu(demo):
    """elliptic_interface2d(32, 8): the constraint residual of the converged solve is below the stop rule's bound,
    the estimate is the one of tests/test_gpu_spectrum.py (float64 NumPy CG: 62 steps, kappa = 195.11)."""
    p = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    lines = p.stdout.splitlines()
    fields = dict(kv.split("=") for ln in lines for kv in ln.split())
    assert float(fields["constraint_residual"]) <= float(fields["bound"]) and fields["same"] == "1"
    assert fields["converged"] == "1" and 55 <= int(fields["steps"]) <= 70
    assert abs(float(fields["kappa"]) - 195.11) <= 0.01
    assert fields["refused"] == "1"
