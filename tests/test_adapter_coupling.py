"""System::update_coupling of include/alfd/dealii_adapter.hpp (the call site of a time loop whose immersed body moves over
a fixed background mesh) compiled against the mock deal.II classes (tests/adapter/coupling_demo.cpp) and driven once on
the GPU: the updated System solves the moved problem to the bits of a System that uploaded it from scratch."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, "fictitious_domain_al_preconditioners_amd", "lib")


@pytest.fixture(scope="module")
def demo(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("adapter_coupling") / "coupling_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "adapter", "coupling_demo.cpp"), "-L" + LIB, "-lalfd",
                           "-lalfd_synth", "-Wl,-rpath," + LIB, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_update_coupling_compiles_and_fails_loudly_without_gpu(demo):
    """Without a device the first System cannot be created: alfd_create -> ALFD_E_HIP -> Error, exit code 3."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    p = subprocess.run([demo], capture_output=True, text=True, timeout=120)
    assert p.returncode == 3, (p.returncode, p.stderr)
    assert "alfd_create" in p.stderr


@pytest.mark.gpu
def test_update_coupling_on_the_gpu(demo):
    """laplace2d_circle(32, 3), the circle moved from (0.4, 0.4) to (0.43, 0.38): same counts and the same solution bits
    as the fresh System from the same initial guess; the update forms no product with A and uploads no transfer (there is
    no hierarchy: one power iteration for lambda_max); an update after a new A is refused and setup() repairs it."""
    p = subprocess.run([demo], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    fields = {}
    for ln in p.stdout.splitlines():
        words = ln.split()
        if words[0] == "updated":
            i = words.index("fresh")
            fields["updated"], fields["fresh"] = words[1:i], words[i + 1:i + 3]
            words = words[i + 3:]
        fields.update(kv.split("=") for kv in words)
    assert fields["updated"] == fields["fresh"] and fields["same"] == "1", p.stdout
    assert int(fields["updated"][0].split("=")[1]) > 0
    assert (fields["products_a"], fields["transfer_uploads"], fields["power_iterations"]) == ("0", "0", "1"), p.stdout
    assert fields["refused"] == "1"
