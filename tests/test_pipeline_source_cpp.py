"""Directional sources through the pipeline and the C++ mirror, driven by a C++11 caller: tests/cpp/test_pipeline_source.cpp sends
eight jobs with a source facing each (rvb_pipeline_submit_directed) through one lane with one pair per launch and through two lanes
with two pairs per launch, and holds every histogram against rvb_set_source_pattern + the step-by-step calls on a separate context,
bit for bit (exact mode); then the refusals, and Raytracer::setSourcePattern through getAllRaw against the C-ABI's records.  Without a
GPU the program must compile, link (plain g++, no HIP headers) and stop at rvb_create: there is no CPU path."""
import os
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "parallel-reverb-raytracer_amd")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "test_pipeline_source")


def _build():
    subprocess.check_call(["make", "-C", PKG, "-j4"], stdout=subprocess.DEVNULL)
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-Wall", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "include", "shims"),
                           os.path.join(ROOT, "tests", "cpp", "test_pipeline_source.cpp"), "-o", BIN, "-L" + PKG, "-lrayverb", "-lrvb_hip",
                           "-Wl,-rpath," + PKG])


def test_source_pattern_caller_compiles_and_links():
    """... and, where there is no GPU, stops at rvb_create (the gpu-marked test runs it where there is one)."""
    import torch
    _build()
    if not torch.cuda.is_available():
        r = subprocess.run([BIN], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 2 and "no CPU path" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_caller_gets_bit_identical_impulse_responses_with_directed_sources():
    _build()
    r = subprocess.run([BIN], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "all source pattern pipeline checks passed" in r.stdout
