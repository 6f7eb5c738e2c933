"""The registry that owns a handle's device and pinned memory (nbody-llm_amd/csrc/handle_mem.h), on the CPU: the header is
free of HIP, so tools/sanitize_handle_mem.cpp drives it over a malloc-backed seam that counts calls and fails allocations on
request, under AddressSanitizer (with LeakSanitizer) + UndefinedBehaviorSanitizer.  It checks that release_all frees exactly
the live blocks once, the three growth rules' capacities, failed grows, the keeping grow (a failed copy frees the fresh block
and keeps the old one), the scoped scratch on every exit path, and frees of null and of pointers the registry never held."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_handle_mem_under_sanitizers(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "san_handle_mem"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
           "nbody-llm_amd/csrc", "tools/sanitize_handle_mem.cpp", "-o", str(exe)]
    build = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and "sanitize" in build.stderr:
        pytest.skip("sanitizer runtime not available: " + build.stderr.splitlines()[-1])
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ok" in run.stdout and "ERROR" not in run.stderr and "FAILED" not in run.stdout
