"""The Krylov workspace (faspsolver_amd/csrc/krylov_ws.h) owns its memory: its growth and free logic, instantiated over
malloc / free in the stand-alone program tests/krylov_ws_check.cpp, built with AddressSanitizer and UBSan and run on the CPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_krylov_ws_host_check(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "krylov_ws_check")
    subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "faspsolver_amd", "csrc"), os.path.join(ROOT, "tests", "krylov_ws_check.cpp"),
                    "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "krylov_ws_check ok" in out.stdout
