"""The growth logic of the library's device buffers (csrc/dev_buf.h: KzvDevBuf of the model handle, KzvScratch of the process
workspaces) under AddressSanitizer and UBSan, on the CPU: tests/host/dev_buf_main.cpp drives both types with a malloc-backed counting
allocator as a stand-alone program, built and run here as a child process (nothing sanitized is loaded into Python)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dev_buf_and_scratch_logic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the buffer logic is tested as a sanitized host program")
    exe = str(tmp_path / "dev_buf_main")
    # the sanitizer runtimes are linked into the program: it runs the same whatever libraries the environment loads ahead of it
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "dev_buf_main.cpp"), "-o", exe, "-pthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dev_buf: ok" in r.stdout
