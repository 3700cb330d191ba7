"""The bookkeeping of the deferred folds (csrc/fold_queue.h: the queue behind KzvLnDeferScope and KzvTnFoldScope) under AddressSanitizer
and UBSan, on the CPU: tests/host/fold_queue_main.cpp drives it with a recording fake fold at both capacities (63 and 5 pending entries)
as a stand-alone program, built and run here as a child process (nothing sanitized is loaded into Python)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_queue_logic_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found: the fold queue is tested as a sanitized host program")
    exe = str(tmp_path / "fold_queue_main")
    # the sanitizer runtimes are linked into the program: it runs the same whatever libraries the environment loads ahead of it
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tests", "host", "fold_queue_main.cpp"), "-o", exe, "-pthread"]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fold_queue: ok" in r.stdout
