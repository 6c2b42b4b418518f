"""The host-only snapshot validator (muzero.jl_amd/csrc/mz_snap_layout.h, the
checks mz_snapshot_load runs before it touches the engine) under
AddressSanitizer + UBSan on the CPU: tests/sanitize/snap_layout_asan.cpp, a
stand-alone program, feeds it well-formed, truncated and mutated headers, `len`
arrays, flags and counters.  Any sanitizer report fails the run
(-fno-sanitize-recover); nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "sanitize", "snap_layout_asan.cpp")


def test_snapshot_layout_sanitizer_clean(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no host compiler")
    exe = str(tmp_path / "snap_layout_asan")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "snap_layout_asan: 0 failures" in r.stdout, r.stdout
