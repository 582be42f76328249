"""The owners of a handle's HIP resources (pcramp_amd/csrc/pcr_owned.hpp) under a sanitizer, on the CPU:
tests/owned_check.cpp is compiled as a stand-alone program over malloc-backed fakes of the HIP entry points the header
calls, with -fsanitize=address,undefined, and run.  It checks what ensure / ensure_slack / release allocate and free and
when `generation` moves, a failed allocation, the moves, that a borrowed stream is never destroyed and an owned one once,
a growing vector of event pairs, and that in the end the four live counters are zero and every block was freed exactly
once.  No sanitizer runtime goes into this Python process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "owned_check.cpp")


def test_owner_types_under_a_sanitizer(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "owned_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("owned ok"), r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout
