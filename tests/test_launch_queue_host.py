"""The launcher thread's queue (pcramp_amd/csrc/pcr_launch_queue.hpp, no HIP in it) under a sanitizer, on the CPU:
tests/launch_queue_check.cpp is compiled as a stand-alone program with -fsanitize=thread (address + undefined where the
toolchain has no working thread-sanitizer runtime) and run.  It checks FIFO order across two producer handles, that
flush returns only when the handle's jobs are done, that a poisoned handle drops its later jobs while the other
handle's still run, and that stop joins the thread.  No sanitizer runtime goes into this Python process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "launch_queue_check.cpp")


def _build_and_run(cxx, flags, exe):
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-pthread"] + flags + ["-o", exe, SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if b.returncode != 0:
        return None, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    return r.returncode, r.stdout


def test_launch_queue_under_a_sanitizer(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    rc, out = _build_and_run(cxx, ["-fsanitize=thread"], str(tmp_path / "check_tsan"))
    which = "thread"
    if rc is None or "FATAL: ThreadSanitizer" in out:
        # no thread-sanitizer runtime here (or one that cannot start on this kernel's address-space layout)
        rc, out = _build_and_run(cxx, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], str(tmp_path / "check_asan"))
        which = "address,undefined"
    print("sanitizer: %s" % which)
    print(out)
    assert rc == 0, out
    assert out.strip().endswith("launch queue ok"), out
    assert "Sanitizer" not in out, out
