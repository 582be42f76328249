"""The pairs of the launcher thread's queue (pcramp_amd/csrc/pcr_launch_queue.hpp, no HIP in it) under a sanitizer, on the
CPU, as test_launch_queue_host.py does for the queue itself: tests/launch_queue_pair_check.cpp is compiled as a
stand-alone program and run.  It checks which jobs pair in an A B C A B C A sequence of three owners, that a held job is
released by its owner's flush, by the owner's rule, by the time cap and by stop(), that a successor that cannot pair
leaves the order of launches the order of the pushes, and that a failed pair poisons both owners."""
import shutil

import test_launch_queue_host as Q


def test_launch_queue_pairs_under_a_sanitizer(tmp_path, monkeypatch):
    monkeypatch.setattr(Q, "SRC", Q.os.path.join(Q.ROOT, "tests", "launch_queue_pair_check.cpp"))
    cxx = shutil.which(Q.os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    rc, out = Q._build_and_run(cxx, ["-fsanitize=thread"], str(tmp_path / "pair_tsan"))
    if rc is None or "FATAL: ThreadSanitizer" in out:
        rc, out = Q._build_and_run(cxx, ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], str(tmp_path / "pair_asan"))
    print(out)
    assert rc == 0, out
    assert out.strip().endswith("launch queue pairs ok"), out
    assert "Sanitizer" not in out, out
