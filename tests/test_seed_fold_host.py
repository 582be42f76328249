"""The folded seeds of the position-index scan (pcrhost::orientation_fold_seeds, pcramp_amd/csrc/pcr_host.hpp) under a
sanitizer, on the CPU: tests/seed_fold_check.cpp is compiled as a stand-alone program with -fsanitize=address,undefined
and run.  It checks, exhaustively over every set of at most k mismatching slots, that a window which reaches the floor is
found by some folded seed (lengths 18 ... 25, select thresholds 0.81 / 0.9 / 1.0, every centring; plain oligos and oligos
with 1-3 IUPAC slots), the entries read by plain oligos at 0.9, and that no folded seed sits at an offset above 22.  No
sanitizer runtime goes into this Python process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "seed_fold_check.cpp")


def test_folded_seeds_under_a_sanitizer(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "seed_fold_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("seed fold ok"), r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout


def test_fold_is_exported():
    """The host-only ABI entry beside pcr_host_orientation_seeds: a plain 20-mer at floor 18 folds into 29 seeds that read
    8 runs' worth of entries (27 quarter runs, one whole run, one quarter run)."""
    import numpy as np
    from pcramp_amd import api, words as W
    assert "pcr_host_orientation_fold_seeds" in api.ABI_SYMBOLS
    word = W.centered_word(W.codes_from_text("ACGTTGCAAGCTTGACCATG"))
    sd = api.host_orientation_fold_seeds(word, 18)
    assert sd is not None and len(sd) == 29
    assert sum(hi - lo + 1 for _, _, lo, hi in sd) == 32
    assert max(off for _, off, _, _ in sd) <= 22 and max(code for code, _, _, _ in sd) < (1 << 18)
    assert api.host_orientation_fold_seeds(W.centered_word(W.codes_from_text("ACGTTGCAAGCTTGAC")), 8) is None     # 16-mer, k = 8: no structure
