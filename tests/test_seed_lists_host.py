"""The seed lists of a screen pass (pcrseed::list_seeds / plan_slices, pcramp_amd/csrc/pcr_seed_lists.hpp) under a sanitizer, on
the CPU: tests/seed_lists_check.cpp is compiled as a stand-alone program with -fsanitize=address,undefined and run.  It carries
the listing loops and the merge walk that the header replaced, written with std::vector, and requires byte equality of every
output over a chain of passes that share their caches: lengths 18 ... 25 at four thresholds, IUPAC slots, one pair, several
groups in both modes, repeated / replaced / swapped / resized batches (the positional memo), the cache-clear threshold crossed
between and inside passes, five index generations, degenerate run tables, every false return, fold on and off.  No sanitizer
runtime goes into this Python process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "seed_lists_check.cpp")


def test_seed_lists_under_a_sanitizer(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "seed_lists_check")
    b = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert b.returncode == 0, b.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert r.stdout.strip().endswith("seed lists ok"), r.stdout
    assert "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout


def test_listing_header_has_no_hip():
    """The header stands alone: the check program above includes nothing else of the library but pcr_host.hpp through it."""
    text = open(os.path.join(ROOT, "pcramp_amd", "csrc", "pcr_seed_lists.hpp")).read()
    assert "hip/" not in text and "__global__" not in text and "__device__" not in text
