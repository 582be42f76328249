"""The host side of the reference's MPI mode: how the reference divides --trial over its tasks (main.cpp:65), and -- where the
reference binary was built (oracle/_ref/pcramp) with the MPICH it links against -- that tests/golden/program_mpi.json is what the
reference writes under `mpiexec` today.  No GPU."""
import json
import os
import tempfile

import pytest

from pcramp_amd import design

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")


def reference_division(num_trial, world):
    """main.cpp:65 in unsigned arithmetic: max(1u, num_trial/N + (num_trial%N == 0 ? 0u : 1u))"""
    return max(1, num_trial // world + (0 if num_trial % world == 0 else 1))


def test_trials_per_rank_is_the_reference_division():
    for world in range(1, 9):
        for num_trial in list(range(0, 70)) + [999, 1000, 1001, 4096, (1 << 20)]:
            assert design.trials_per_rank(num_trial, world) == reference_division(num_trial, world), (num_trial, world)
    with pytest.raises(ValueError):
        design.trials_per_rank(10, 0)


def test_options_from_argv_world():
    argv = ["pcramp", "-t", "t.fa", "-o", "out.txt", "--count", "4", "--trial", "30", "--seed", "11"]
    assert design.options_from_argv(argv)["num_trial"] == 30
    assert design.options_from_argv(argv, world=1)["num_trial"] == 30
    assert design.options_from_argv(argv, world=4)["num_trial"] == 8
    assert design.options_from_argv(argv, world=64)["num_trial"] == 1
    assert design.options_from_argv(argv, world=4)["seed"] == 11                    # every rank is given the same seed
    assert design.options_from_argv(["pcramp"], world=3)["num_trial"] == reference_division(design.DEFAULTS["num_trial"], 3)
    with open(os.path.join(G, "program_mpi.json")) as f:
        runs = json.load(f)["runs"]
    for run in runs:
        o = design.options_from_argv(run["argv"], world=run["world"])
        n = int(run["argv"][run["argv"].index("--trial") + 1])
        assert o["num_trial"] == reference_division(n, run["world"]) and o["seed"] == run["seed"]


def test_golden_covers_the_cases():
    with open(os.path.join(G, "program_mpi.json")) as f:
        doc = json.load(f)
    runs = doc["runs"]
    worlds = [r["world"] for r in runs]
    assert worlds.count(2) >= 24 and worlds.count(3) >= 6 and worlds.count(4) >= 4
    trials = [(int(r["argv"][r["argv"].index("--trial") + 1]), r["world"]) for r in runs]
    assert any(n < w for n, w in trials)
    assert sum(1 for n, w in trials if n % w) >= 3
    assert any(r["world"] == 3 and r["json"] and not r["aborted"] for r in runs)
    assert "dropped" in doc
    assert os.path.getsize(os.path.join(G, "program_mpi.json")) < 300 * 1024


def _reference_here():
    import make_golden_mpi as M
    return os.path.exists(M.EXE) and os.path.exists(M.MPIEXEC)


@pytest.mark.skipif(not _reference_here(), reason="the reference binary (oracle/_ref/pcramp) or its mpiexec is not on this machine")
def test_reference_still_writes_the_golden():
    """Three program_mpi.json cases (worlds 2, 3 and 4) re-run through mpiexec exactly as tests/make_golden_mpi.py runs them."""
    import make_golden_mpi as M
    with open(os.path.join(G, "program_mpi.json")) as f:
        runs = json.load(f)["runs"]
    picks = []
    for world in (2, 3, 4):
        picks.append(next(r for r in runs if r["world"] == world and not r["aborted"]))
    with tempfile.TemporaryDirectory() as tmp:
        libdir = os.path.join(tmp, "lib")
        os.makedirs(libdir)
        for so in ("libmpi.so.12", "libgfortran.so.4", "libquadmath.so.0"):
            os.symlink(os.path.join("/opt/conda/lib", so), os.path.join(libdir, so))
        env = dict(os.environ, LD_LIBRARY_PATH=libdir, OMP_NUM_THREADS="1")
        for run in picks:
            targets, bgs = M.inputs(run["spec"], run["input_seed"])
            with open(os.path.join(tmp, "t.fa"), "w") as f:
                f.write("".join("%s\n%s\n" % (d, q) for d, q in targets))
            if bgs:
                with open(os.path.join(tmp, "b.fa"), "w") as f:
                    f.write("".join("%s\n%s\n" % (d, q) for d, q in bgs))
            out, aborted, _ = M.run_once(tmp, env, run["world"], run["argv"])
            assert not aborted, run["argv"]
            assert out == run["output"], (run["world"], run["argv"])
