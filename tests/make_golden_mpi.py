"""Writes tests/golden/program_mpi.json: whole runs of the reference PROGRAM in its MPI mode (`mpiexec -n N pcramp ...`), the
form of distribution its users run (main.cpp:60-113, :926-927, :1420-1601).  A script, not a test: run it where the reference
binary exists (oracle/_ref/pcramp, made by __graft_entry__.build()) and the MPICH it was linked against is installed.

The inputs are those of tests/golden/program.json (oracle/make_golden.py::program_golden), regenerated from their seeds with
tests/testdata.py, at worlds 2, 3 and 4, plus a few --trial values chosen so that the world does not divide them or exceeds
them.  Every case runs three times and is kept only if all runs write the same bytes (the reference's root takes the ranks' records in
arrival order, which can matter on an exact tie); the file says how many were dropped.  tests/test_gpu_design_trial_ranks.py
replays the runs through pcr_design with trial ranks attached.

    python tests/make_golden_mpi.py
"""
import json
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from testdata import mutate, rand_seq  # noqa: E402

EXE = os.path.join(ROOT, "oracle", "_ref", "pcramp")
MPIEXEC = "/opt/conda/bin/mpiexec"
OUT = os.path.join(HERE, "golden", "program_mpi.json")
REPEATS = 3          # runs of every case; kept only if all write the same bytes


def inputs(spec, input_seed):
    """(targets, backgrounds) as [(defline, text)], as program_golden made them."""
    r2 = random.Random(input_seed)
    roots = [rand_seq(r2, spec["L"] + 7 * k) for k in range(spec["n_fam"])]
    targets = [(">target_%d family %d" % (k * spec["per"] + j, k), mutate(r2, roots[k], spec["div"]))
               for k in range(spec["n_fam"]) for j in range(spec["per"])]
    bgs = [(">bg_%d" % i, mutate(r2, roots[i % len(roots)], spec["bg_div"])) for i in range(spec["n_bg"])]
    return targets, bgs


def with_trial(argv, n):
    a = list(argv)
    a[a.index("--trial") + 1] = str(n)
    return a


def cases(program_runs):
    """(program.json run index, world, argv) of every case."""
    out = [(ri, 2, run["argv"]) for ri, run in enumerate(program_runs)]
    # (runs 6, 7, 10, 15, 18 and 23 tie exactly at worlds 3 or 4, so that their output follows the arrival order at the reference's
    # root and changed between repeated runs: they are left out there)
    out += [(ri, 3, program_runs[ri]["argv"]) for ri in (0, 1, 2, 3, 4, 9, 13, 19)]      # 1, 9 and 19 write JSON
    out += [(ri, 4, program_runs[ri]["argv"]) for ri in (0, 2, 4, 5, 12, 16)]
    # --trial below the world, and values the world does not divide
    out += [(0, 4, with_trial(program_runs[0]["argv"], 3)), (5, 3, with_trial(program_runs[5]["argv"], 2)),
            (3, 2, with_trial(program_runs[3]["argv"], 31)), (1, 3, with_trial(program_runs[1]["argv"], 29)),
            (13, 4, with_trial(program_runs[13]["argv"], 37))]
    return out


def run_once(tmp, env, world, argv):
    for name in ("out.txt",):
        p = os.path.join(tmp, name)
        if os.path.exists(p):
            os.remove(p)
    cmd = ["timeout", "-k", "10", "300", MPIEXEC, "-launcher", "fork", "-hosts", "localhost", "-iface", "lo", "-n", str(world), EXE] + argv[1:]
    pr = subprocess.run(cmd, cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    # as program_golden: a `throw` inside the reference's OpenMP regions ends the program, its buffered output file lost
    aborted = pr.returncode != 0
    out = ""
    if not aborted:
        with open(os.path.join(tmp, "out.txt"), "rb") as f:
            out = f.read().decode("latin-1").replace(EXE, "pcramp")
    return out, int(aborted), pr.stderr.decode("latin-1")[-160:] if aborted else ""


def main():
    if not os.path.exists(EXE) or not os.path.exists(MPIEXEC):
        sys.exit("make_golden_mpi: needs %s (build()) and %s" % (EXE, MPIEXEC))
    with open(os.path.join(HERE, "golden", "program.json")) as f:
        program_runs = json.load(f)["runs"]
    runs, dropped = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        libdir = os.path.join(tmp, "lib")
        os.makedirs(libdir)
        for so in ("libmpi.so.12", "libgfortran.so.4", "libquadmath.so.0"):
            os.symlink(os.path.join("/opt/conda/lib", so), os.path.join(libdir, so))
        env = dict(os.environ, LD_LIBRARY_PATH=libdir, OMP_NUM_THREADS="1")
        for ri, world, argv in cases(program_runs):
            base = program_runs[ri]
            targets, bgs = inputs(base["spec"], base["input_seed"])
            with open(os.path.join(tmp, "t.fa"), "w") as f:
                f.write("".join("%s\n%s\n" % (d, q) for d, q in targets))
            if bgs:
                with open(os.path.join(tmp, "b.fa"), "w") as f:
                    f.write("".join("%s\n%s\n" % (d, q) for d, q in bgs))
            first = run_once(tmp, env, world, argv)
            if any(run_once(tmp, env, world, argv)[:2] != first[:2] for _ in range(REPEATS - 1)):
                dropped += 1
                print("dropped: run", ri, "world", world, argv[7:])
                continue
            out, aborted, tail = first
            runs.append({"argv": argv, "world": world, "seed": base["seed"], "json": base["json"], "input_seed": base["input_seed"],
                         "spec": base["spec"], "program_run": ri, "output": out, "aborted": aborted, "stderr_tail": tail})
            print("run", ri, "world", world, argv[7:], "->", "aborted" if aborted else
                  "%d assays" % (out.count("ASSAY.") + out.count('"forward primer"')))
    doc = {"note": "the reference program under `mpiexec -n <world>`, one thread per rank; every case ran %d times and is kept only "
                   "if all outputs are byte-identical (tests/make_golden_mpi.py)" % REPEATS,
           "dropped": dropped, "runs": runs}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=0)
        f.write("\n")
    print("%d runs, %d dropped -> %s (%d bytes)" % (len(runs), dropped, OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
