"""The `pcramp` program (pcramp_amd/bin/pcramp) end to end on the GPU: FASTA files in, the reference's output file out, byte for
byte.  Every run is a fresh child process with argv[0] = "pcramp" in a temporary directory, one at a time.

  - the 24 runs of tests/golden/program.json and the 6 of tests/golden/writers.json (oracle/make_golden.py), their t.fa / b.fa
    written as the reference read them; the runs the reference aborted must fail here too
  - every case of tests/golden/cli.json that reached the design loop (tests/make_golden_cli.py: weights, filters, groups, gzip, ...)
  - a group of several FASTA files reads as one file holding their records in sorted file-name order
  - a gzip-compressed input reads as the plain one

A child that dies by a signal fails its test and no further child is started.  Run with `-m gpu`."""
import json
import os
import subprocess
import tempfile

import pytest

from cli_cases import materialize, program_inputs, write_program_inputs, writers_inputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.join(HERE, "golden")
EXE = os.path.join(os.path.dirname(HERE), "pcramp_amd", "bin", "pcramp")
_died = []                          # the first child that died by a signal


def run(argv, write_inputs, timeout=300):
    """(exit status, out.txt text or None) of one child run in a fresh directory prepared by write_inputs(dir)."""
    if _died:
        pytest.fail("not started: an earlier pcramp child died by signal (%s)" % _died[0])
    assert os.path.exists(EXE), "pcramp_amd/bin/pcramp was not built"
    with tempfile.TemporaryDirectory() as tmp:
        write_inputs(tmp)
        pr = subprocess.run(argv, executable=EXE, cwd=tmp, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        p = os.path.join(tmp, "out.txt")
        out = open(p, "rb").read().decode("latin-1") if os.path.exists(p) else None
    if pr.returncode < 0:
        _died.append("signal %d, %s" % (-pr.returncode, " ".join(argv)))
        pytest.fail("pcramp died by signal %d: %s\n%s" % (-pr.returncode, " ".join(argv), pr.stderr.decode("latin-1")[-2000:]))
    return pr.returncode, out, pr.stderr.decode("latin-1")


def _load(name):
    with open(os.path.join(G, name)) as f:
        return json.load(f)


PROGRAM = _load("program.json")["runs"]
WRITERS = _load("writers.json")["runs"]
CLI = [r for r in _load("cli.json")["runs"] if r["stage"] == "design"]


@pytest.mark.parametrize("ri", range(len(PROGRAM)))
def test_program_runs(ri):
    run_ = PROGRAM[ri]
    targets, bgs = program_inputs(run_)
    assert [[d, len(q)] for d, q in targets] == run_["targets"] and [[d, len(q)] for d, q in bgs] == run_["backgrounds"]
    status, out, err = run(run_["argv"], lambda d: write_program_inputs(d, targets, bgs))
    if run_["aborted"]:
        assert status != 0, "the reference aborted this run"
        return
    assert status == 0, err[-2000:]
    assert out == run_["output"]


@pytest.mark.parametrize("ri", range(len(WRITERS)))
def test_writers_runs(ri):
    run_ = WRITERS[ri]
    targets, bgs = writers_inputs(ri)
    assert [[d, len(q)] for d, q in targets] == run_["targets"] and [[d, len(q)] for d, q in bgs] == run_["backgrounds"]
    status, out, err = run(run_["argv"], lambda d: write_program_inputs(d, targets, bgs))
    assert status == 0, err[-2000:]
    assert out == run_["output"]


def test_replay_counts():
    assert len(PROGRAM) == 24 and len(WRITERS) == 6 and len(CLI) >= 20


@pytest.mark.parametrize("case", CLI, ids=[r["name"] for r in CLI])
def test_cli_cases(case):
    status, out, err = run(case["argv"], lambda d: materialize(case, d))
    assert status == case["status"], err[-2000:]
    assert out == case["output"]


POOL = dict(n_fam=2, per=4, L=500, div=0.03)
ARGS = ["--thread", "1", "--count", "2", "--trial", "20", "--seed", "5"]


def _case(files):
    return {"input_seed": 8, "pool": POOL, "files": files}


def test_multi_file_group_is_its_files_in_sorted_order():
    recs = [{"def": ">r%d" % i, "seq": i} for i in range(7)]
    split = _case([{"path": "T/g/b.fa", "records": recs[2:4], "width": 60}, {"path": "T/g/a.fa", "records": recs[0:2]},
                   {"path": "T/g/c.fna.gz", "records": recs[4:6]}, {"path": "T/h/x.fa", "records": recs[6:]},
                   {"path": "T/g/d.fasta", "records": [{"def": ">too short", "seq": {"of": 0, "to": 40}}]}])
    joined = _case([{"path": "T/g/all.fa", "records": recs[0:6]}, {"path": "T/h/x.fa", "records": recs[6:]}])
    argv = ["pcramp", "-T", "T", "-o", "out.txt"] + ARGS
    s1, o1, e1 = run(argv, lambda d: materialize(split, d))
    s2, o2, e2 = run(argv, lambda d: materialize(joined, d))
    assert s1 == 0 and s2 == 0, e1[-2000:] + e2[-2000:]
    assert "target sequence summary Number of sequences = 2" in o1
    assert o1 == o2


def test_gzip_input_reads_as_plain():
    recs = [{"def": ">r%d [w=%d]" % (i, 1 + i % 3), "seq": i} for i in range(6)]
    for argv in (["pcramp", "-T", "T", "-o", "out.txt"] + ARGS, ["pcramp", "-T", "T", "--o.json", "-o", "out.txt"] + ARGS):
        outs = []
        for name in ("T/g/x.fa", "T/g/x.fa.gz"):
            case = _case([{"path": name, "records": recs, "width": 61}, {"path": name.replace("/g/", "/h/"), "records": recs[:3]}])
            status, out, err = run(argv, lambda d: materialize(case, d))
            assert status == 0, err[-2000:]
            outs.append(out)
        assert outs[0] == outs[1]
