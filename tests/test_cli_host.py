"""The `pcramp` program (pcramp_amd/bin/pcramp) on every case of tests/golden/cli.json that ends before the design loop: the
reference's quits (usage, unknown switches, missing -o / -t, bad paths, values out of range: no output file, exit 0) and its
ingest errors (unreadable file, illegal base, negative weight: the version / command line / seed lines only, exit 1).  None of
them may touch the GPU, so this runs anywhere."""
import json
import os
import subprocess
import tempfile

import pytest

from cli_cases import materialize

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(os.path.dirname(HERE), "pcramp_amd", "bin", "pcramp")

with open(os.path.join(HERE, "golden", "cli.json")) as _f:
    RUNS = [r for r in json.load(_f)["runs"] if r["stage"] in ("quit", "ingest")]


def run(argv, case=None, timeout=60):
    """(exit status, out.txt bytes or None) of one run in a fresh directory; HIP_VISIBLE_DEVICES hides every GPU, so a run
    that reached for one would fail instead of passing on a machine that has one."""
    with tempfile.TemporaryDirectory() as tmp:
        if case:
            materialize(case, tmp)
        env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
        pr = subprocess.run(argv, executable=EXE, cwd=tmp, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=timeout)
        p = os.path.join(tmp, "out.txt")
        out = open(p, "rb").read().decode("latin-1") if os.path.exists(p) else None
    return pr.returncode, out, pr.stderr.decode("latin-1")


def test_golden_has_host_cases():
    assert os.path.exists(EXE), "pcramp_amd/bin/pcramp was not built"
    assert sum(r["stage"] == "quit" for r in RUNS) >= 15 and sum(r["stage"] == "ingest" for r in RUNS) >= 6


@pytest.mark.parametrize("case", RUNS, ids=[r["name"] for r in RUNS])
def test_reference_run_before_design(case):
    status, out, err = run(case["argv"], case)
    assert status == case["status"], err
    assert (out is not None) == bool(case["exists"])
    if case["exists"]:
        assert out == case["output"]


def test_json_configuration_is_refused():
    # --json / --json.root (the reference's hidden configuration file) are not read: a message, no output file, exit 1
    case = {"input_seed": 1, "pool": dict(n_fam=1, per=2, L=300, div=0.03), "files": [{"path": "t.fa", "records": [{"def": ">a", "seq": 0}]}]}
    for extra in (["--json", "conf.json"], ["--json.root", "a|b"]):
        status, out, err = run(["pcramp", "-t", "t.fa", "-o", "out.txt", "--seed", "1"] + extra, case)
        assert status == 1 and out is None and "json" in err.lower()


def test_time_based_seed_is_written():
    # without --seed the seed is time-based (options.cpp:916-918); the first lines are written before the inputs are read
    status, out, _ = run(["pcramp", "-t", "missing.fa", "-o", "out.txt"])
    assert status == 1
    lines = out.split("\n")
    assert lines[0] == "PCRamp version 0.3" and lines[1] == "Command line: pcramp -t missing.fa -o out.txt" and lines[3] == ""
    assert lines[2].startswith("Random number seed = ") and int(lines[2].split("= ")[1]) > 1_600_000_000
