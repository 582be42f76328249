"""The design loop in the reference's MPI mode (pcr_design with pcr_design_trial_ranks): every rank holds the whole sets, draws
its share of the trials from `seed + rank`, and the ranks' best assays are reduced to one winner per iteration.
tests/golden/program_mpi.json holds whole output files of the reference under `mpiexec -n <world>` (tests/make_golden_mpi.py);
every rank must leave that file byte for byte, and the same pool.

Every rank is a fresh child process (this file run as a script on a JSON spec) with a time limit; the ranks of a world share the
one GPU through the host-collective communicator over gloo, and world 1 exercises RCCL.  The parent never opens the GPU; at most
four children have it open at a time."""
import json
import os
import random
import socket
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CHILD_TIMEOUT = 900
PCR_ERR_ARG, PCR_ERR_STATE = -1, -3


def _mpi_runs():
    with open(os.path.join(G, "program_mpi.json")) as f:
        return json.load(f)["runs"]


def _program_runs():
    with open(os.path.join(G, "program.json")) as f:
        return json.load(f)["runs"]


def _inputs(run):
    """(targets [(defline, text)], backgrounds) of a program.json / program_mpi.json run, regenerated from its seeds."""
    from testdata import mutate, rand_seq
    sp, r2 = run["spec"], random.Random(run["input_seed"])
    roots = [rand_seq(r2, sp["L"] + 7 * k) for k in range(sp["n_fam"])]
    targets = [(">target_%d family %d" % (k * sp["per"] + j, k), mutate(r2, roots[k], sp["div"])) for k in range(sp["n_fam"]) for j in range(sp["per"])]
    bgs = [(">bg_%d" % i, mutate(r2, roots[i % len(roots)], sp["bg_div"])) for i in range(sp["n_bg"])]
    return targets, bgs


# ------------------------------------------------------------------------------------------------ child side
def _child(spec):
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)
    import datetime
    import torch.distributed as dist
    from pcramp_amd import api, design, shard

    world, rank = spec.get("world", 1), spec.get("rank", 0)
    if spec.get("comm") == "gloo":
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % spec["port"], world_size=world, rank=rank,
                                timeout=datetime.timedelta(seconds=300))
    out = {"results": []}
    d0 = api.Screener(0)                                                # (owns the communicator)
    comm = None
    try:
        if spec.get("comm") == "gloo":
            comm = d0.comm_init_host(world, rank, shard.gloo_allgather())
        elif spec.get("comm") == "rccl":
            comm = d0.comm_init_rank(api.Screener.comm_unique_id(), 1, 0)
        for job in spec["jobs"]:
            run = _mpi_runs()[job["ri"]] if job["src"] == "mpi" else _program_runs()[job["ri"]]
            targets, bgs = _inputs(run)
            texts = [q for _, q in targets]
            if job.get("alter_rank") == rank:                          # one base of one target differs on this rank
                texts[3] = ("A" if texts[3][0] != "A" else "C") + texts[3][1:]
            d = api.Screener(0)                                         # a fresh handle per job (sets, multiplex DB)

            def load(rows=(0, len(texts))):
                d.load_texts(texts[rows[0]:rows[1]], [1.0] * (rows[1] - rows[0]))
                if bgs:
                    d.load_texts([q for _, q in bgs], [1.0] * len(bgs), which=api.BACKGROUND)

            def run_design(argv, trial_world, trial_delta=0):
                o = design.options_from_argv(argv, world=trial_world)
                o["num_trial"] += trial_delta
                text, pool = design.design(d, [x for x, _ in targets], [len(q) for _, q in targets], [x for x, _ in bgs],
                                           [len(q) for _, q in bgs], argv=argv, **o)
                return {"rc": 0, "text": text.decode("latin-1"), "pool": [["%x" % x for p in q for x in p] for q in pool]}

            res = {}
            try:
                mode = job.get("mode", "design")
                if mode == "shard_then_trials":
                    n = len(texts)
                    lo, hi = (0, n // 2) if rank == 0 else (n // 2, n)
                    load((lo, hi))
                    d.shard_targets(comm, lo, n)
                    d.design_trial_ranks(comm)
                elif mode == "trials_then_shard":
                    load()
                    d.design_trial_ranks(comm)
                    d.shard_targets(comm, 0, len(texts))
                else:
                    load()
                    d.design_trial_ranks(comm)
                    res["world"] = d.design_trial_world()
                    argv = list(run["argv"]) + (job.get("argv_extra", []) if job.get("differ_rank") == rank else [])
                    if mode == "detach_first":                          # attached and detached without a design in between
                        d.design_trial_ranks(None)
                        res["world_after"] = d.design_trial_world()
                        res.update(run_design(argv, 1))
                    else:
                        res.update(run_design(argv, world, job.get("trial_delta", 0) if job.get("differ_rank") == rank else 0))
                        if mode == "then_one_rank":                     # detach, the sets as loaded, the one-rank design
                            d.design_trial_ranks(None)
                            res["world_after"] = d.design_trial_world()
                            load()
                            one = run_design(list(_program_runs()[job["one_rank_ri"]]["argv"]), 1)
                            res["one_rank_text"] = one["text"]
            except api.PcrError as e:
                res.update({"rc": e.rc, "msg": str(e)})
            d.close()
            out["results"].append(res)
    finally:
        if comm is not None:
            d0.comm_destroy(comm)
        d0.close()
        if spec.get("comm") == "gloo":
            dist.destroy_process_group()
    return out


# ------------------------------------------------------------------------------------------------ parent side
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(specs):
    """Start one child per spec (they are the ranks of one run), wait with a time limit, return their outputs."""
    assert len(specs) <= 4
    tmp = tempfile.mkdtemp(prefix="pcramp_trial_ranks_")
    procs = []
    for k, spec in enumerate(specs):
        sp, op = os.path.join(tmp, "spec%d.json" % k), os.path.join(tmp, "out%d.json" % k)
        with open(sp, "w") as f:
            json.dump(spec, f)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), sp, op]
        procs.append((subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT), op))
    outs = []
    try:
        for p, op in procs:
            try:
                log, _ = p.communicate(timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                for q, _ in procs:
                    q.kill()
                raise AssertionError("a rank did not finish within %d s" % CHILD_TIMEOUT)
            log = log.decode(errors="replace")
            assert p.returncode == 0, "rank exited with %d:\n%s" % (p.returncode, log[-4000:])
            with open(op) as f:
                outs.append(json.load(f))
    finally:
        for q, _ in procs:
            if q.poll() is None:
                q.kill()
    return outs


def _world(world, jobs, comm="gloo"):
    """The same job list on every rank of a world of `world` ranks."""
    port = _free_port()
    return _run([{"world": world, "rank": r, "port": port, "comm": comm, "jobs": jobs} for r in range(world)])


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("world", [2, 3, 4])
def test_reference_mpi_runs(world):
    """Every program_mpi.json run at this world over gloo: every rank's text equals the reference's file byte for byte and every
    rank holds the same pool; an aborted run returns the same nonzero code on every rank."""
    runs = [(k, r) for k, r in enumerate(_mpi_runs()) if r["world"] == world]
    assert len(runs) >= 5
    outs = _world(world, [{"src": "mpi", "ri": k} for k, _ in runs])
    for j, (k, g) in enumerate(runs):
        res = [outs[r]["results"][j] for r in range(world)]
        assert all(x.get("world") == world for x in res), (k, res[0])
        if g["aborted"]:
            assert res[0]["rc"] != 0 and all(x["rc"] == res[0]["rc"] for x in res), (k, res)
            continue
        for r in range(world):
            assert res[r]["rc"] == 0, (k, r, res[r].get("msg"))
            assert res[r]["text"] == g["output"], (k, r, g["argv"])
        assert all(x["pool"] == res[0]["pool"] for x in res)


def test_world1_rccl_equals_one_rank():
    """World 1 over RCCL with trial ranks attached is the one-rank program: program.json's text for several runs (text, JSON,
    the top-down start, the 5' / 3' moves, TaqMAMA, an aborted run)."""
    prog = _program_runs()
    picks = [0, 1, 2, 4, 5, 16, 20]
    assert prog[20].get("aborted")
    res = _run([{"world": 1, "rank": 0, "comm": "rccl", "jobs": [{"src": "program", "ri": ri} for ri in picks]}])[0]["results"]
    for ri, x in zip(picks, res):
        assert x.get("world") == 1, (ri, x)
        if prog[ri].get("aborted"):
            assert x["rc"] != 0, ri
            continue
        assert x["rc"] == 0, (ri, x.get("msg"))
        assert x["text"] == prog[ri]["output"], ri


def test_detach_leaves_nothing_behind():
    """World 2 over gloo: after a design with trial ranks and a detach, the same handle designs as one rank does (program.json);
    attaching and detaching without a design in between changes nothing either.  The world-2 text itself differs from the one-rank
    text, so the attachment is what made the difference."""
    mpi, prog = _mpi_runs(), _program_runs()
    k = next(i for i, r in enumerate(mpi) if r["world"] == 2 and r["program_run"] == 0 and r["argv"] == prog[0]["argv"])
    assert mpi[k]["output"] != prog[0]["output"]
    jobs = [{"src": "mpi", "ri": k, "mode": "then_one_rank", "one_rank_ri": 0}, {"src": "program", "ri": 3, "mode": "detach_first"}]
    outs = _world(2, jobs)
    for r in range(2):
        a, b = outs[r]["results"]
        assert a["rc"] == 0 and b["rc"] == 0, (r, a.get("msg"), b.get("msg"))
        assert a["world"] == 2 and a["world_after"] == 0 and b["world_after"] == 0
        assert a["text"] == mpi[k]["output"]
        assert a["one_rank_text"] == prog[0]["output"]
        assert b["text"] == prog[3]["output"]


def test_refusals_on_every_rank():
    """Sets that differ on one rank (attach), a different num_trial or command line on one rank (pcr_design): PCR_ERR_ARG on every
    rank.  Trial ranks with a target shard, in either order: PCR_ERR_STATE on every rank.  No rank hangs."""
    k = next(i for i, r in enumerate(_mpi_runs()) if r["world"] == 2 and not r["aborted"])
    jobs = [{"src": "mpi", "ri": k, "alter_rank": 1},
            {"src": "mpi", "ri": k, "differ_rank": 1, "trial_delta": 1},
            {"src": "mpi", "ri": k, "differ_rank": 0, "argv_extra": ["--seed", "43"]},
            {"src": "mpi", "ri": k, "mode": "shard_then_trials"},
            {"src": "mpi", "ri": k, "mode": "trials_then_shard"}]
    outs = _world(2, jobs)
    for r in range(2):
        res = outs[r]["results"]
        assert [x["rc"] for x in res] == [PCR_ERR_ARG] * 3 + [PCR_ERR_STATE] * 2, (r, res)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with open(sys.argv[1]) as f:
        spec = json.load(f)
    result = _child(spec)
    with open(sys.argv[2], "w") as f:
        json.dump(result, f)
