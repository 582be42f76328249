"""The design loop over targets sharded across ranks (pcr_design with pcr_shard_targets + pcr_shard_sampler_targets), and the
gather of rank-local bitsets at arbitrary boundaries (pcr_shard_gather_bits).  Every golden program run, with its targets cut
at a boundary inside the list, must leave on every rank the reference's output file byte for byte, and the same pool.

Every rank is a fresh child process (this file run as a script on a JSON spec) with a time limit; two or three ranks share the
one GPU through the host-collective communicator over gloo, one rank exercises RCCL.  The parent never opens the GPU; at most
three children have it open at a time."""
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

# the input specs of oracle/make_golden.py::writers_golden, by run index (as test_gpu_design_program.py)
WRITER_SPECS = [dict(n_fam=3, per=4, L=600, n_bg=2), dict(n_fam=3, per=4, L=600, n_bg=2), dict(n_fam=1, per=4, L=500, n_bg=0),
                dict(n_fam=1, per=4, L=500, n_bg=0), dict(n_fam=2, per=3, L=451, n_bg=3), dict(n_fam=2, per=3, L=451, n_bg=3)]


def _inputs(src, ri):
    """(run, targets [(defline, text)], backgrounds) of writers.json / program.json run ri, inputs regenerated from their seeds."""
    from testdata import mutate, rand_seq
    if src == "writers":
        with open(os.path.join(G, "writers.json")) as f:
            run = json.load(f)["runs"][ri]
        sp, r2, div, bg_div = WRITER_SPECS[ri], random.Random(6000 + ri // 2), 0.03, 0.12
    else:
        with open(os.path.join(G, "program.json")) as f:
            run = json.load(f)["runs"][ri]
        sp = run["spec"]
        r2, div, bg_div = random.Random(run["input_seed"]), sp["div"], sp["bg_div"]
    roots = [rand_seq(r2, sp["L"] + 7 * k) for k in range(sp["n_fam"])]
    targets = [(">target_%d family %d" % (k * sp["per"] + j, k), mutate(r2, roots[k], div)) for k in range(sp["n_fam"]) for j in range(sp["per"])]
    bgs = [(">bg_%d" % i, mutate(r2, roots[i % len(roots)], bg_div)) for i in range(sp["n_bg"])]
    return run, targets, bgs


def _synth_case():
    """About 2 000 targets x 2 kb (families of 50), a few hundred trials, 3 iterations."""
    from pcramp_amd import synth, words as W
    packed, off, lens = synth.make_sequences(2000, 2000, 4242, family=50)
    texts = []
    for i in range(len(lens)):
        codes = synth.sequence_codes(packed, off, lens, i)
        texts.append(W.text_from_codes(codes))
    targets = [(">synth_%d" % i, t) for i, t in enumerate(texts)]
    argv = ["pcramp", "-t", "t.fa", "-o", "out.txt", "--count", "3", "--trial", "300", "--seed", "1234"]
    return {"argv": argv, "json": 0}, targets, []


# ------------------------------------------------------------------------------------------------ child side
def _child(spec):
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)
    import datetime
    import numpy as np
    import torch.distributed as dist
    from pcramp_amd import api, design, shard

    world, rank = spec.get("world", 1), spec.get("rank", 0)
    if spec.get("comm") == "gloo":
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % spec["port"], world_size=world, rank=rank,
                                timeout=datetime.timedelta(seconds=300))
    out = {"results": []}
    d0 = d = api.Screener(0)                                            # (owns the communicator and serves the gathers)
    comm = None
    try:
        if spec.get("comm") == "gloo":
            comm = d0.comm_init_host(world, rank, shard.gloo_allgather())
        elif spec.get("comm") == "rccl":
            comm = d0.comm_init_rank(api.Screener.comm_unique_id(), 1, 0)
        for job in spec["jobs"]:
            res = {}
            if job.get("env") is not None:
                os.environ["PCRAMP_SHARD_COMBINE"] = job["env"]
            if job["kind"] == "gather":
                d = d0
                n_total, n_vec, bounds = job["n_total"], job["n_vec"], job["bounds"]
                lo, hi = bounds[rank], bounds[rank + 1]
                d.load_texts(["ACGT" * 10] * (hi - lo))
                d.shard_targets(comm, lo, n_total)
                rng = np.random.default_rng(job["seed"])
                full = rng.integers(0, 2, size=(n_vec, n_total), dtype=np.uint8)      # the same on every rank
                lw, gw = (hi - lo + 63) // 64 + job.get("extra", 0), (n_total + 63) // 64 + 1
                local = np.zeros((n_vec, lw * 64), np.uint8)
                local[:, :hi - lo] = full[:, lo:hi]
                local[:, hi - lo:] = rng.integers(0, 2, size=(n_vec, lw * 64 - (hi - lo)), dtype=np.uint8)   # garbage past n
                lwords = np.packbits(local, axis=1, bitorder="little").view(np.uint64).copy()
                d_local = torch.from_numpy(lwords.view(np.int64)).to("cuda:0")
                d_global = torch.full((n_vec, gw), -1, dtype=torch.int64, device="cuda:0")
                try:
                    if job.get("bad_rank") == rank:
                        d.shard_gather_bits(d_local, n_vec, 0, d_global, gw)              # stride below the word count
                    else:
                        d.shard_gather_bits(d_local, n_vec, lw, d_global, gw)
                    got = d_global.cpu().numpy().view(np.uint64)
                    want = np.zeros((n_vec, gw * 64), np.uint8)
                    want[:, :n_total] = full
                    res["ok"] = bool((got == np.packbits(want, axis=1, bitorder="little").view(np.uint64)).all())
                    res["rc"] = 0
                except api.PcrError as e:
                    res["rc"], res["msg"] = e.rc, str(e)
                d.shard_targets(None, 0, 0)
                out["results"].append(res)
                continue
            if job["src"] == "synth":
                run, targets, bgs = _synth_case()
            else:
                run, targets, bgs = _inputs(job["src"], job["ri"])
            n = len(targets)
            lo, hi = job.get("range", [0, n])
            d = api.Screener(0)                                         # a fresh handle per run (sets, multiplex DB)
            d.load_texts([q for _, q in targets[lo:hi]], [1.0] * (hi - lo))
            if bgs:
                d.load_texts([q for _, q in bgs], [1.0] * len(bgs), which=api.BACKGROUND)
            try:
                if comm is not None and job.get("shard", True):
                    d.shard_targets(comm, lo, n)
                    copy = job.get("copy", "ok")
                    if rank == 0 and copy == "ok":
                        d.shard_sampler_targets(texts=[q for _, q in targets])
                    elif rank == 0 and copy == "altered":
                        alt = [q for _, q in targets]
                        k = job["alter"]
                        alt[k] = ("A" if alt[k][0] != "A" else "C") + alt[k][1:]
                        d.shard_sampler_targets(texts=alt)
                    else:
                        d.shard_sampler_targets()
                argv = list(run["argv"]) + job.get("argv_extra", [])
                o = design.options_from_argv(argv)
                text, pool = design.design(d, [x for x, _ in targets], [len(q) for _, q in targets], [x for x, _ in bgs],
                                           [len(q) for _, q in bgs], argv=argv, **o)
                res = {"rc": 0, "text": text.decode("latin-1"), "pool": [["%x" % x for p in q for x in p] for q in pool]}
            except api.PcrError as e:
                res = {"rc": e.rc, "msg": str(e)}
            if comm is not None:
                d.shard_targets(None, 0, 0)
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
    assert len(specs) <= 3
    tmp = tempfile.mkdtemp(prefix="pcramp_shard_design_")
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


def _world(jobs_per_rank, comm="gloo"):
    port = _free_port()
    return _run([{"world": len(jobs_per_rank), "rank": r, "port": port, "comm": comm, "jobs": jobs} for r, jobs in enumerate(jobs_per_rank)])


def _n_targets(src, ri):
    if src == "writers":
        sp = WRITER_SPECS[ri]
    else:
        with open(os.path.join(G, "program.json")) as f:
            sp = json.load(f)["runs"][ri]["spec"]
    return sp["n_fam"] * sp["per"]


def _golden(src, ri):
    with open(os.path.join(G, src + ".json")) as f:
        return json.load(f)["runs"][ri]


def _cuts(n, world, rng, single=False):
    """world contiguous ranges with seeded boundaries inside [1, n); single: the last rank holds one target"""
    if single:
        inner = sorted(rng.sample(range(1, n - 1), world - 2)) + [n - 1]
    else:
        inner = sorted(rng.sample(range(1, n), world - 1))
    b = [0] + inner + [n]
    return [[b[r], b[r + 1]] for r in range(world)]


def _check_runs(runs, outs, world):
    for k, (src, ri) in enumerate(runs):
        g = _golden(src, ri)
        res = [outs[r]["results"][k] for r in range(world)]
        if g.get("aborted"):
            assert res[0]["rc"] != 0 and all(x["rc"] == res[0]["rc"] for x in res), (src, ri, res)
            continue
        for r in range(world):
            assert res[r]["rc"] == 0, (src, ri, r, res[r].get("msg"))
            assert res[r]["text"] == g["output"], (src, ri, r)
        assert all(x["pool"] == res[0]["pool"] for x in res)


pytestmark = pytest.mark.gpu


def test_every_golden_run_world2():
    """All 6 writers.json runs and every program.json run at world 2 over gloo, a seeded boundary inside the target list: every
    rank's text equals the reference's file; the aborted runs return the same nonzero code on both ranks."""
    with open(os.path.join(G, "program.json")) as f:
        n_prog = len(json.load(f)["runs"])
    runs = [("writers", i) for i in range(6)] + [("program", i) for i in range(n_prog)]
    rng = random.Random(2718)
    jobs = [[], []]
    for src, ri in runs:
        for r, rg in enumerate(_cuts(_n_targets(src, ri), 2, rng)):
            jobs[r].append({"kind": "design", "src": src, "ri": ri, "range": rg})
    _check_runs(runs, _world(jobs), 2)


@pytest.mark.parametrize("mode", ["auto", "chain"])
def test_world3(mode):
    """World 3, one rank holding a single target: multiplex with backgrounds, the top-down start, the 5' / 3' moves, JSON."""
    runs = [("program", 1), ("program", 2), ("program", 3), ("program", 16), ("writers", 4)]
    rng = random.Random(31)
    jobs = [[], [], []]
    for src, ri in runs:
        for r, rg in enumerate(_cuts(_n_targets(src, ri), 3, rng, single=True)):
            jobs[r].append({"kind": "design", "src": src, "ri": ri, "range": rg, "env": mode})
    _check_runs(runs, _world(jobs), 3)


def test_world1_rccl():
    """World 1 over RCCL (the on-stream device path of the gather): a multiplex run with backgrounds."""
    runs = [("program", 3), ("writers", 0)]
    jobs = [{"kind": "design", "src": src, "ri": ri} for src, ri in runs]
    outs = _run([{"world": 1, "rank": 0, "comm": "rccl", "jobs": jobs}])
    _check_runs(runs, outs, 1)


def test_synthetic_world2_equals_unsharded():
    """~2 000 targets x 2 kb, 300 trials, 3 iterations: the world-2 text equals the unsharded pcr_design text."""
    want = _run([{"comm": None, "jobs": [{"kind": "design", "src": "synth", "shard": False}]}])[0]["results"][0]
    assert want["rc"] == 0, want.get("msg")
    cut = 1000 + 37
    outs = _world([[{"kind": "design", "src": "synth", "range": [0, cut]}], [{"kind": "design", "src": "synth", "range": [cut, 2000]}]])
    for r in range(2):
        got = outs[r]["results"][0]
        assert got["rc"] == 0, got.get("msg")
        assert got["text"] == want["text"] and got["pool"] == want["pool"]
    assert want["text"].count("ASSAY") >= 1


def _gather_jobs(world, seed, bad_rank=None):
    rng = random.Random(seed)
    jobs = []
    for k in range(4):
        n_total = rng.randint(world + 1, 400)
        inner = sorted(rng.sample(range(1, n_total), world - 1))
        if world > 1 and k == 1:                                         # a rank of one row
            inner = [1] + sorted(rng.sample(range(2, n_total), world - 2))
        b = [0] + inner + [n_total]
        jobs.append({"kind": "gather", "n_total": n_total, "n_vec": rng.randint(1, 5), "bounds": b, "seed": rng.randint(0, 1 << 30),
                     "extra": k % 2, "bad_rank": bad_rank if k == 3 else None})
    return jobs


@pytest.mark.parametrize("world", [2, 3])
def test_gather_bits_gloo(world):
    """Random n_vec, boundaries (one with a 1-row rank) and bits: the result equals the concatenation, padding bits zero; a rank
    with a bad argument gives PCR_ERR_ARG on every rank."""
    jobs = _gather_jobs(world, 77 + world, bad_rank=world - 1)
    outs = _world([jobs] * world)
    for r in range(world):
        res = outs[r]["results"]
        for j in range(3):
            assert res[j]["rc"] == 0 and res[j]["ok"], (r, j, res[j])
        assert res[3]["rc"] == PCR_ERR_ARG, res[3]


def test_gather_bits_rccl():
    jobs = _gather_jobs(1, 5)
    res = _run([{"world": 1, "rank": 0, "comm": "rccl", "jobs": jobs}])[0]["results"]
    assert all(x["rc"] == 0 and x["ok"] for x in res), res


def test_refusals_on_every_rank():
    """A sampler copy whose bytes differ from one rank's rows, rank 0 passing no copy, and pcr_design with arguments that differ
    across ranks: PCR_ERR_ARG on every rank, and no rank hangs."""
    n = _n_targets("writers", 0)
    rg = [[0, 5], [5, n]]
    base = {"kind": "design", "src": "writers", "ri": 0}
    jobs = [[], []]
    for r in range(2):
        jobs[r].append(dict(base, range=rg[r], copy="altered", alter=7))
        jobs[r].append(dict(base, range=rg[r], copy="none"))
        jobs[r].append(dict(base, range=rg[r], argv_extra=["--seed", "43"] if r == 1 else []))
    outs = _world(jobs)
    for r in range(2):
        res = outs[r]["results"]
        assert [x["rc"] for x in res] == [PCR_ERR_ARG] * 3, res


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with open(sys.argv[1]) as f:
        spec = json.load(f)
    result = _child(spec)
    with open(sys.argv[2], "w") as f:
        json.dump(result, f)
