"""The local search over targets sharded across ranks (pcr_shard_targets, pcr_shard.inc): pcr_optimize_batch,
pcr_optimization_move and pcr_make_degenerate with the target set cut at arbitrary boundaries must return what the unsharded
call returns -- the reference's own answers on the goldens -- with both combines (exact partials, ordered chain).

Every rank is a fresh child process (this file run as a script on a JSON spec) with a time limit; two ranks share the one GPU
through the host-collective communicator over gloo (RCCL refuses two ranks on one device), one rank exercises RCCL.  The
parent never opens the GPU; at most two children have it open at a time."""
import json
import os
import random
import socket
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden")
CHILD_TIMEOUT = 600
PCR_ERR_ARG, PCR_ERR_STATE = -1, -3


def _hexpair(p):
    return ["%x" % p[0][0], "%x" % p[0][1], "%x" % p[1][0], "%x" % p[1][1]]


def _pair(h):
    return ((int(h[0], 16), int(h[1], 16)), (int(h[2], 16), int(h[3], 16)))


# ------------------------------------------------------------------------------------------------ child side
class _Rc(Exception):
    def __init__(self, rc, msg):
        super().__init__(msg)
        self.rc = rc


def _child(spec):
    import torch  # noqa: F401  (before the library: one HIP runtime in the process)
    import datetime
    import torch.distributed as dist
    from pcramp_amd import api, moves, shard

    world, rank = spec.get("world", 1), spec.get("rank", 0)
    if spec.get("comm") in ("gloo", "rccl2"):                            # (rccl2: gloo carries RCCL's unique id)
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % spec["port"], world_size=world, rank=rank,
                                timeout=datetime.timedelta(seconds=120))
    out = {"results": []}
    d = api.Screener(spec.get("device", 0))

    def check(rc):
        if rc != 0:
            raise _Rc(rc, api._err(d.L))
    d._check = check
    comm = None
    try:
        for job in spec["jobs"]:
            res = {}
            if job.get("env") is not None:
                os.environ["PCRAMP_SHARD_COMBINE"] = job["env"]
            seqs, wts = job["seqs"], job["weights"]
            lo, hi = job.get("range", [0, len(seqs)])
            d.load_texts(seqs[lo:hi], wts[lo:hi], which=api.TARGET)
            if job.get("bgs"):
                d.load_texts(job["bgs"], [1.0] * len(job["bgs"]), which=api.BACKGROUND)
            if job.get("amplicons"):
                d.multiplex_load(job["amplicons"], job["sel"]["min_primer"])
            s = job["sel"]
            sel = [_pair(p) for p in job["select_pairs"]]
            d.select_words(sel, s["thr"], s["min_primer"], s["opt5"], s["opt3"], which=api.TARGET)
            if job.get("bgs"):
                d.select_words(sel, s["bg_thr"], s["bg_min_len"], s["opt5"], s["opt3"], which=api.BACKGROUND)
            res["n_entries"] = len(d.entries())
            for op in job.get("before", []):                         # unsharded work on this handle first (cache history)
                moves.optimize_batch(d, [_pair(p) for p in op["pairs"]], **op["kw"])
            if job.get("shard"):
                if comm is None:
                    if spec["comm"] == "gloo":
                        comm = d.comm_init_host(world, rank, shard.gloo_allgather())
                    elif spec["comm"] == "rccl2":
                        uid = [api.Screener.comm_unique_id() if rank == 0 else None]
                        dist.broadcast_object_list(uid, src=0)
                        comm = d.comm_init_rank(uid[0], world, rank)
                    else:
                        comm = d.comm_init_rank(api.Screener.comm_unique_id(), 1, 0)
                first = job.get("claim_first", lo)
                try:
                    d.shard_targets(comm, first, len(seqs))
                    res["mode"] = d.shard_combine_mode()
                except _Rc as e:
                    res["attach_rc"] = e.rc
                    out["results"].append(res)
                    continue
            res["ops"] = []
            for op in job["ops"]:
                pairs = [_pair(p) for p in op.get("pairs", [])]
                pool = [_pair(p) for p in op["pool"]] if op.get("pool") is not None else None
                try:
                    if op["op"] == "optimize_batch":
                        kw = dict(op["kw"])
                        if pool is not None:
                            kw["pool"] = pool
                        bp, bs, it = moves.optimize_batch(d, pairs, **kw)
                        r = {"best": [_hexpair(p) for p in bp], "score": [[int(np.float32(x).view(np.uint32)) for x in sc] for sc in bs],
                             "iters": it}
                    elif op["op"] == "make_degenerate":
                        got, ok = moves.make_degenerate(d, pairs, max_dimer=op["max_dimer"], **op["kw"])
                        r = {"best": [_hexpair(p) for p in got], "valid": ok}
                    elif op["op"] == "optimization_move":
                        w, sc = moves.optimization_move(d, pairs[0], op["move"], op["side"], **op["kw"])
                        r = {"word": ["%x" % w[0], "%x" % w[1]], "score": [int(np.float32(x).view(np.uint32)) for x in sc]}
                    elif op["op"] == "design":
                        import ctypes as C
                        blob = (C.c_uint8 * 4096)()                  # (refused before the arguments are read)
                        fn = d.L.pcr_design
                        fn.restype = C.c_int
                        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
                        r = {"rc": int(fn(d.h, C.addressof(blob), C.addressof(blob), 0, None, None, 0, None))}
                    r["rc"] = r.get("rc", 0)
                except _Rc as e:
                    r = {"rc": e.rc, "msg": str(e)}
                res["ops"].append(r)
            if job.get("shard"):
                d.shard_targets(None, 0, 0)
            out["results"].append(res)
    finally:
        if comm is not None:
            d.comm_destroy(comm)
        d.close()
        if spec.get("comm") in ("gloo", "rccl2"):
            dist.destroy_process_group()
    return out


# ------------------------------------------------------------------------------------------------ parent side
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(specs):
    """Start one child per spec (all at once: they are the ranks of one run), wait with a time limit, return their outputs."""
    tmp = tempfile.mkdtemp(prefix="pcramp_shard_")
    procs = []
    for k, spec in enumerate(specs):
        sp, op = os.path.join(tmp, "spec%d.json" % k), os.path.join(tmp, "out%d.json" % k)
        with open(sp, "w") as f:
            json.dump(spec, f)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), sp, op]
        procs.append((subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT), op))
    outs, logs = [], []
    try:
        for p, op in procs:
            try:
                log, _ = p.communicate(timeout=CHILD_TIMEOUT)
            except subprocess.TimeoutExpired:
                for q, _ in procs:
                    q.kill()
                raise AssertionError("a rank did not finish within %d s" % CHILD_TIMEOUT)
            logs.append(log.decode(errors="replace"))
            assert p.returncode == 0, "rank exited with %d:\n%s" % (p.returncode, logs[-1][-4000:])
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


def _sel(o, bg_thr=None, bg_min_len=16):
    return {"thr": float(np.float32(o["target_threshold"]) * np.float32(o["search_multiplier"])), "min_primer": o["min_primer"],
            "opt5": int(o["optimize_5"]), "opt3": int(o["optimize_3"]), "bg_thr": bg_thr if bg_thr is not None else 0.0, "bg_min_len": bg_min_len}


def _kw(o, mo):
    return dict(target_threshold=o["target_threshold"], search_multiplier=o["search_multiplier"], amp_min=o["amp_min"],
                amp_max=o["amp_max"], use_taq_mama=bool(o["use_taq_mama"]), **mo)


def _golden_jobs():
    """(job without range/shard, expected answers per op) for every golden case of moves / multiplex_optimize / degenerate."""
    out = []
    with open(os.path.join(G, "moves.json")) as f:
        for c in json.load(f)["cases"]:
            o, mo = c["options"], c["move_options"]
            ops, want = [], []
            for pi, bp, sc in c["optimize"]:
                ops.append({"op": "optimize_batch", "pairs": [c["pairs"][pi]], "kw": _kw(o, mo)})
                want.append({"best": [bp], "score": [[int(np.float32(x).view(np.uint32)) for x in sc]]})
            pi, side, move, wh, sc, _ = c["moves"][0]
            ops.append({"op": "optimization_move", "pairs": [c["pairs"][pi]], "move": move, "side": side, "kw": _kw(o, mo)})
            want.append({"word": wh, "score": [int(np.float32(x).view(np.uint32)) for x in sc]})
            out.append(({"seqs": c["seqs"], "weights": c["weights"], "bgs": c["backgrounds"], "select_pairs": c["pairs"],
                         "sel": _sel(o, float(np.float32(c["bg_select_threshold"])), c["bg_min_len"]), "ops": ops}, want))
    with open(os.path.join(G, "multiplex_optimize.json")) as f:
        for c in json.load(f)["cases"]:
            o, mo = c["options"], c["move_options"]
            ops, want = [], []
            for pi, use_pool, bp, sc in c["optimize"]:
                ops.append({"op": "optimize_batch", "pairs": [c["candidates"][pi]], "kw": _kw(o, mo), "pool": c["pool"] if use_pool else []})
                want.append({"best": [bp], "score": [[int(np.float32(x).view(np.uint32)) for x in sc]]})
            out.append(({"seqs": c["seqs"], "weights": c["weights"], "bgs": c["backgrounds"], "amplicons": c["amplicons"],
                         "select_pairs": c["candidates"] + c["pool"], "sel": _sel(o, float(np.float32(c["bg_select_threshold"])), c["bg_min_len"]),
                         "ops": ops}, want))
    with open(os.path.join(G, "degenerate.json")) as f:
        for c in json.load(f)["cases"]:
            o, mo = c["options"], c["move_options"]
            ops = [{"op": "make_degenerate", "pairs": c["pairs"], "max_dimer": c["max_dimer"], "kw": _kw(o, mo)}]
            want = [{"best": [w for w, _ in c["degenerate"]], "valid": [bool(ok) for _, ok in c["degenerate"]]}]
            out.append(({"seqs": c["seqs"], "weights": c["weights"], "select_pairs": c["pairs"], "sel": _sel(o), "ops": ops}, want))
    return out


def _norm(r):
    r = dict(r)
    for k in ("best",):
        if k in r:
            r[k] = [[x.lower().lstrip("0") or "0" for x in p] for p in r[k]]
    if "word" in r:
        r["word"] = [x.lower().lstrip("0") or "0" for x in r["word"]]
    return r


def _split(n, how):
    cut = 5 if how == "uneven" else n // 2
    return [[0, cut], [cut, n]]


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("how", ["uneven", "even"])
@pytest.mark.parametrize("mode", ["exact", "chain"])
def test_goldens_world2_gloo(how, mode):
    """moves.json optimize(), multiplex_optimize.json and degenerate.json at world 2 (host communicator over gloo, both ranks on
    the one GPU): every rank returns the reference's assays, Scores (as float bits) and validity flags."""
    cases = _golden_jobs()
    jobs = [[], []]
    for job, _ in cases:
        for r, rng in enumerate(_split(len(job["seqs"]), how)):
            jobs[r].append(dict(job, range=rng, shard=True, env=mode))
    outs = _world(jobs)
    for r in range(2):
        for (job, want), res in zip(cases, outs[r]["results"]):
            assert res["mode"] == (1 if mode == "exact" else 2)
            for w, got in zip(want, res["ops"]):
                assert got["rc"] == 0, got
                g = _norm(got)
                for k, v in _norm(w).items():
                    assert g[k] == v, (r, k)


def _many_case(weights_kind, n_base=8):
    from pcramp_amd import words as W
    from testdata import family_targets, sample_pair, mutate, rand_seq
    rng = random.Random(90210)
    seqs = family_targets(rng, 4, 10, 700, div=0.05)
    bgs = [mutate(rng, s, 0.12) for s in seqs[::3]] + [rand_seq(rng, 600) for _ in range(4)]
    txt = []
    while len(txt) < n_base:
        p = sample_pair(rng, rng.choice(seqs))
        if p:
            txt.append(p)
    for f, r in list(txt[:4]):
        txt.append((mutate(rng, f, 0.1), mutate(rng, r, 0.1)))
    cw = lambda s: W.centered_word(W.codes_from_text(s))
    pairs = [(cw(f), cw(r)) for f, r in txt]
    if weights_kind == "wide":                                         # 1e-20 .. 1e20: no exact partials, auto picks the chain
        tw = [float(np.float32(10.0 ** (-20 + (i * 7) % 41))) for i in range(len(seqs))]
    else:
        tw = [1.0] * len(seqs)
    if weights_kind == "empty_rank":                                   # the last rank's shard: random sequences only
        seqs = seqs + [rand_seq(rng, 700) for _ in range(6)]
        tw = tw + [1.0] * 6
    batch = (pairs * 12)[:len(pairs) * 12]
    random.Random(5).shuffle(batch)
    sel = {"thr": float(np.float32(1.0) * np.float32(0.9)), "min_primer": 18, "opt5": 1, "opt3": 1,
           "bg_thr": float(np.float32(0.8) * np.float32(0.9)), "bg_min_len": 16}
    job = {"seqs": seqs, "weights": tw, "bgs": bgs, "select_pairs": [_hexpair(p) for p in pairs], "sel": sel,
           "ops": [{"op": "optimize_batch", "pairs": [_hexpair(p) for p in batch], "kw": dict(degen=16)}]}
    return job, [_hexpair(p) for p in pairs]


def _unsharded(job):
    return _run([{"comm": None, "jobs": [dict(job)]}])[0]["results"][0]["ops"]


@pytest.mark.parametrize("kind", ["wide", "empty_rank"])
def test_many_assays_world2_equals_unsharded(kind):
    """>= 128 assays at world 2 == one unsharded rank, element for element (best, Score, iterations): once with weights that
    only the ordered chain sums exactly (auto must pick it), once with a rank whose shard has no word-DB entries."""
    job, _ = _many_case(kind)
    assert len(job["ops"][0]["pairs"]) >= 128
    want = _unsharded(job)
    n = len(job["seqs"])
    cut = n - 6 if kind == "empty_rank" else 17
    outs = _world([[dict(job, range=[0, cut], shard=True, env="auto")], [dict(job, range=[cut, n], shard=True, env="auto")]])
    for r in range(2):
        res = outs[r]["results"][0]
        assert res["mode"] == (2 if kind == "wide" else 1)
        assert res["ops"] == want
    if kind == "empty_rank":
        assert outs[1]["results"][0]["n_entries"] == 0 and outs[0]["results"][0]["n_entries"] > 0
    assert len(set(want[0]["iters"])) > 1


def test_world1_rccl_equals_unsharded():
    """World 1 through RCCL (the device-side collective path), each combine: sharded == unsharded on the same batch."""
    job, _ = _many_case("plain")
    jobs = [dict(job)] + [dict(job, shard=True, env=m) for m in ("exact", "chain")]
    res = _run([{"world": 1, "rank": 0, "comm": "rccl", "jobs": jobs}])[0]["results"]
    assert res[1]["mode"] == 1 and res[2]["mode"] == 2
    assert res[1]["ops"] == res[0]["ops"] and res[2]["ops"] == res[0]["ops"]


def test_world2_rccl_two_devices():
    q = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, timeout=300)
    n_dev = int(q.stdout.decode().strip().splitlines()[-1]) if q.returncode == 0 else 0
    if n_dev < 2:
        pytest.skip("world 2 over RCCL needs two GPUs; this box has %d (two ranks on one GPU are covered over gloo above)" % n_dev)
    job, _ = _many_case("plain")
    want = _unsharded(job)
    n = len(job["seqs"])
    port = _free_port()
    specs = []
    for r, rng in enumerate(([0, 13], [13, n])):
        specs.append({"world": 2, "rank": r, "port": port, "comm": "rccl2", "device": r, "jobs": [dict(job, range=rng, shard=True, env="auto")]})
    outs = _run(specs)
    for r in range(2):
        assert outs[r]["results"][0]["ops"] == want


def test_refusals_on_every_rank():
    """Non-contiguous ranges -> PCR_ERR_ARG, ranks given different batches -> PCR_ERR_ARG, pcr_design with a shard attached ->
    PCR_ERR_STATE: on every rank, and no rank hangs (the children's time limit ends the test otherwise)."""
    job, pairs = _many_case("plain")
    n = len(job["seqs"])
    small = dict(job, ops=[{"op": "optimize_batch", "pairs": pairs[:3], "kw": dict(degen=16)}])
    gap = [dict(small, range=[0, 11], shard=True), dict(small, range=[11, n], shard=True, claim_first=12)]
    other = dict(small, ops=[{"op": "optimize_batch", "pairs": pairs[3:6], "kw": dict(degen=16)}])
    differ = [dict(small, range=[0, 11], shard=True), dict(other, range=[11, n], shard=True)]
    design = [dict(small, range=rng, shard=True, ops=[{"op": "design"}]) for rng in ([0, 11], [11, n])]
    outs = _world([[gap[0], differ[0], design[0]], [gap[1], differ[1], design[1]]])
    for r in range(2):
        res = outs[r]["results"]
        assert res[0]["attach_rc"] == PCR_ERR_ARG
        assert res[1]["ops"][0]["rc"] == PCR_ERR_ARG
        assert res[2]["ops"][0]["rc"] == PCR_ERR_STATE


def test_cache_history_does_not_matter():
    """Rank 0 runs an unrelated optimize_batch first; the sharded batch still equals the unsharded run."""
    job, pairs = _many_case("plain")
    want = _unsharded(job)
    n = len(job["seqs"])
    before = [{"pairs": [pairs[1], pairs[5], pairs[9]], "kw": dict(degen=4)}]
    outs = _world([[dict(job, range=[0, 9], shard=True, before=before)], [dict(job, range=[9, n], shard=True)]])
    for r in range(2):
        assert outs[r]["results"][0]["ops"] == want


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with open(sys.argv[1]) as f:
        spec = json.load(f)
    result = _child(spec)
    with open(sys.argv[2], "w") as f:
        json.dump(result, f)
