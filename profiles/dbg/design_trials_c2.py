# One design iteration of 1 000 trials in all (pcr_design --count 1 --trial 1000) on C2's targets (10 000 x 10 kb, no backgrounds):
# unsharded, with trial ranks (the reference's MPI mode, pcr_design_trial_ranks) at world 1 over RCCL, and with trial ranks at
# world 2 over gloo, 500 trials per rank, both ranks on the one GPU (a correctness rig, not a scaling figure).
# GPU box:  PCRAMP_TIMING=1 python profiles/dbg/design_trials_c2.py [n_trial]
# Prints one JSON line per configuration (wall time of the call; world 1: whether its text equals the unsharded one; world 2:
# whether both ranks wrote the same text).  PCRAMP_TIMING=1 adds the library's phase split of the iteration on stderr
# ("reduction" = the time spent in the all-gather of the ranks' best assays, waiting for the slower rank included).
import hashlib, json, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def setup():
    from pcramp_amd import api, synth
    c2 = synth.workload("C2")
    s = api.Screener(0)
    s.load_sequences(c2["packed"], c2["byte_offsets"], c2["lengths"])
    return s, c2, len(c2["lengths"])


def run_design(s, c2, n, n_trial, world=1):
    from pcramp_amd import design
    argv = ["pcramp", "-t", "t.fa", "-o", "out.txt", "--count", "1", "--trial", str(n_trial), "--seed", "2025"]
    o = design.options_from_argv(argv, world=world)
    t0 = time.perf_counter()
    text, pool = design.design(s, [">c2_%d" % i for i in range(n)], [int(x) for x in c2["lengths"]], argv=argv, **o)
    return (time.perf_counter() - t0) * 1e3, hashlib.sha256(text).hexdigest()


def rank_main(rank, port, n_trial, out_path):
    import datetime
    import torch  # noqa: F401
    import torch.distributed as dist
    from pcramp_amd import shard
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, world_size=2, rank=rank, timeout=datetime.timedelta(seconds=300))
    s, c2, n = setup()
    comm = s.comm_init_host(2, rank, shard.gloo_allgather())
    t0 = time.perf_counter()
    s.design_trial_ranks(comm)
    attach_ms = (time.perf_counter() - t0) * 1e3
    ms, h = run_design(s, c2, n, n_trial, world=2)
    with open(out_path, "w") as f:
        json.dump({"ms": ms, "attach_ms": attach_ms, "sha": h}, f)
    s.design_trial_ranks(None)
    s.comm_destroy(comm)
    s.close()
    dist.destroy_process_group()


def main():
    n_trial = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    import tempfile
    import torch  # noqa: F401
    from pcramp_amd import api
    s, c2, n = setup()
    ms, want = run_design(s, c2, n, n_trial)
    print(json.dumps({"config": "unsharded", "ms": ms, "n_trial": n_trial}), flush=True)
    # (the iteration changes the flags and splits the targets: world 1 starts from a fresh load)
    s.close()
    s, c2, n = setup()
    comm = s.comm_init_rank(api.Screener.comm_unique_id(), 1, 0)
    t0 = time.perf_counter()
    s.design_trial_ranks(comm)
    attach_ms = (time.perf_counter() - t0) * 1e3
    ms, h = run_design(s, c2, n, n_trial)
    print(json.dumps({"config": "trial_ranks_world1_rccl", "ms": ms, "attach_ms": attach_ms, "n_trial": n_trial, "same_as_unsharded": h == want}), flush=True)
    s.design_trial_ranks(None)
    s.comm_destroy(comm)
    s.close()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    tmp = tempfile.mkdtemp(prefix="design_trials_c2_")
    outs = [os.path.join(tmp, "rank%d.json" % r) for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), str(port), str(n_trial), outs[r]]) for r in range(2)]
    for p in procs:
        try:
            p.wait(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            sys.exit("world 2 did not finish")
    if max(p.returncode for p in procs):
        sys.exit(max(p.returncode for p in procs))
    res = []
    for o in outs:
        with open(o) as f:
            res.append(json.load(f))
    print(json.dumps({"config": "trial_ranks_world2_gloo_shared_gpu", "ms": [r["ms"] for r in res], "attach_ms": [r["attach_ms"] for r in res],
                      "n_trial": n_trial, "trials_per_rank": -(-n_trial // 2), "ranks_agree": res[0]["sha"] == res[1]["sha"]}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--rank":
        rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        main()
