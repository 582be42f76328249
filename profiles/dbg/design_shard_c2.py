# One design iteration (pcr_design --count 1 --trial 1000) on C2's targets (10 000 x 10 kb, no backgrounds): unsharded, sharded at
# world 1 over RCCL, and sharded at world 2 over gloo with both ranks on the one GPU (a correctness rig, not a scaling figure).
# GPU box:  PCRAMP_TIMING=1 python profiles/dbg/design_shard_c2.py [n_trial]
# Prints one JSON line per configuration (wall time of the call, and whether its text equals the unsharded one); PCRAMP_TIMING=1
# adds the library's phase split of the iteration on stderr ("exchanges" = the time spent in the sharded loop's collectives).
import hashlib, json, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def setup(lo=None, hi=None):
    from pcramp_amd import api, synth
    c2 = synth.workload("C2")
    s = api.Screener(0)
    n = len(c2["lengths"])
    lo, hi = (0, n) if lo is None else (lo, hi)
    s.load_sequences(c2["packed"], c2["byte_offsets"][lo:hi], c2["lengths"][lo:hi])
    return s, c2, n


def run_design(s, c2, n, n_trial):
    from pcramp_amd import design
    argv = ["pcramp", "-t", "t.fa", "-o", "out.txt", "--count", "1", "--trial", str(n_trial), "--seed", "2025"]
    o = design.options_from_argv(argv)
    t0 = time.perf_counter()
    text, pool = design.design(s, [">c2_%d" % i for i in range(n)], [int(x) for x in c2["lengths"]], argv=argv, **o)
    return (time.perf_counter() - t0) * 1e3, hashlib.sha256(text).hexdigest()


def rank_main(rank, port, n_trial, want):
    import datetime
    import torch  # noqa: F401
    import torch.distributed as dist
    from pcramp_amd import shard
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, world_size=2, rank=rank, timeout=datetime.timedelta(seconds=300))
    from pcramp_amd import synth
    n = len(synth.workload("C2")["lengths"])
    cut = n // 2 + 37                                       # not a multiple of 64
    s, c2, n = setup(*((0, cut) if rank == 0 else (cut, n)))
    comm = s.comm_init_host(2, rank, shard.gloo_allgather())
    s.shard_targets(comm, 0 if rank == 0 else cut, n)
    if rank == 0:
        s.shard_sampler_targets(packed=c2["packed"], byte_offsets=c2["byte_offsets"], lengths=c2["lengths"])
    else:
        s.shard_sampler_targets()
    ms, h = run_design(s, c2, n, n_trial)
    if rank == 0:
        print(json.dumps({"config": "world2_gloo_shared_gpu", "ms": ms, "n_trial": n_trial, "same_as_unsharded": h == want}), flush=True)
    s.shard_targets(None, 0, 0)
    s.comm_destroy(comm)
    s.close()
    dist.destroy_process_group()


def main():
    n_trial = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
    import torch  # noqa: F401
    from pcramp_amd import api
    s, c2, n = setup()
    ms, want = run_design(s, c2, n, n_trial)
    print(json.dumps({"config": "unsharded", "ms": ms, "n_trial": n_trial}), flush=True)
    # (the iteration changes the flags and splits the targets: world 1 starts from a fresh load)
    s.close()
    s, c2, n = setup()
    comm = s.comm_init_rank(api.Screener.comm_unique_id(), 1, 0)
    s.shard_targets(comm, 0, n)
    s.shard_sampler_targets(packed=c2["packed"], byte_offsets=c2["byte_offsets"], lengths=c2["lengths"])
    ms, h = run_design(s, c2, n, n_trial)
    print(json.dumps({"config": "world1_rccl", "ms": ms, "n_trial": n_trial, "same_as_unsharded": h == want}), flush=True)
    s.shard_targets(None, 0, 0)
    s.comm_destroy(comm)
    s.close()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), str(port), str(n_trial), want]) for r in range(2)]
    for p in procs:
        try:
            p.wait(timeout=900)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            sys.exit("world 2 did not finish")
    sys.exit(max(p.returncode for p in procs))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--rank":
        rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    else:
        main()
