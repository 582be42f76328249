# pcr_optimize_batch for 256 assays on C5's shard: unsharded, sharded at world 1 over RCCL with each combine, and sharded at
# world 2 over gloo with both ranks on the one GPU.  GPU box:  python profiles/dbg/opt_shard_c5.py [n_trial] [reps]
# Prints one JSON line per configuration (median of `reps` timed calls after one warm-up call).
import json, os, socket, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np

KW = dict(degen=16, target_threshold=1.0, search_multiplier=0.9, amp_min=80, amp_max=200, have_background=False)


def setup(lo=None, hi=None):
    from pcramp_amd import api, synth
    c5 = synth.workload("C5_shard")
    s = api.Screener(0)
    n = len(c5["lengths"])
    lo, hi = (0, n) if lo is None else (lo, hi)
    s.load_sequences(c5["packed"], c5["byte_offsets"][lo:hi], c5["lengths"][lo:hi])
    return s, n


def trials(n_trial):
    s, _ = setup()
    t, _, _ = s.random_assays(2025, n_trial)               # (the same assays on every rank: sampled over all targets)
    s.close()
    return t


def timed(s, trial, reps):
    from pcramp_amd import moves
    thr = float(np.float32(1.0) * np.float32(0.9))
    s.select_words(trial, thr, 18, count=False)
    first = moves.optimize_batch(s, trial, **KW)
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        moves.optimize_batch(s, trial, **KW)
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), first


def rank_main(rank, port, n_trial, reps):
    import datetime
    import torch  # noqa: F401
    import torch.distributed as dist
    from pcramp_amd import shard
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, world_size=2, rank=rank, timeout=datetime.timedelta(seconds=120))
    trial = trials(n_trial)
    s, n = setup()
    s.close()
    cut = n // 2
    s, _ = setup(*((0, cut) if rank == 0 else (cut, n)))
    comm = s.comm_init_host(2, rank, shard.gloo_allgather())
    s.shard_targets(comm, 0 if rank == 0 else cut, n)
    ms, first = timed(s, trial, reps)
    if rank == 0:
        print(json.dumps({"config": "world2_gloo_shared_gpu", "mode": s.shard_combine_mode(), "ms": ms, "n_trial": n_trial,
                          "iters_max": max(first[2]), "best_hash": hash(tuple(first[0]))}), flush=True)
    s.comm_destroy(comm)
    s.close()
    dist.destroy_process_group()


def main():
    n_trial = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    import torch  # noqa: F401
    from pcramp_amd import api
    trial = trials(n_trial)
    s, n = setup()
    ms, first = timed(s, trial, reps)
    print(json.dumps({"config": "unsharded", "ms": ms, "n_trial": n_trial, "iters_max": max(first[2]), "best_hash": hash(tuple(first[0]))}), flush=True)
    comm = s.comm_init_rank(api.Screener.comm_unique_id(), 1, 0)
    for mode in ("exact", "chain"):
        os.environ["PCRAMP_SHARD_COMBINE"] = mode
        s.shard_targets(comm, 0, n)
        ms, got = timed(s, trial, reps)
        print(json.dumps({"config": "world1_rccl", "mode": s.shard_combine_mode(), "ms": ms, "same_as_unsharded": got == first}), flush=True)
    os.environ.pop("PCRAMP_SHARD_COMBINE", None)
    s.shard_targets(None, 0, 0)
    s.comm_destroy(comm)
    s.close()
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--rank", str(r), str(port), str(n_trial), str(reps)]) for r in range(2)]
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
        rank_main(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5]))
    else:
        main()
