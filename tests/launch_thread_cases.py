"""Inputs shared by test_gpu_launch_thread.py and the child process it starts (python launch_thread_cases.py close):
the shape of test_lean_passes_leave_a_consistent_state -- three families of related 2 400-base sequences plus four
unrelated 1 500-base ones, the smallest at which the third form of the seed scan and the lean pass run -- at 43 and at
130 sequences (a bitset of three words, the last one partial), and batches of even size whose oligos come from the
family roots."""
import os
import random
import sys

from testdata import rand_seq, revcomp, mutate


def make_seqs(n_seqs, seed=77031):
    rng = random.Random(seed)
    per_family = (n_seqs - 4) // 3
    assert 3 * per_family + 4 == n_seqs
    roots = [rand_seq(rng, 2400) for _ in range(3)]
    seqs = []
    for r in roots:
        seqs += [r] + [mutate(rng, r, 0.03) for _ in range(per_family - 1)]
    seqs += [rand_seq(rng, 1500) for _ in range(4)]
    return roots, seqs


def make_batches(orc, roots, n, seed, sizes=(2, 4, 6, 8, 10, 12, 14, 16)):
    """n batches, each different: sizes cycle through `sizes` in a shuffled order, every oligo is drawn afresh (from one
    root or from two), a quarter of the pairs repeat a pair of the batch before (the planner's per-oligo cache hits)."""
    rng = random.Random(seed)
    out, prev = [], []
    for b in range(n):
        k = sizes[(b * 5 + b // len(sizes)) % len(sizes)]
        fam = [roots[b % 3]] if b % 4 else [roots[b % 3], roots[(b + 1) % 3]]
        batch = []
        for i in range(k):
            if prev and rng.random() < 0.25:
                batch.append(prev[rng.randrange(len(prev))])
                continue
            root = fam[i % len(fam)]
            a = rng.randrange(0, 2000)
            f = root[a:a + rng.randint(18, 25)]
            r = revcomp(root[a + 100:a + 100 + rng.randint(18, 25)])
            batch.append((orc.centered_word(f), orc.centered_word(r)))
        out.append(batch)
        prev = batch
    return out


def screener(api, launch_thread, stream=None):
    """A handle with PCRAMP_LAUNCH_THREAD as asked (the library reads it when the handle is created)."""
    old = os.environ.get("PCRAMP_LAUNCH_THREAD")
    os.environ["PCRAMP_LAUNCH_THREAD"] = "1" if launch_thread else "0"
    try:
        return api.Screener(0, stream=stream)
    finally:
        if old is None:
            os.environ.pop("PCRAMP_LAUNCH_THREAD", None)
        else:
            os.environ["PCRAMP_LAUNCH_THREAD"] = old


def _child_close():
    """close() with passes still queued behind the launcher thread must return, and the process must exit normally."""
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    from pcramp_amd import api
    from oracle_lib import Oracle
    orc = Oracle()
    roots, seqs = make_seqs(43)
    batches = make_batches(orc, roots, 6, 5)
    thr = float(np.float32(1.0) * np.float32(0.9))
    dev = screener(api, True)
    dev.load_texts(seqs, [1.0] * len(seqs))
    words = int(dev.bitset_words())
    outs = [torch.zeros((2, len(p), words), dtype=torch.int64, device="cuda:0") for p in batches]
    dev.screen_device(batches[0], thr, outs[0][0].data_ptr(), outs[0][1].data_ptr(), 1.0, 1.0, 80, 200, False)
    dev.synchronize()
    for p, o in zip(batches[1:], outs[1:]):
        dev.screen_device(p, thr, o[0].data_ptr(), o[1].data_ptr(), 1.0, 1.0, 80, 200, False)
    n, depth = dev.launcher_stats()
    dev.close()                                 # no synchronize before it
    torch.cuda.synchronize()
    print("closed with %d pipelined passes" % n)
    sys.stdout.flush()


if __name__ == "__main__":
    if sys.argv[1:] == ["close"]:
        _child_close()
