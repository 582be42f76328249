"""Times pcr_pool_dimers beside the host route it replaces (stand-alone; bench.py is untouched).

Pools: the 50-pair panel of the C2 workload of pcramp_amd.synth (100 oligos, 10 000 cells) and a 500-pair pool sampled from
the same sequences by synth.make_pairs (1 000 oligos, 1 000 000 cells); plain oligos, rule ASSAY.  Every line is the median of
--repeats host-clock timings of the synchronous call on warm buffers, with the minimum and maximum.

  pool_dimers  Screener.pool_dimers(pool, rule="assay") with cap sized beforehand: every cell, one call.
  host_route   what a caller without pcr_pool_dimers does: pcr_dimer (Screener.max_dimer_tm) on every ordered pair of distinct
               oligos as a fake (F, R) assay, and pcr_thermo with check_homo_dimer = 1 (Screener.is_valid) for the diagonal.
               It yields tm_max only.  For plain oligos it is the same number: the script compares the two matrices bit for
               bit and fails if they differ, and prints a checksum of the host route's matrix.

    python profiles/bench_pool_dimers.py
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_pool_dimers.py   # k_pool_dimer beside k_thermo_wave, per duplex:
                                                                                    # the lines give launches and duplexes per launch

The host_route lines need nothing this call added: copied into the commit before it, the script reports those lines only.
Prints one JSON object per line.
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def distinct(pool):
    out = []
    seen = set()
    for f, r in pool:
        for w in ((int(f[0]), int(f[1])), (int(r[0]), int(r[1]))):
            if w not in seen:
                seen.add(w)
                out.append(w)
    return out


def host_route(d, oligos, fake):
    """pcr_dimer on every ordered pair, pcr_thermo's homodimer on the diagonal -> float32 [n, n] of tm_max."""
    n = len(oligos)
    m = np.asarray(d.max_dimer_tm(fake), np.float32).reshape(n, n).copy()
    homo = d.is_valid(oligos, True)
    m[np.arange(n), np.arange(n)] = [h["homodimer_tm"] for h in homo]
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pool-pairs", type=int, default=500)
    a = ap.parse_args()

    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale)
    pools = [("panel", wl["pairs"]),
             ("pool", synth.make_pairs(wl["packed"], wl["byte_offsets"], wl["lengths"], a.pool_pairs, 20261019))]
    d = api.Screener(0)                                                     # no sequences, no word DB: the call needs neither
    for name, pool in pools:
        oligos = distinct(pool)
        n = len(oligos)
        assert all(W.word_degeneracy(w) == 1 for w in oligos), "the host route's diagonal is the first expansion only"
        common = dict(pool=name, pairs=len(pool), oligos=n, cells=n * n, duplexes=n * n, launches=a.repeats + a.warmup + 1)
        # the n * n fake assays as a pcr_pair array, built once outside the timings (the diagonal's heterodimer is overwritten)
        words = np.array(oligos, dtype=np.uint64).reshape(n, 2)
        fake = np.ascontiguousarray(np.concatenate([np.repeat(words, n, axis=0), np.tile(words, (n, 1))], axis=1))
        got = None
        if hasattr(api.Screener, "pool_dimers"):
            ids, rec = d.pool_dimers(pool, rule="assay")
            assert len(rec) == n * n
            ts = measure(lambda: d.pool_dimers(pool, rule="assay", cap=n * n), a.repeats, a.warmup)
            got = api.Screener.dimer_matrix(rec, n)
            print(json.dumps(dict(call="pool_dimers", records=int(len(rec)), above_40=int((rec["tm_max"] >= 40.0).sum()),
                                  median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                                  **common)), flush=True)
        want = host_route(d, oligos, fake)
        ts = measure(lambda: host_route(d, oligos, fake), a.repeats, a.warmup)
        same = None if got is None else bool((got.view(np.uint32) == want.view(np.uint32)).all())
        print(json.dumps(dict(call="host_route", tm_max_sha16=hashlib.sha256(want.tobytes()).hexdigest()[:16], bit_equal=same,
                              median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                              **common)), flush=True)
        if same is False:
            bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
            raise SystemExit("pool_dimers and the host route differ in %d cells, first (%d, %d)" % (len(bad), bad[0][0], bad[0][1]))
    d.close()


if __name__ == "__main__":
    main()
