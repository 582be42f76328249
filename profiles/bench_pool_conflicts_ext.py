"""Times pcr_pool_conflicts_ext beside the two calls whose device work it combines, and beside the host route that yields the
same records (stand-alone; bench.py is untouched).  Needs a GPU.

Pools: the 50-pair panel of the C2 workload of pcramp_amd.synth on its own targets (10 000 x 10 kb, every binding site at
0.81), and tests/pool_dimer_cases.full_pool (1 024 pairs of distinct plain oligos, 2 048 oligos) on the first --full-scale
of those targets (random oligos have next to no site there: the dimer work is what the full pool weighs).  Settings: no
whole-oligo dimers, min_run = 4, min_extension = 1, rule POOL, dg_max = --dg-max.  The legs are timed alternately, round by
round, on warm buffers with the arrays sized beforehand: a host clock around synchronous calls.  Every line gives the median of
--repeats rounds with the minimum and maximum.

  ext          (a) Screener.pool_conflicts(pool, dimers=None, ext_min_run=4, ext_dg_max=..., cap=every cell): one call of
               pcr_pool_conflicts_ext.
  two_calls    (b) Screener.pool_conflicts(pool, dimers=None, cap=every cell) and Screener.pool_dimers_end3(pool, dg_max=...,
               cap=(cells, 0)), cell records only: the same kernels, n_distinct^2 records downloaded where (a) downloads n_pool^2.
  host_route   (c) two_calls and host_ext below: the oligo -> row attribution and the reduction over unordered pairs in numpy.

The script fails unless host_route's records equal ext's byte for byte.

    python profiles/bench_pool_conflicts_ext.py
    python profiles/bench_pool_conflicts_ext.py --skip-full

Prints one JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELL_FIELDS = ("q_expansion", "t_expansion", "run", "extension", "overlap", "overlap_matches", "flags", "dG", "tm", "dH", "dS")


def host_ext(dtype, ids, base, cells, keep):
    """pool_conflicts' records (dimers=None), pool_dimers_end3's record of every cell with a placement and which of them the dG
    filter keeps -> the records of pcr_pool_conflicts_ext: its definition in numpy."""
    ids = np.asarray(ids, np.int64)
    n_pool = len(ids) // 2
    n_ol = int(ids.max()) + 1 if n_pool else 0
    n_cells = n_pool * (n_pool + 1) // 2
    out = np.zeros(n_cells, dtype)
    a_of = np.repeat(np.arange(n_pool), np.arange(n_pool, 0, -1))
    start = a_of * n_pool - a_of * (a_of - 1) // 2
    out["row_a"] = a_of
    out["row_b"] = np.arange(n_cells) - start + a_of
    out["melt"] = np.float32(-1.0)
    at = base["row_a"].astype(np.int64) * n_pool - base["row_a"].astype(np.int64) * (base["row_a"].astype(np.int64) - 1) // 2 + \
        (base["row_b"].astype(np.int64) - base["row_a"])
    for f in base.dtype.names:
        out[f][at] = base[f]
    kept = np.zeros(n_cells, bool)
    kept[at] = True
    # the dense matrices of the cells with a placement
    c = cells["query_oligo"].astype(np.int64) * n_ol + cells["target_oligo"]
    place = np.zeros(n_ol * n_ol, np.int64)
    place[c] = cells["n_placements"]
    live = np.zeros(n_ol * n_ol, bool)
    live[c] = keep
    where = np.full(n_ol * n_ol, -1, np.int64)
    where[c] = np.arange(len(cells))
    # the eight ordered cells of every pair, ascending; a repeat is equal to its left neighbour
    f, r = ids[0::2], ids[1::2]
    A, B = out["row_a"].astype(np.int64), out["row_b"].astype(np.int64)
    cand = []
    for qa in (f[A], r[A]):
        for tb in (f[B], r[B]):
            cand += [qa * n_ol + tb, tb * n_ol + qa]
    cand = np.sort(np.stack(cand, axis=1), axis=1)
    first = np.ones(cand.shape, bool)
    first[:, 1:] = cand[:, 1:] != cand[:, :-1]
    out["ext_placements"] = (place[cand] * first).sum(axis=1)
    ok = live[cand] & first
    out["ext_cells"] = ok.sum(axis=1)
    # the best kept cell: walk the columns in (q, t) order, a later one wins only if it is strictly better
    best = np.full(n_cells, -1, np.int64)
    dg = np.zeros(n_cells, np.float32)
    run = np.zeros(n_cells, np.int64)
    for k in range(8):
        w = where[cand[:, k]]
        d_k = cells["dG"][w]
        r_k = cells["run"][w].astype(np.int64)
        better = ok[:, k] & ((best < 0) | (d_k < dg) | ((d_k == dg) & (r_k > run)))
        best[better], dg[better], run[better] = w[better], d_k[better], r_k[better]
    has = best >= 0
    out["ext_query"][has] = cells["query_oligo"][best[has]]
    out["ext_target"][has] = cells["target_oligo"][best[has]]
    for name in CELL_FIELDS:
        out["ext_" + name][has] = cells[name][best[has]]
    out["flags"][has] |= 4
    return out[kept | has]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--full-scale", type=float, default=0.05, help="the share of the targets the full pool runs on")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--min-run", type=int, default=4)
    ap.add_argument("--min-extension", type=int, default=1)
    ap.add_argument("--dg-max", type=float, default=-3.0)
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pool_conflicts_ext: no GPU")
    from pcramp_amd import api, synth
    from bench_pool_dimers_end3 import _Words
    import pool_dimer_cases as PC
    W = api.W
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    amp = (80, 200)
    runs = [("panel", a.scale, None)]
    if not a.skip_full:
        runs.append(("full", a.scale * a.full_scale, PC.full_pool(_Words())))
    for name, scale, pool in runs:
        wl = synth.workload(a.config, 0, scale)
        pool = wl["pairs"] if pool is None else pool
        d = api.Screener(0)
        d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
        n_entries = d.select_sites(W.pairs_array(pool), thr2, 18)
        n_cells = len(pool) * (len(pool) + 1) // 2                                # a buffer for every cell: one call, no count call first
        kw = dict(amp_min=amp[0], amp_max=amp[1], dimers=None, select=False, cap=n_cells)
        xkw = dict(min_run=a.min_run, min_extension=a.min_extension, rule="pool")
        ext = lambda: d.pool_conflicts(pool, a.threshold, ext_min_run=a.min_run, ext_min_extension=a.min_extension, ext_dg_max=a.dg_max, **kw)
        ids, rec = ext()
        ids1, every = d.pool_dimers_end3(pool, **xkw)                             # every cell with a placement: sizes the buffer
        n_kept = int((every["dG"] <= np.float32(a.dg_max)).sum())

        def two_calls():
            i, base = d.pool_conflicts(pool, a.threshold, **kw)
            _, cells = d.pool_dimers_end3(pool, dg_max=a.dg_max, cap=(max(n_kept, 1), 0), **xkw)
            return i, base, cells

        def host_route():
            # ext_placements counts the placements of cells the filter drops as well: the route needs the unfiltered cells for them
            i, base = d.pool_conflicts(pool, a.threshold, **kw)
            _, cells = d.pool_dimers_end3(pool, cap=(len(every), 0), **xkw)
            return host_ext(api.POOL_CONFLICT_EXT_DTYPE, i, base, cells, cells["dG"] <= np.float32(a.dg_max))

        # ---- the legs agree before any is timed
        if ids.tolist() != ids1.tolist():
            sys.exit("the oligo numbering differs")
        if not (rec["ext_cells"] > 0).any():
            sys.exit("no extensible dimer: nothing is compared")
        if len(two_calls()[2]) != n_kept:
            sys.exit("the filtered cell records differ in number")
        if host_route().tobytes() != rec.tobytes():
            sys.exit("host_ext's records differ from pool_conflicts_ext's (%s)" % name)

        legs = [("ext", ext), ("two_calls", two_calls), ("host_route", host_route)]
        ts = {leg: [] for leg, _ in legs}
        for k in range(a.warmup + a.repeats):
            for leg, call in legs:
                t0 = time.perf_counter()
                call()
                d.synchronize()
                if k >= a.warmup:
                    ts[leg].append((time.perf_counter() - t0) * 1e3)
        n_ol = int(ids.max()) + 1
        common = dict(pool=name, config=a.config, scale=scale, targets=int(wl["T"]), pairs=len(pool), oligos=n_ol, entries=int(n_entries),
                      row_pairs=n_cells, records=int(len(rec)), with_products=int((rec["products"] > 0).sum()),
                      with_extension=int((rec["ext_cells"] > 0).sum()), dimer_cells=n_ol * n_ol, cells_with_placement=int(len(every)),
                      cells_kept=n_kept, placements=int(every["n_placements"].sum()), min_run=a.min_run, min_extension=a.min_extension,
                      dg_max=a.dg_max, rounds=a.repeats)
        for leg, _ in legs:
            print(json.dumps(dict(call=leg, median_ms=round(statistics.median(ts[leg]), 3), min_ms=round(min(ts[leg]), 3),
                                  max_ms=round(max(ts[leg]), 3), **common)), flush=True)
        d.close()


if __name__ == "__main__":
    main()
