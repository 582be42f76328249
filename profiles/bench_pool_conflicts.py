"""Times pcr_pool_conflicts beside the host route it replaces (stand-alone; bench.py is untouched).  Needs a GPU.

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs) after
select_sites(pool, float32(0.9)**2): every binding site of the pool at 0.81; --family 10000 makes the same targets one family, a
conserved set where one cell can receive a product from every sequence.  The legs are timed alternately, round by round, on warm
buffers: a host clock around synchronous calls.  Every line gives the median of --repeats rounds with the minimum and maximum.

  conflicts             Screener.pool_conflicts(pool, 0.9, dimers=None, cap=every cell): the records of the cells with a product,
                        one call of pcr_pool_conflicts (without cap the wrapper makes a count call first: twice the time).
  conflicts_dimers      the same with dimers="pool", dimer_floor=0: every cell, with the dimer fields.
  host_route            what a caller did before: Screener.pool_products_tm(tm_floor=0) with every record (cap sized beforehand),
                        Screener.pool_dimers(rule="pool") with every cell, and host_conflicts below: the grouping in numpy.
  host_products_only    host_route without pool_dimers and the dimer part of the grouping: conflicts' counterpart.

The script fails unless host_conflicts' records equal the device's byte for byte, with and without dimers.

    python profiles/bench_pool_conflicts.py
    python profiles/bench_pool_conflicts.py --family 10000

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


def host_conflicts(dtype, ids, rec, dimer_cells=None, dimer_floor=0.0):
    """Every record of pool_products_tm(tm_floor=0), and with dimer_cells every cell of pool_dimers -> the records of
    pcr_pool_conflicts at tm_floor = 0: its definition in numpy."""
    ids = np.asarray(ids, np.int64)
    n_pool = len(ids) // 2
    n_ol = int(ids.max()) + 1 if n_pool else 0
    n_cells = n_pool * (n_pool + 1) // 2
    sp = rec[rec["intended"] == 0]
    v = np.minimum(sp["tm_plus"], sp["tm_minus"]) + np.float32(0.0)
    # rows of every oligo; a product of (x, y) belongs to the unordered pairs of rows(x) x rows(y), once each
    rows = [[] for _ in range(n_ol)]
    for i in range(n_pool):
        for o in sorted({int(ids[2 * i]), int(ids[2 * i + 1])}):
            rows[o].append(i)
    start = lambda a: a * n_pool - a * (a - 1) // 2
    key = sp["plus_oligo"].astype(np.int64) * n_ol + sp["minus_oligo"]
    order = np.argsort(key, kind="stable")
    bounds = np.flatnonzero(np.diff(key[order], prepend=-1, append=-1))
    cell_parts, at_parts = [], []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        x, y = divmod(int(key[order[lo]]), n_ol)
        for a, b in sorted({(min(i, j), max(i, j)) for i in rows[x] for j in rows[y]}):
            cell_parts.append(np.full(hi - lo, start(a) + b - a, np.int64))
            at_parts.append(order[lo:hi])
    out = np.zeros(n_cells, dtype)
    a_of = np.repeat(np.arange(n_pool), np.arange(n_pool, 0, -1))
    out["row_a"] = a_of
    out["row_b"] = np.arange(n_cells) - (a_of * n_pool - a_of * (a_of - 1) // 2) + a_of
    out["melt"] = np.float32(-1.0)
    if cell_parts:
        cell, at = np.concatenate(cell_parts), np.concatenate(at_parts)
        out["products"] = np.bincount(cell, minlength=n_cells)
        seq = sp["sequence"][at].astype(np.int64)
        pairs = np.unique(cell * (int(seq.max()) + 1) + seq)
        out["sequences"] = np.bincount(pairs // (int(seq.max()) + 1), minlength=n_cells)
        # the highest v, then the lowest sequence: one integer key per attribution (v >= +0 orders like its bits)
        best = (v[at].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (~sp["sequence"][at]).astype(np.uint64)
        top = np.zeros(n_cells, np.uint64)
        np.maximum.at(top, cell, best)
        has = out["products"] > 0
        out["melt"][has] = (top[has] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        out["melt_sequence"][has] = ~(top[has] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        out["flags"][has] |= 1
    keep = out["products"] > 0
    if dimer_cells is not None:
        m = np.zeros((n_ol, n_ol), np.float32)
        m[dimer_cells["query_oligo"], dimer_cells["target_oligo"]] = dimer_cells["tm_max"]
        f, r = ids[0::2], ids[1::2]
        A, B = out["row_a"].astype(np.int64), out["row_b"].astype(np.int64)
        cand = []
        for qa in (f[A], r[A]):
            for tb in (f[B], r[B]):
                cand += [qa * n_ol + tb, tb * n_ol + qa]
        cand = np.sort(np.stack(cand, axis=1), axis=1)                              # ascending (q, t): argmax takes the first maximum
        tm = m.reshape(-1)[cand]
        k = np.argmax(tm, axis=1)
        pick = cand[np.arange(n_cells), k]
        out["dimer_tm"] = tm[np.arange(n_cells), k]
        out["dimer_query"], out["dimer_target"] = pick // n_ol, pick % n_ol
        fl = np.float32(dimer_floor)
        out["flags"][out["dimer_tm"] >= fl] |= 2
        keep |= (out["dimer_tm"] >= fl) if fl > 0 else np.ones(n_cells, bool)
    return out[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--family", type=int, default=50, help="sequences per family; 10000 makes the C2 targets one family: a conserved set")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.9)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pool_conflicts: no GPU")
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale, family=a.family)
    pool = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    amp = (80, 200)
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(pool), thr2, 18)

    n_cells = len(pool) * (len(pool) + 1) // 2                                    # a buffer for every cell: one call, no count call first
    conflicts = lambda dimers: d.pool_conflicts(pool, a.threshold, amp_min=amp[0], amp_max=amp[1], dimers=dimers, select=False, cap=n_cells)
    ids, rec_plain = conflicts(None)
    _, rec_dimers = conflicts("pool")
    ids0, all_rec = d.pool_products_tm(pool, a.threshold, tm_floor=0.0, amp_min=amp[0], amp_max=amp[1], select=False)
    cap = max(len(all_rec), 1)

    def host_route(dimers):
        i, rec = d.pool_products_tm(pool, a.threshold, tm_floor=0.0, amp_min=amp[0], amp_max=amp[1], select=False, cap=cap)
        cells = d.pool_dimers(pool, rule="pool")[1] if dimers else None
        return host_conflicts(api.POOL_CONFLICT_DTYPE, i, rec, cells)

    # ---- the legs agree before any is timed
    if not len(rec_plain):
        sys.exit("no spurious product: nothing is compared")
    if ids.tolist() != ids0.tolist():
        sys.exit("the oligo numbering differs")
    for dimers, want in ((False, rec_plain), (True, rec_dimers)):
        if host_route(dimers).tobytes() != want.tobytes():
            sys.exit("host_conflicts' records differ from pool_conflicts' (dimers: %s)" % dimers)

    legs = [("conflicts", lambda: conflicts(None)),
            ("conflicts_dimers", lambda: conflicts("pool")),
            ("host_route", lambda: host_route(True)),
            ("host_products_only", lambda: host_route(False))]
    ts = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.repeats):
        for name, call in legs:
            t0 = time.perf_counter()
            call()
            d.synchronize()
            if k >= a.warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    spurious = int((all_rec["intended"] == 0).sum())
    common = dict(config=a.config, scale=a.scale, family=a.family, targets=int(wl["T"]), pairs=len(pool), threshold=a.threshold,
                  entries=int(n_entries), products=int(len(all_rec)), spurious=spurious, attributions=int(rec_plain["products"].sum()),
                  cells_with_products=int(len(rec_plain)), heaviest_cell=int(rec_plain["products"].max()), cells=int(len(rec_dimers)),
                  rounds=a.repeats)
    for name, _ in legs:
        print(json.dumps(dict(call=name, median_ms=round(statistics.median(ts[name]), 3), min_ms=round(min(ts[name]), 3),
                              max_ms=round(max(ts[name]), 3), **common)), flush=True)
    d.close()


if __name__ == "__main__":
    main()
