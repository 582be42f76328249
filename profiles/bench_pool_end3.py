"""Times pcr_pool_products_end3 beside pcr_pool_products_tm and the host route it replaces (stand-alone; bench.py is untouched).
Needs a GPU.

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs) after
select_sites(pool, float32(0.9)**2): every binding site of the pool at 0.81; --family 10000 makes the same targets one family.
The legs are timed alternately, round by round, on warm buffers: a host clock around synchronous calls.  Every line gives the
median of --repeats rounds with the minimum and maximum.

  end3            Screener.pool_products_end3(pool, 0.9, tm_floor, the rule, cap=the count known beforehand): one call of
                  pcr_pool_products_end3, the kept records.
  products_tm     Screener.pool_products_tm with the same other arguments and every record: what the rule costs on top.
  host_route      what a caller did before: pool_products_tm with every record, site_variants(site_map=True, thermo=False),
                  site_tm, and host_end3 below: the join of the three and the rule in numpy.

The script fails unless host_end3's records equal the device's byte for byte.

    python profiles/bench_pool_end3.py
    python profiles/bench_pool_end3.py --family 10000

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

_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def _popcount32(x):
    return _POP8[np.ascontiguousarray(x, dtype=np.uint32).view(np.uint8).reshape(x.shape + (4,))].sum(axis=-1, dtype=np.uint32)


def oligo_lengths(pool, ids):
    """Occupied slots of every distinct oligo, indexed by its id (pool: [(F, R)] words, ids: the call's oligo_id)."""
    out = np.zeros(int(np.max(ids)) + 1 if len(ids) else 0, np.int64)
    for k, w in enumerate(w for pair in pool for w in pair):
        out[int(ids[k])] = sum(1 for half in w for n in range(16) if (int(half) >> (4 * n)) & 0xF)
    return out


def host_end3(dtype, rec, sites, variants, site_map, lengths, min_clamp3=0, window=0, max_end_mismatch=0, ident_threshold=0.0):
    """pool_products_tm's records (past the floor), site_tm's records, site_variants' records with their site map and the oligos'
    lengths -> the records of pcr_pool_products_end3 under a rule without the TaqMAMA factor: its definition in numpy."""
    L = lengths[sites["oligo"].astype(np.int64)]
    var = np.asarray(site_map, np.int64)
    clamp3 = variants["clamp3"][var].astype(np.int64)
    mask = variants["mismatch_mask"][var].astype(np.uint32)                       # bit i: the oligo's i-th base from its 5' end
    win = np.minimum(int(window), L)
    end_mm = _popcount32(np.where(win > 0, mask >> (L - win).astype(np.uint32), 0).astype(np.uint32)).astype(np.int64)
    ident = sites["matches"].astype(np.float32) * (1.0 / L.astype(np.float64)).astype(np.float32)
    site_ok = (clamp3 >= np.minimum(int(min_clamp3), L)) & ((int(window) == 0) | (end_mm <= int(max_end_mismatch)))
    # a product's plus site is (plus_oligo, sequence, loc5 = begin, strand 1), its minus site (minus_oligo, sequence, loc3 = end, strand 2)
    key = lambda oligo, seq, at: (oligo.astype(np.uint64) << np.uint64(52)) | (seq.astype(np.uint64) << np.uint64(32)) | (at.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
    at = {}
    for strand, where, o_f, at_f in ((1, "loc5", "plus_oligo", "begin"), (2, "loc3", "minus_oligo", "end")):
        idx = np.flatnonzero(sites["strand"] == strand)
        k = key(sites["oligo"][idx], sites["sequence"][idx], sites[where][idx])
        order = np.argsort(k, kind="stable")
        want = key(rec[o_f], rec["sequence"], rec[at_f])
        if not len(want):
            at[strand] = np.zeros(0, np.int64)
            continue
        pos = np.minimum(np.searchsorted(k[order], want), max(len(k), 1) - 1)
        if not len(k) or (k[order][pos] != want).any():
            raise ValueError("host_end3: a product has no site record")
        at[strand] = idx[order][pos]
    p, m = at[1], at[2]
    keep = site_ok[p] & site_ok[m]
    thr = np.float32(ident_threshold)
    if thr != 0:
        keep &= np.sqrt(ident[p] * ident[m], dtype=np.float32) >= thr
    out = np.zeros(len(rec), dtype)
    for f in rec.dtype.names:
        out[f] = rec[f]
    out["clamp3_plus"], out["clamp3_minus"] = clamp3[p], clamp3[m]
    out["end_mismatch_plus"], out["end_mismatch_minus"] = end_mm[p], end_mm[m]
    out["id_plus"], out["id_minus"] = ident[p], ident[m]
    return out[keep]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--family", type=int, default=50, help="sequences per family; 10000 makes the C2 targets one family: a conserved set")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--tm-floor", type=float, default=50.0)
    ap.add_argument("--min-clamp3", type=int, default=3)
    ap.add_argument("--window", type=int, default=5)
    ap.add_argument("--max-end-mismatch", type=int, default=1)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_pool_end3: no GPU")
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale, family=a.family)
    pool = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    amp = (80, 200)
    rule = dict(min_clamp3=a.min_clamp3, window=a.window, max_end_mismatch=a.max_end_mismatch)
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(pool), thr2, 18)

    common_kw = dict(tm_floor=a.tm_floor, amp_min=amp[0], amp_max=amp[1], select=False)
    ids, kept, before = d.pool_products_end3(pool, a.threshold, **rule, **common_kw)
    ids0, all_rec = d.pool_products_tm(pool, a.threshold, **common_kw)
    _, sites = d.site_tm(pool, a.threshold)
    cap_tm, cap_end3, cap_sites = max(len(all_rec), 1), max(len(kept), 1), max(len(sites), 1)
    lengths = oligo_lengths(pool, ids)

    def end3():
        return d.pool_products_end3(pool, a.threshold, cap=cap_end3, **rule, **common_kw)

    def products_tm():
        return d.pool_products_tm(pool, a.threshold, cap=cap_tm, **common_kw)

    def host_route():
        _, rec = products_tm()
        _, variants, site_map = d.site_variants(pool, a.threshold, site_map=True, thermo=False, cap=cap_sites)
        _, st = d.site_tm(pool, a.threshold, cap=cap_sites)
        return host_end3(api.PRODUCT_END3_DTYPE, rec, st, variants, site_map, lengths, **rule)

    # ---- the legs agree before any is timed
    if before != len(all_rec):
        sys.exit("n_before_rule differs from pool_products_tm's count")
    if not (0 < len(kept) < before):
        sys.exit("the rule keeps all or nothing: nothing is compared")
    if ids.tolist() != ids0.tolist():
        sys.exit("the oligo numbering differs")
    if host_route().tobytes() != kept.tobytes() or end3()[1].tobytes() != kept.tobytes():
        sys.exit("host_end3's records differ from pool_products_end3's")

    legs = [("end3", end3), ("products_tm", products_tm), ("host_route", host_route)]
    ts = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.repeats):
        for name, call in legs:
            t0 = time.perf_counter()
            call()
            d.synchronize()
            if k >= a.warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    common = dict(config=a.config, scale=a.scale, family=a.family, targets=int(wl["T"]), pairs=len(pool), threshold=a.threshold,
                  tm_floor=a.tm_floor, rule=rule, entries=int(n_entries), sites=int(len(sites)), products_before_rule=int(before),
                  products_kept=int(len(kept)), rounds=a.repeats)
    for name, _ in legs:
        print(json.dumps(dict(call=name, median_ms=round(statistics.median(ts[name]), 3), min_ms=round(min(ts[name]), 3),
                              max_ms=round(max(ts[name]), 3), **common)), flush=True)
    d.close()


if __name__ == "__main__":
    main()
