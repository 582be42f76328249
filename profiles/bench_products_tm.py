"""Times pcr_pool_products_tm beside the host route it replaces (stand-alone; bench.py is untouched).

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %) after select_sites(pool,
float32(0.9)**2): every binding site of the pool at 0.81.  --pairs 50 is the workload's panel; any other number samples that many
pairs from the same sequences with synth.make_pairs (--pairs 500: the denser case).  Every line is the median of --repeats
host-clock timings of the synchronous call on warm buffers, ending in a synchronise, with the minimum and maximum.

  products_tm       Screener.pool_products_tm(pool, 0.9, tm_floor, bits=True), cap sized beforehand: kept records and both bitsets.
  products_tm_bits  the same call with cap = 0: the count and both bitsets, no record leaves the device.
  host_route        what a caller without the call does: Screener.pool_products + Screener.site_tm (caps sized beforehand) +
                    Screener.product_tm + the floor and the bit packing in numpy.

The script fails unless the host route's kept records, Tm and bits equal products_tm's; every line carries a checksum of them.

    python profiles/bench_products_tm.py [--pairs 500]
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_products_tm.py --only products_tm   # the share of k_site_tm

The host_route line needs nothing this call added: copied into the commit before it, the script reports that line only (compare
the checksums).  Prints one JSON object per line.
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

FIELDS8 = ["plus_oligo", "minus_oligo", "sequence", "begin", "end", "inner_start", "inner_length", "intended"]


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def host_route(d, pool, thr, tm_floor, amp, caps, words):
    """-> (kept pool_products records, tm_plus, tm_minus, fr, rf)"""
    ids, prod = d.pool_products(pool, thr, amp[0], amp[1], select=False, cap=caps[0])
    _, sites = d.site_tm(pool, thr, select=False, cap=caps[1])
    d.synchronize()
    plus, minus = d.product_tm(prod, sites)
    keep = np.minimum(plus, minus) >= np.float32(tm_floor) if tm_floor > 0 else np.ones(len(prod), bool)
    kept, plus, minus = prod[keep], plus[keep], minus[keep]
    n_ol = int(ids.max()) + 1
    key = kept["plus_oligo"].astype(np.int64) * n_ol + kept["minus_oligo"]           # ascending: the records are in key order
    fr, rf = np.zeros((len(pool), words), np.uint64), np.zeros((len(pool), words), np.uint64)
    for i in range(len(pool)):
        f, r = int(ids[2 * i]), int(ids[2 * i + 1])
        for bits, k in ((fr, f * n_ol + r), (rf, r * n_ol + f)):
            lo, hi = np.searchsorted(key, [k, k + 1])
            s = np.unique(kept["sequence"][lo:hi]).astype(np.uint64)
            np.bitwise_or.at(bits[i], (s >> np.uint64(6)).astype(np.int64), np.uint64(1) << (s & np.uint64(63)))
    return kept, plus, minus, fr, rf


def checksum(rec8, plus, minus, fr, rf):
    h = hashlib.sha256()
    for x in (rec8, plus, minus, fr, rf):
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--pairs", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--tm-floor", type=float, default=50.0)
    ap.add_argument("--only", choices=["products_tm", "products_tm_bits", "host_route"], default=None)
    a = ap.parse_args()

    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale)
    pool = wl["pairs"] if a.pairs == len(wl["pairs"]) else synth.make_pairs(wl["packed"], wl["byte_offsets"], wl["lengths"], a.pairs, 9100)
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    amp = (80, 200)
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(pool), thr2, 18)
    words = int(d.bitset_words())
    _, prod = d.pool_products(pool, a.threshold, amp[0], amp[1], select=False)
    _, sites = d.site_tm(pool, a.threshold, select=False)
    caps = (max(len(prod), 1), max(len(sites), 1))
    common = dict(config=a.config, scale=a.scale, targets=int(wl["T"]), pairs=len(pool), threshold=a.threshold, tm_floor=a.tm_floor,
                  entries=int(n_entries), items=int(len(sites)), jobs=int(sites["n_expansions"].sum()), products=int(len(prod)),
                  launches=a.repeats + a.warmup + 1)
    del prod, sites
    line = lambda call, ts, **kw: print(json.dumps(dict(call=call, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                                                        max_ms=round(max(ts), 4), **kw, **common)), flush=True)
    have = hasattr(api.Screener, "pool_products_tm")
    kept, plus, minus, fr, rf = host_route(d, pool, a.threshold, a.tm_floor, amp, caps, words)
    ref_sum = checksum(kept, plus, minus, fr, rf)

    if have:
        run = lambda cap: d.pool_products_tm(pool, a.threshold, tm_floor=a.tm_floor, amp_min=amp[0], amp_max=amp[1], select=False,
                                             bits=True, cap=cap)
        _, rec, gfr, gfr_rf = run(max(len(kept), 1))
        if len(rec) != len(kept) or rec[FIELDS8].tolist() != kept.tolist():
            raise SystemExit("products_tm's kept records differ from the host route's")
        if rec["tm_plus"].tobytes() != plus.tobytes() or rec["tm_minus"].tobytes() != minus.tobytes():
            raise SystemExit("products_tm's Tm differ from the host route's")
        if gfr.tobytes() != fr.tobytes() or gfr_rf.tobytes() != rf.tobytes():
            raise SystemExit("products_tm's bitsets differ from the host route's")
        cap = max(len(rec), 1)

        def full():
            run(cap)
            d.synchronize()

        def bits_only():
            n = d.L.pcr_pool_products_tm(*raw_args)
            if n != len(kept):
                raise SystemExit("the count-only call returned %d, not %d" % (n, len(kept)))
            d.synchronize()

        import ctypes as C
        arr = W.pairs_array(pool)
        ids = np.zeros(2 * len(pool), np.uint32)
        targs = api.ThermoArgs(0.05, 9e-7, 0.0, 0.0, 0.0, 0.0)
        bfr, brf = np.zeros((len(pool), words), np.uint64), np.zeros((len(pool), words), np.uint64)
        raw_args = (d.h, api.TARGET, arr.ctypes.data, len(pool), float(a.threshold), amp[0], amp[1], C.byref(targs), 0.0, float(a.tm_floor),
                    ids.ctypes.data, None, 0, bfr.ctypes.data, brf.ctypes.data)
        if a.only in (None, "products_tm"):
            line("products_tm", measure(full, a.repeats, a.warmup), kept=int(len(kept)), checksum=ref_sum)
        if a.only in (None, "products_tm_bits"):
            ts = measure(bits_only, a.repeats, a.warmup)
            if bfr.tobytes() != fr.tobytes() or brf.tobytes() != rf.tobytes():
                raise SystemExit("the count-only call's bitsets differ from the host route's")
            line("products_tm_bits", ts, kept=int(len(kept)), checksum=ref_sum)
    if a.only in (None, "host_route"):
        ts = measure(lambda: host_route(d, pool, a.threshold, a.tm_floor, amp, caps, words), a.repeats, a.warmup)
        line("host_route", ts, kept=int(len(kept)), checksum=ref_sum)
    d.close()


if __name__ == "__main__":
    main()
