"""Times pcr_pool_anneal_profile beside the routes it replaces (stand-alone; bench.py is untouched).  Needs a GPU.

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs) after
select_sites(pool, float32(0.9)**2): every binding site of the pool at 0.81; --family 10000 makes the same targets one family, a
conserved set where every pair amplifies most sequences.  The gradient is np.arange(50, 70.5, 0.5): 41 temperatures.  The legs are
timed alternately, round by round, on warm buffers: a host clock around synchronous calls.  Every line gives the median of
--repeats rounds with the minimum and maximum.

  anneal_profile        Screener.anneal_profile(pool, temps, 0.9): points and pair_sequences.
  anneal_profile_melt   the same with melt=True: both melt matrices and the spurious vector come back too.
  products_tm_loop      (a) what a caller does today: pcr_pool_products_tm(tm_floor=T, both bitsets, cap = 0) once per temperature,
                        the calls alone -- the population counts that turn its rows into pair_sequences are not timed.
  records_numpy         (b) one Screener.pool_products_tm(tm_floor=0) with every record (cap sized beforehand), then host_profile
                        below: the group-by and the histograms in numpy, giving every output of anneal_profile(melt=True).
  products_tm_single    (c) one of (a)'s calls, at the middle temperature: one melt and one join, the floor no design with a
                        single melt and a single join can beat.

The script fails unless (b)'s outputs equal anneal_profile's bit for bit and (a)'s counts and rows agree with its points,
pair_sequences and melt matrices at every temperature.

    python profiles/bench_anneal_profile.py
    python profiles/bench_anneal_profile.py --family 10000

Prints one JSON object per line.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_profile(point_dtype, ids, rec, temps, n_seq):
    """Every record of pool_products_tm(tm_floor=0) -> (points, pair_sequences, melt_fr, melt_rf, melt_spurious): the
    definition of pcr_pool_anneal_profile in numpy."""
    ids = np.asarray(ids, np.int64)
    n_pool, n_t = len(ids) // 2, len(temps)
    n_ol = int(ids.max()) + 1
    v = np.minimum(rec["tm_plus"], rec["tm_minus"]) + np.float32(0.0)
    # temps ascends and v >= 0: the kept temperatures are those <= v (a temperature <= 0 is below every v)
    u = np.searchsorted(temps, v, side="right")
    intended = rec["intended"] != 0
    points = np.zeros(n_t, point_dtype)
    points["temperature"] = temps
    for field, mask in (("products_intended", intended), ("products_spurious", ~intended)):
        hist = np.bincount(u[mask], minlength=n_t + 1)
        points[field] = (hist[::-1].cumsum()[::-1])[1:]                          # kept at t: u > t
    seq = rec["sequence"].astype(np.int64)
    key = rec["plus_oligo"].astype(np.int64) * n_ol + rec["minus_oligo"]          # ascending: the records are in key order
    fr, rf = np.full((n_pool, n_seq), -1.0, np.float32), np.full((n_pool, n_seq), -1.0, np.float32)
    for i in range(n_pool):
        f, r = int(ids[2 * i]), int(ids[2 * i + 1])
        for m, k in ((fr, f * n_ol + r), (rf, r * n_ol + f)):
            lo, hi = np.searchsorted(key, [k, k + 1])
            np.maximum.at(m[i], seq[lo:hi], v[lo:hi])
    spur = np.full(n_seq, -1.0, np.float32)
    np.maximum.at(spur, seq[~intended], v[~intended])

    def kept_counts(m):                                                          # rows of melt values -> [rows, n_t]
        has = m >= 0
        uu = np.where(has, np.searchsorted(temps, m, side="right"), 0)
        flat = (np.arange(m.shape[0])[:, None] * (n_t + 1) + uu)[has]
        hist = np.bincount(flat, minlength=m.shape[0] * (n_t + 1)).reshape(m.shape[0], n_t + 1)
        return hist[:, ::-1].cumsum(axis=1)[:, ::-1][:, 1:]

    pair_seq = kept_counts(np.maximum(fr, rf)).astype(np.uint32)
    points["cells"] = pair_seq.sum(axis=0, dtype=np.uint64)
    points["spurious_sequences"] = kept_counts(spur[None, :])[0]
    return points, pair_seq, fr, rf, spur


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
        sys.exit("bench_anneal_profile: no GPU")
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale, family=a.family)
    pool = wl["pairs"]
    temps = np.arange(50, 70.5, 0.5).astype(np.float32)
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    amp = (80, 200)
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(pool), thr2, 18)
    n_seq, words = int(d.num_sequences()), int(d.bitset_words())

    profile = lambda melt: d.anneal_profile(pool, temps, a.threshold, amp_min=amp[0], amp_max=amp[1], select=False, melt=melt)
    ids, points, pair_seq, fr, rf, spur = profile(True)
    ids0, all_rec = d.pool_products_tm(pool, a.threshold, tm_floor=0.0, amp_min=amp[0], amp_max=amp[1], select=False)
    cap = max(len(all_rec), 1)

    # (a) / (c): the raw call, count and both bitsets, no record
    arr = W.pairs_array(pool)
    oid = np.zeros(2 * len(pool), np.uint32)
    targs = api.ThermoArgs(0.05, 9e-7, 0.0, 0.0, 0.0, 0.0)
    bfr, brf = np.zeros((len(pool), words), np.uint64), np.zeros((len(pool), words), np.uint64)

    def products_tm_bits(tm_floor):
        n = d.L.pcr_pool_products_tm(d.h, api.TARGET, arr.ctypes.data, len(pool), float(a.threshold), amp[0], amp[1], C.byref(targs), 0.0,
                                     float(tm_floor), oid.ctypes.data, None, 0, bfr.ctypes.data, brf.ctypes.data)
        if n < 0:
            sys.exit(api._err(d.L))
        return n

    def loop():
        for t in temps:
            products_tm_bits(t)

    def records_numpy():
        i, rec = d.pool_products_tm(pool, a.threshold, tm_floor=0.0, amp_min=amp[0], amp_max=amp[1], select=False, cap=cap)
        return host_profile(api.ANNEAL_POINT_DTYPE, i, rec, temps, n_seq)

    # ---- the legs agree before any is timed
    if int(points[0]["products_intended"] + points[0]["products_spurious"]) == 0 or not pair_seq.any():
        sys.exit("no product at the lowest temperature: nothing is compared")
    for got, want, what in zip(records_numpy(), (points, pair_seq, fr, rf, spur), ("points", "pair_sequences", "melt_fr", "melt_rf", "melt_spurious")):
        if np.ascontiguousarray(got).tobytes() != np.ascontiguousarray(want).tobytes():
            sys.exit("records_numpy's %s differ from anneal_profile's" % what)
    for t, temp in enumerate(temps):
        n = products_tm_bits(temp)
        if n != int(points[t]["products_intended"] + points[t]["products_spurious"]):
            sys.exit("pool_products_tm at %.1f counts %d products, the profile %d" % (temp, n, int(points[t]["products_intended"] + points[t]["products_spurious"])))
        if bfr.tobytes() != api.melt_to_bits(fr, temp).tobytes() or brf.tobytes() != api.melt_to_bits(rf, temp).tobytes():
            sys.exit("pool_products_tm's rows at %.1f differ from melt_to_bits" % temp)
        pop = np.unpackbits((bfr | brf).view(np.uint8), axis=1).sum(axis=1)
        if pop.tolist() != pair_seq[:, t].tolist():
            sys.exit("pool_products_tm's rows at %.1f do not have pair_sequences' populations" % temp)

    legs = [("anneal_profile", lambda: profile(False)),
            ("anneal_profile_melt", lambda: profile(True)),
            ("products_tm_loop", loop),
            ("records_numpy", records_numpy),
            ("products_tm_single", lambda: products_tm_bits(temps[len(temps) // 2]))]
    ts = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.repeats):
        for name, call in legs:
            t0 = time.perf_counter()
            call()
            d.synchronize()
            if k >= a.warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    top = api.anneal_ceiling(points, pair_seq, keep=1.0)
    common = dict(config=a.config, scale=a.scale, family=a.family, targets=int(wl["T"]), pairs=len(pool), threshold=a.threshold,
                  temperatures=len(temps), entries=int(n_entries), products=int(len(all_rec)), spurious=int((all_rec["intended"] == 0).sum()),
                  cells_at_lowest=int(points[0]["cells"]), cells_at_highest=int(points[-1]["cells"]), ceiling=float(temps[top]) if top >= 0 else None,
                  rounds=a.repeats)
    for name, _ in legs:
        print(json.dumps(dict(call=name, median_ms=round(statistics.median(ts[name]), 3), min_ms=round(min(ts[name]), 3),
                              max_ms=round(max(ts[name]), 3), **common)), flush=True)
    d.close()


if __name__ == "__main__":
    main()
