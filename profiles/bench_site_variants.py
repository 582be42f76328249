"""Times pcr_site_variants beside the route it replaces (stand-alone; bench.py is untouched).  Needs a GPU.

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs) after
select_sites(pairs, float32(0.9)**2): every binding site of the panel at 0.81.  The legs are timed alternately, round by round,
on warm buffers: a host clock around synchronous calls.  Every line gives the median of --repeats rounds with the minimum and
maximum, and the sites, variants and (variant, expansion) jobs the call itself counts (counts[0], the return value, counts[1]).

  site_variants         Screener.site_variants(panel, 0.9): grouped on the device, one melt per variant.
  site_variants_cold    the same with thermo=False: the census alone.
  site_variants_map     with site_map=True (one count-only call first, then the call).
  site_tm_unique        what a caller without it does: Screener.site_tm (one melt per site), then for every record the bases
                        loc5 - 1 .. loc3 + 1 cut from the host copy of the sequences (words.unpack_codes, done once outside
                        the timed part and reported as unpack_ms), reverse-complemented for strand 2, and np.unique over
                        (oligo, bases).  Its rows count what the sequences spell, the device's what the word DB's entries
                        spell: the two differ only at sequence ends and splits, so `rows` is printed beside `variants`.

    python profiles/bench_site_variants.py
    python profiles/bench_site_variants.py --family 10000 --repeats 3      # the same targets as one family: a conserved set

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


def host_unique(W, codes, first_code, lengths, rec):
    """np.unique over (oligo, the template bases under and beside the site, oligo-oriented) of site_tm's records -> rows."""
    rows = 0
    for o in np.unique(rec["oligo"]):
        r = rec[rec["oligo"] == o]
        width = int(r["loc3"][0] - r["loc5"][0]) + 3
        at = r["loc5"].astype(np.int64)[:, None] - 1 + np.arange(width, dtype=np.int64)[None, :]
        inside = (at >= 0) & (at < lengths[r["sequence"]].astype(np.int64)[:, None])
        got = codes[np.where(inside, at, 0) + first_code[r["sequence"]][:, None]]
        got = np.where(inside, got, 0).astype(np.uint8)
        minus = r["strand"] == 2
        got[minus] = W._COMP[got[minus]][:, ::-1]
        rows += len(np.unique(got, axis=0))
    return rows


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
        sys.exit("bench_site_variants: no GPU")
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale, family=a.family)
    panel = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(panel), thr2, 18)

    # what the call counts
    pa = W.pairs_array(panel)
    ids = np.zeros(2 * len(panel), np.uint32)
    args = api.ThermoArgs(0.05, 9e-7, 0.0, 0.0, 0.0, 0.0)
    counts = np.zeros(2, np.uint64)
    n_var = int(d.L.pcr_site_variants(d.h, api.TARGET, pa.ctypes.data, len(panel), a.threshold, C.byref(args), 0.0, ids.ctypes.data,
                                      None, 0, None, 0, counts.ctypes.data))
    if n_var < 0:
        sys.exit(api._err(d.L))
    out = np.zeros(max(n_var, 1), api.SITE_VARIANT_DTYPE)
    d.L.pcr_site_variants(d.h, api.TARGET, pa.ctypes.data, len(panel), a.threshold, C.byref(args), 0.0, ids.ctypes.data,
                          out.ctypes.data, n_var, None, 0, counts.ctypes.data)
    n_sites, n_jobs = int(counts[0]), int(counts[1])
    _, rec = d.site_tm(panel, a.threshold)
    site_jobs = int(rec["n_expansions"].sum())
    assert len(rec) == n_sites and n_jobs <= site_jobs

    t0 = time.perf_counter()
    codes = W.unpack_codes(wl["packed"], 2 * len(wl["packed"]))
    unpack_ms = (time.perf_counter() - t0) * 1e3
    first_code = 2 * np.asarray(wl["byte_offsets"], dtype=np.int64)
    lengths = np.asarray(wl["lengths"], dtype=np.int64)
    rows = [0]

    def site_tm_unique():
        _, r = d.site_tm(panel, a.threshold, cap=n_sites)
        rows[0] = host_unique(W, codes, first_code, lengths, r)

    cap = max(n_var, 1)
    legs = [("site_variants", lambda: d.site_variants(panel, a.threshold, cap=cap)),
            ("site_variants_cold", lambda: d.site_variants(panel, a.threshold, thermo=False, cap=cap)),
            ("site_variants_map", lambda: d.site_variants(panel, a.threshold, site_map=True, cap=cap)),
            ("site_tm", lambda: d.site_tm(panel, a.threshold, cap=n_sites)),
            ("site_tm_unique", site_tm_unique)]
    ts = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.repeats):
        for name, call in legs:
            t0 = time.perf_counter()
            call()
            if k >= a.warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    common = dict(config=a.config, scale=a.scale, family=a.family, targets=int(wl["T"]), pairs=len(panel), threshold=a.threshold, entries=int(n_entries),
                  sites=n_sites, variants=n_var, jobs=n_jobs, site_tm_jobs=site_jobs, rounds=a.repeats)
    for name, _ in legs:
        line = dict(call=name, median_ms=round(statistics.median(ts[name]), 3), min_ms=round(min(ts[name]), 3),
                    max_ms=round(max(ts[name]), 3), **common)
        if name == "site_tm_unique":
            line.update(rows=rows[0], unpack_ms=round(unpack_ms, 1))
        print(json.dumps(line), flush=True)
    d.close()


if __name__ == "__main__":
    main()
