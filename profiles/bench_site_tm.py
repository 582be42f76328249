"""Times pcr_site_tm beside the host route it replaces (stand-alone; bench.py is untouched).

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs) after
select_sites(pairs, float32(0.9)**2): every binding site of the panel at 0.81.  Every line is the median of --repeats
host-clock timings of the synchronous call on warm buffers, with the minimum and maximum.

  site_tm     Screener.site_tm(panel, 0.9, select=False) with cap sized by a count-only call first.
  host_route  what a caller without pcr_site_tm does: Screener.entries(), the target strings cut in Python, one fake
              (oligo, target word) pair per site through pcr_dimer (Screener.max_dimer_tm).  It applies max_dimer_tm's strand
              rule (both concentrations primer_strand / degeneracy), so only its time is comparable, not its values.

    python profiles/bench_site_tm.py
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_site_tm.py     # k_site_tm beside k_thermo_wave, per job:
                                                                                  # the lines give launches and jobs per launch

The host_route line needs nothing this call added: copied into the commit before it, the script reports that line only.
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

_BASE = {1: "A", 2: "C", 4: "G", 8: "T"}
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def host_route(d, W, oligos, thr2):
    """entries() -> Python string cutting -> pcr_dimer on fake pairs.  -> (sites, jobs)."""
    entries = d.entries()
    slots = np.array([W.slots_from_word((e[0], e[1])) for e in entries], dtype=np.uint8).reshape(len(entries), 32)
    fake, jobs = [], 0
    for c in oligos:
        cs = np.asarray(W.slots_from_word(c), dtype=np.uint8)
        occ = np.nonzero(cs)[0]
        start, stop = int(occ[0]), int(occ[-1])
        floor = int(np.float32(len(occ)) * np.float32(thr2))
        hit = np.nonzero(((slots & cs) != 0).sum(axis=1) >= floor)[0]
        degen = int(W.word_degeneracy(c))
        seen = set()
        for i in hit:
            e = entries[i]
            if e[4] not in (1, 2) or (e[3], e[2], e[4]) in seen:
                continue
            seen.add((e[3], e[2], e[4]))
            t = [int(v) for v in slots[i][max(start - 1, 0):min(stop + 1, 31) + 1]]
            while t and not t[0]:
                t.pop(0)
            while t and not t[-1]:
                t.pop()
            if not t or any(v not in _BASE for v in t):
                continue
            target = "".join(_COMP[_BASE[v]] for v in reversed(t))
            fake.append((c, W.centered_word(W.codes_from_text(target))))
            jobs += degen
    tm = d.max_dimer_tm(fake) if fake else np.zeros(0, np.float32)
    return len(tm), jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--threshold", type=float, default=0.9)
    a = ap.parse_args()

    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale)
    panel = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(panel), thr2, 18)
    common = dict(config=a.config, scale=a.scale, targets=int(wl["T"]), pairs=len(panel), threshold=a.threshold, entries=int(n_entries),
                  launches=a.repeats + a.warmup + 1)

    if hasattr(api.Screener, "site_tm"):
        ids, rec = d.site_tm(panel, a.threshold, select=False)
        cap = max(len(rec), 1)
        ts = measure(lambda: d.site_tm(panel, a.threshold, select=False, cap=cap), a.repeats, a.warmup)
        print(json.dumps(dict(call="site_tm", items=int(len(rec)), jobs=int(rec["n_expansions"].sum()), records=int(len(rec)),
                              no_tm=int((rec["flags"] & 1).sum()), median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                              max_ms=round(max(ts), 4), **common)), flush=True)

    oligos = []
    for f, r in panel:
        for w in ((int(f[0]), int(f[1])), (int(r[0]), int(r[1]))):
            if w not in oligos:
                oligos.append(w)
    sites, jobs = host_route(d, W, oligos, thr2)
    ts = measure(lambda: host_route(d, W, oligos, thr2), a.repeats, a.warmup)
    print(json.dumps(dict(call="host_route", items=int(sites), jobs=int(jobs), median_ms=round(statistics.median(ts), 4),
                          min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), **common)), flush=True)
    d.close()


if __name__ == "__main__":
    main()
