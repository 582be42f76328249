"""Times pcr_pool_probe_candidates beside the host path it replaces (stand-alone; bench.py is untouched).

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %), its pool's products from
Screener.pool_products after select_sites(pool, float32(0.9)**2), each grouped under the pool pair that owns it (the others
take no part).  Every line is the median of --repeats host-clock timings of the synchronous call on warm buffers, with the
minimum and maximum.

  candidates         pcr_pool_probe_candidates without args: enumeration, grouping, support filter, rank and cut.
  candidates_thermo  the same with args: every candidate that min_sequences admits is melted and pcr_thermo's verdict applied.
  host               what a caller without the call does: product_amplicons(..., REGION_INSERT, sequences=True) for the insert
                     texts, then a Python dictionary (group, word) -> sequences and records over the windows that pass the rules
                     (the rules themselves vectorised with numpy), sorted and cut.

The script fails unless the two give the same candidates: group, word, length, sequences and records of every record, in order.
The counts it prints: windows (before the rules, as the call's capacity check adds them up), candidates (distinct (group, word)
that pass the rules), thermo_jobs (the candidates min_sequences admits: what the engine melts), records and records_thermo (what
the call returns without and with args); ns_per_job is the whole call with args divided by thermo_jobs.

    python profiles/bench_probe_candidates.py
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_probe_candidates.py --only candidates   # the share of each kernel

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


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def passing_windows(W, codes, a):
    """The words of one insert that pass the rules, as code bytes (both strands as asked; a word once)."""
    out = set()
    n = len(codes)
    for L in range(a.len_min, min(a.len_max, n) + 1):
        win = np.lib.stride_tricks.sliding_window_view(codes, L)
        win = win[np.isin(win, (1, 2, 4, 8)).all(axis=1)]
        for strand in (1, 2):
            if not (a.strands & strand) or not len(win):
                continue
            w = win if strand == 1 else W._COMP[win][:, ::-1]
            c, g = (w == 2).sum(axis=1), (w == 4).sum(axis=1)
            frac = (c + g).astype(np.float32) / np.float32(L)
            ok = (frac >= np.float32(a.gc_min)) & (frac <= np.float32(a.gc_max))
            if a.no_5g:
                ok &= w[:, 0] != 4
            if a.c_ge_g:
                ok &= c >= g
            if a.max_run and L > a.max_run:
                same = w[:, 1:] == w[:, :-1]
                run = np.lib.stride_tricks.sliding_window_view(same, a.max_run, axis=1).all(axis=2).any(axis=1)
                ok &= ~run
            out.update(bytes(r) for r in np.ascontiguousarray(w[ok]))
    return out


def host_candidates(d, api, W, prod, group, a):
    """-> [(group, word bytes, sequences, records)] in the call's order, cut at per_group."""
    info, texts = d.product_amplicons(prod, api.REGION_INSERT, sequences=True)
    words_of = {}
    table = {}                                                               # (group, word) -> [set of sequences, records]
    for k in range(len(prod)):
        g = int(group[k])
        if g == api.NO_GROUP:
            continue
        c = int(info["amplicon"][k])
        if c not in words_of:
            words_of[c] = passing_windows(W, W.codes_from_text(texts[c]), a)
        s = int(prod["sequence"][k])
        for w in words_of[c]:
            e = table.get((g, w))
            if e is None:
                table[(g, w)] = [{s}, 1]
            else:
                e[0].add(s)
                e[1] += 1
    n_distinct = len(table)
    rows = [(g, w, len(e[0]), e[1]) for (g, w), e in table.items() if len(e[0]) >= a.min_sequences]
    rows.sort(key=lambda r: (r[0], -r[2], -r[3], len(r[1]), r[1]))
    return rows, n_distinct


def cut(rows, per_group):
    out, taken = [], {}
    for r in rows:
        if per_group and taken.get(r[0], 0) >= per_group:
            continue
        taken[r[0]] = taken.get(r[0], 0) + 1
        out.append(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-repeats", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--len-min", type=int, default=20)
    ap.add_argument("--len-max", type=int, default=30)
    ap.add_argument("--strands", type=int, default=3)
    ap.add_argument("--max-run", type=int, default=4)
    ap.add_argument("--gc-min", type=float, default=0.3)
    ap.add_argument("--gc-max", type=float, default=0.8)
    ap.add_argument("--min-sequences", type=int, default=2)
    ap.add_argument("--per-group", type=int, default=8)
    ap.add_argument("--only", choices=["candidates", "candidates_thermo", "host"], default=None)
    a = ap.parse_args()
    a.no_5g = a.c_ge_g = True

    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale)
    pool = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(list(pool)), thr2, 18)
    ids, prod = d.pool_products(pool, a.threshold, 80, 200, select=False, cap=1 << 20)
    if not len(prod):
        raise SystemExit("the pool forms no product: nothing is compared")
    first = {}
    for i in range(len(pool)):
        first.setdefault(frozenset((int(ids[2 * i]), int(ids[2 * i + 1]))), i)
    group = np.array([first.get(frozenset((int(p), int(m))), api.NO_GROUP) for p, m in zip(prod["plus_oligo"], prod["minus_oligo"])], np.uint32)
    rules = api.PROBE_NO_5G | api.PROBE_C_GE_G
    rec = np.ascontiguousarray(prod, api.PRODUCT_DTYPE)
    targs = api.ThermoArgs(0.05, 2.5e-7, 65.0, 75.0, 40.0, 40.0)

    def call(out, cap, thermo, min_sequences=None, per_group=None):
        n = d.L.pcr_pool_probe_candidates(d.h, api.TARGET, rec.ctypes.data, group.ctypes.data, len(rec), a.len_min, a.len_max, a.strands, rules,
                                          a.max_run, a.gc_min, a.gc_max, a.min_sequences if min_sequences is None else min_sequences,
                                          C.byref(targs) if thermo else None, 0, a.per_group if per_group is None else per_group,
                                          None if out is None else out.ctypes.data, cap)
        if n < 0:
            raise SystemExit("pcr_pool_probe_candidates: %s" % api._err(d.L))
        return int(n)

    insert = np.maximum(rec["inner_length"].astype(np.int64) - 12, 0)[group != api.NO_GROUP]
    windows = int(sum(np.maximum(insert - L + 1, 0).sum() for L in range(a.len_min, a.len_max + 1))) * (2 if a.strands == 3 else 1)
    n_distinct = call(None, 0, False, min_sequences=1, per_group=0)
    n_jobs = call(None, 0, False, per_group=0)
    n_rec = call(None, 0, False)
    n_rec_thermo = call(None, 0, True)
    common = dict(config=a.config, scale=a.scale, targets=int(wl["T"]), pairs=len(pool), threshold=a.threshold, entries=int(n_entries),
                  products=int(len(prod)), grouped=int((group != api.NO_GROUP).sum()), windows=windows, candidates=n_distinct, thermo_jobs=n_jobs,
                  records=n_rec, records_thermo=n_rec_thermo, len_min=a.len_min, len_max=a.len_max, min_sequences=a.min_sequences,
                  per_group=a.per_group, launches=a.repeats + a.warmup)
    line = lambda name, ts, **kw: print(json.dumps(dict(call=name, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                                                        max_ms=round(max(ts), 4), **kw, **common)), flush=True)
    # the same candidates: every one that min_sequences admits, in order, and the cut
    out_all = np.zeros(max(n_jobs, 1), api.PROBE_CANDIDATE_DTYPE)
    if call(out_all, n_jobs, False, per_group=0) != n_jobs:
        raise SystemExit("the count changed between two calls")
    rows, host_distinct = host_candidates(d, api, W, prod, group, a)
    as_rows = lambda r: [(int(x["group"]), W.codes_from_text(W.word_text((int(x["word"][0]), int(x["word"][1])))).tobytes(), int(x["sequences"]),
                          int(x["records"])) for x in r]
    if host_distinct != n_distinct or as_rows(out_all[:n_jobs]) != rows:
        raise SystemExit("the device's candidates are not the host's")
    out = np.zeros(max(n_rec, n_rec_thermo, 1), api.PROBE_CANDIDATE_DTYPE)
    if call(out, len(out), False) != n_rec or as_rows(out[:n_rec]) != cut(rows, a.per_group):
        raise SystemExit("the device's cut is not the host's")

    if a.only in (None, "candidates"):
        line("candidates", measure(lambda: call(out, len(out), False), a.repeats, a.warmup))
    if a.only in (None, "candidates_thermo"):
        ts = measure(lambda: call(out, len(out), True), a.repeats, a.warmup)
        line("candidates_thermo", ts, ns_per_job=round(1e6 * (statistics.median(ts)) / max(n_jobs, 1), 1))
    if a.only in (None, "host"):
        line("host", measure(lambda: host_candidates(d, api, W, prod, group, a), a.host_repeats, 0))
    d.close()


if __name__ == "__main__":
    main()
