"""Times pcr_pool_probe_hits beside the composition it replaces (stand-alone; bench.py is untouched).

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %) with one 20-base probe per pair, cut
from the middle of the stretch between the two primers of the product the pair was sampled from, after select_sites(pool + (P, P)
per probe, float32(0.9)**2): every binding site of the primers and the probes at 0.81.  Every line is the median of --repeats
host-clock timings of the synchronous call on warm buffers, ending in a synchronise, with the minimum and maximum.

  probe_hits       Screener.probe_hits(pool, probes, 0.9, tm_floor, probe_tm_floor, bits=True), cap sized beforehand: the kept
                   records and the detected rows.
  probe_hits_bits  the same call with cap = 0: the count and the detected rows, no record leaves the device.
  composition      what a caller without the call does: Screener.pool_products_tm(bits=True) + Screener.site_tm on the panel (P, P)
                   at the probe concentration (caps sized beforehand) + host_join below, in numpy.

The script fails unless the composition's records and rows equal probe_hits' bit for bit; every line carries a checksum of them.

    python profiles/bench_probe_hits.py
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_probe_hits.py --only probe_hits   # the share of each kernel

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

ORDER = ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "probe", "probe_loc5", "probe_strand")
NO_PROBE = 0xFFFFFFFF


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def host_join(hit_dtype, prod, fr, rf, sites, ids, pid, probe_tm_floor):
    """pool_products_tm's kept records and rows + site_tm's records for the panel (P, P) of the distinct probes -> (hit records
    in order, detected rows): the definition of pcr_pool_probe_hits in numpy."""
    ids, pid = np.asarray(ids, np.int64), np.asarray(pid, np.int64)
    by_seq = np.argsort(sites["sequence"], kind="stable")
    ps = sites[by_seq]
    lo, hi = np.searchsorted(ps["sequence"], prod["sequence"], "left"), np.searchsorted(ps["sequence"], prod["sequence"], "right")
    cnt = hi - lo
    pi = np.repeat(np.arange(len(prod)), cnt)
    si = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    p3 = prod["inner_start"][pi].astype(np.int64) + 3
    m5 = prod["inner_start"][pi].astype(np.int64) + prod["inner_length"][pi] - 8
    ok = (ps["loc5"][si] > p3) & (ps["loc3"][si] < m5)
    if np.float32(probe_tm_floor) > 0:
        ok &= ps["tm_max"][si] >= np.float32(probe_tm_floor)
    p, s = prod[pi[ok]], ps[si[ok]]
    hits = np.zeros(len(p), hit_dtype)
    for f in ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "inner_start", "inner_length", "tm_plus", "tm_minus"):
        hits[f] = p[f]
    hits["probe"], hits["probe_loc5"], hits["probe_loc3"], hits["probe_strand"] = s["oligo"], s["loc5"], s["loc3"], s["strand"]
    hits["tm_probe"] = s["tm_max"]
    hits["flags"] = p["flags"] | np.where(s["flags"] & 1, 4, 0).astype(np.uint32)
    n_ol, n_pr = int(ids.max()) + 1 if len(ids) else 1, int(pid[pid != NO_PROBE].max()) + 1 if (pid != NO_PROBE).any() else 1
    assay = lambda a, b, q: (np.minimum(a, b) * n_ol + np.maximum(a, b)) * n_pr + q
    with_probe = pid != NO_PROBE
    pool_key = assay(ids[0::2][with_probe], ids[1::2][with_probe], pid[with_probe])
    hit_key = assay(hits["plus_oligo"].astype(np.int64), hits["minus_oligo"].astype(np.int64), hits["probe"].astype(np.int64))
    hits["intended"] = p["intended"] | np.where(np.isin(hit_key, pool_key), 2, 0).astype(np.uint32)
    order = np.lexsort([hits[f] for f in reversed(ORDER)])
    hits, hit_key = hits[order], hit_key[order]
    detected = fr | rf                                                       # a pair without a probe is detected by its product
    by_key = np.argsort(hit_key, kind="stable")
    sorted_key, sorted_seq = hit_key[by_key], hits["sequence"][by_key]
    for i in np.nonzero(with_probe)[0]:
        k = assay(ids[2 * i], ids[2 * i + 1], pid[i])
        a, b = np.searchsorted(sorted_key, [k, k + 1])
        q = np.unique(sorted_seq[a:b]).astype(np.uint64)
        detected[i] = 0
        np.bitwise_or.at(detected[i], (q >> np.uint64(6)).astype(np.int64), np.uint64(1) << (q & np.uint64(63)))
    return hits, detected


def composition(d, api, pool, panel_pp, thr, tm_floor, probe_tm_floor, probe_strand, amp, caps, pid):
    ids, prod, fr, rf = d.pool_products_tm(pool, thr, tm_floor=tm_floor, amp_min=amp[0], amp_max=amp[1], select=False, bits=True, cap=caps[0])
    _, sites = d.site_tm(panel_pp, thr, primer_strand=probe_strand, select=False, cap=caps[1])
    d.synchronize()
    return host_join(api.PROBE_HIT_DTYPE, prod, fr, rf, sites, ids, pid, probe_tm_floor)


def checksum(hits, detected):
    h = hashlib.sha256()
    for x in (hits, detected):
        h.update(np.ascontiguousarray(x).tobytes())
    return h.hexdigest()[:16]


def probes_of(synth, W, wl, pool, origins, length=20):
    """One probe per pair: `length` bases from the middle of the stretch between the primers of the product it was cut from."""
    out = []
    for (f, r), (t, fs, amp) in zip(pool, origins):
        fl, rl = (sum(1 for x in W.slots_from_word(w) if x) for w in (f, r))
        gap_lo, gap_hi = fs + fl, fs + amp - rl
        at = gap_lo + (gap_hi - gap_lo - length) // 2
        codes = synth.sequence_codes(wl["packed"], wl["byte_offsets"], wl["lengths"], t)[at:at + length]
        if at < gap_lo or at + length > gap_hi or (codes == 0).any():
            raise SystemExit("no room for a probe inside the product of a pair")
        out.append(W.centered_word(codes))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--tm-floor", type=float, default=50.0)
    ap.add_argument("--probe-tm-floor", type=float, default=50.0)
    ap.add_argument("--probe-strand", type=float, default=2.5e-7)
    ap.add_argument("--only", choices=["probe_hits", "probe_hits_bits", "composition"], default=None)
    a = ap.parse_args()

    import ctypes as C
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale)
    pool = wl["pairs"]
    probes = probes_of(synth, W, wl, pool, wl["origins"])
    distinct = list(dict.fromkeys((int(p[0]), int(p[1])) for p in probes))
    panel_pp = [(p, p) for p in distinct]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    amp = (80, 200)
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(list(pool) + panel_pp), thr2, 18)
    words = int(d.bitset_words())
    _, prod = d.pool_products_tm(pool, a.threshold, tm_floor=a.tm_floor, amp_min=amp[0], amp_max=amp[1], select=False)
    _, sites = d.site_tm(panel_pp, a.threshold, primer_strand=a.probe_strand, select=False)
    caps = (max(len(prod), 1), max(len(sites), 1))
    run = lambda cap: d.probe_hits(pool, probes, a.threshold, tm_floor=a.tm_floor, probe_tm_floor=a.probe_tm_floor,
                                   probe_strand=a.probe_strand, amp_min=amp[0], amp_max=amp[1], select=False, bits=True, cap=cap)
    ids, pid, rec, detected = run(1 << 16)
    common = dict(config=a.config, scale=a.scale, targets=int(wl["T"]), pairs=len(pool), probes=len(distinct), threshold=a.threshold,
                  tm_floor=a.tm_floor, probe_tm_floor=a.probe_tm_floor, entries=int(n_entries), products=int(len(prod)),
                  probe_sites=int(len(sites)), hits=int(len(rec)), launches=a.repeats + a.warmup + 1)
    del prod, sites
    line = lambda call, ts, **kw: print(json.dumps(dict(call=call, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                                                        max_ms=round(max(ts), 4), **kw, **common)), flush=True)
    comp = lambda: composition(d, api, pool, panel_pp, a.threshold, a.tm_floor, a.probe_tm_floor, a.probe_strand, amp, caps, pid)
    want, want_detected = comp()
    if len(rec) == 0 or not detected.any():
        raise SystemExit("no hit at these floors: nothing is compared")
    if rec.tobytes() != want.tobytes():
        raise SystemExit("probe_hits' records differ from the composition's")
    if detected.tobytes() != want_detected.tobytes():
        raise SystemExit("probe_hits' detected rows differ from the composition's")
    ref_sum = checksum(want, want_detected)
    cap = max(len(rec), 1)

    def full():
        run(cap)
        d.synchronize()

    arr = W.pairs_array(pool)
    pr = np.array([(int(p[0]), int(p[1])) for p in probes], np.uint64)
    oid, qid = np.zeros(2 * len(pool), np.uint32), np.zeros(len(pool), np.uint32)
    targs = api.ThermoArgs(0.05, 9e-7, 0.0, 0.0, 0.0, 0.0)
    rows = np.zeros((len(pool), words), np.uint64)
    raw_args = (d.h, api.TARGET, arr.ctypes.data, pr.ctypes.data, len(pool), float(a.threshold), amp[0], amp[1], C.byref(targs),
                float(a.probe_strand), 0.0, float(a.tm_floor), float(a.probe_tm_floor), oid.ctypes.data, qid.ctypes.data, None, 0,
                rows.ctypes.data)

    def bits_only():
        n = d.L.pcr_pool_probe_hits(*raw_args)
        if n != len(rec):
            raise SystemExit("the count-only call returned %d, not %d" % (n, len(rec)))
        d.synchronize()

    if a.only in (None, "probe_hits"):
        line("probe_hits", measure(full, a.repeats, a.warmup), checksum=ref_sum)
    if a.only in (None, "probe_hits_bits"):
        ts = measure(bits_only, a.repeats, a.warmup)
        if rows.tobytes() != want_detected.tobytes():
            raise SystemExit("the count-only call's detected rows differ from the composition's")
        line("probe_hits_bits", ts, checksum=ref_sum)
    if a.only in (None, "composition"):
        line("composition", measure(comp, a.repeats, a.warmup), checksum=ref_sum)
    d.close()


if __name__ == "__main__":
    main()
