"""Times pcr_site_repair beside the route it replaces (stand-alone; bench.py is untouched).  Needs a GPU.

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs) after
select_sites(pairs, float32(0.9)**2): every binding site of the panel at 0.81.  The legs are timed alternately, round by round,
on warm buffers: a host clock around synchronous calls.  Every line gives the median of --repeats rounds with the minimum and
maximum, and the sites, variants, step records and steps taken.

  site_repair           Screener.site_repair(panel, 0.9, ...): the greedy on the device, every step's word through is_valid.
  site_repair_cold      the same with thermo=False.
  site_variants_cold    Screener.site_variants(thermo=False) alone: the part the two calls share.
  host_route            what a caller without it does: site_variants(site_map=True, thermo=False) + site_tm for each site's
                        sequence, the per-oligo variant and (variant, sequence) tables rebuilt in numpy, the same greedy
                        with numpy over candidates x variants x pairs, is_valid on the words of the steps.  Its steps must
                        equal the device's, field for field: the script fails otherwise.

    python profiles/bench_site_repair.py
    python profiles/bench_site_repair.py --family 10000 --repeats 3      # the same targets as one family: a conserved set

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


def planes_of_words(words):
    """uint64[n, 2] words -> uint32[n, 4] slot masks (A, C, G, T)."""
    out = np.zeros((len(words), 4), np.uint32)
    for k in range(32):
        nib = (words[:, k >> 4] >> np.uint64((15 - (k & 15)) * 4)) & np.uint64(0xF)
        for b in range(4):
            out[:, b] |= (((nib >> np.uint64(b)) & np.uint64(1)) << np.uint64(k)).astype(np.uint32)
    return out


def degeneracy(planes, start, stop):
    """planes uint32[..., 4] -> the product over the slots start..stop of the bases there."""
    d = np.ones(planes.shape[:-1], np.int64)
    for k in range(start, stop + 1):
        d = d * ((planes >> np.uint32(k)) & np.uint32(1)).sum(axis=-1).astype(np.int64)
    return d


def host_greedy(api, var, smap, sites, oligo_words, rule):
    """The greedy of pcr_site_repair in numpy -> list of (oligo, step, variant, word planes, n_expansions, candidates,
    sequences_held, sites_held, variants_held, sequences_total, gain, flags)."""
    max_degeneracy, max_mismatch, clamp3, max_candidates, max_steps = rule
    planes = planes_of_words(var["word"])
    site_seq = sites["sequence"].astype(np.int64)
    rows = []
    for o, word in enumerate(oligo_words):
        w = planes_of_words(np.array([word], np.uint64))[0]
        occ = int(w[0] | w[1] | w[2] | w[3])
        start, stop = (occ & -occ).bit_length() - 1, occ.bit_length() - 1
        mask = np.uint32(occ)
        clamp = np.uint32(sum(1 << k for k in range(max(stop - clamp3 + 1, 0), stop + 1)) & occ) if clamp3 else np.uint32(0)
        never = clamp3 > stop - start + 1
        first = int(np.searchsorted(var["oligo"], o, "left"))
        last = int(np.searchsorted(var["oligo"], o, "right"))
        foot = planes[first:last] & mask
        n_sites = var["sites"][first:last].astype(np.int64)
        mine = (smap >= first) & (smap < last)
        pairs = np.unique(np.stack([site_seq[mine], smap[mine].astype(np.int64) - first], axis=1), axis=0)
        seq_id = np.unique(pairs[:, 0], return_inverse=True)[1].reshape(-1) if len(pairs) else np.zeros(0, np.int64)
        pair_var = pairs[:, 1] if len(pairs) else np.zeros(0, np.int64)
        total = int(seq_id.max()) + 1 if len(pairs) else 0
        single = (np.bitwise_count(foot).sum(axis=1) == bin(occ).count("1")) & ((foot[:, 0] | foot[:, 1] | foot[:, 2] | foot[:, 3]) == mask) \
            if len(foot) else np.zeros(0, bool)

        def held_by(ws):                                  # ws uint32[m, 4] -> bool[m, variants]
            miss = ~((foot[None, :, 0] & ws[:, None, 0]) | (foot[None, :, 1] & ws[:, None, 1]) | (foot[None, :, 2] & ws[:, None, 2])
                     | (foot[None, :, 3] & ws[:, None, 3])) & mask
            return (np.bitwise_count(miss) <= max_mismatch) & ((miss & clamp) == 0) & (not never)

        def sequences_of(hv):                             # bool[m, variants] -> bool[m, total]
            out = np.zeros((hv.shape[0], total), bool)
            for m in range(hv.shape[0]):
                out[m, seq_id[hv[m, pair_var]]] = True
            return out

        hv = held_by(w[None, :])
        hs = sequences_of(hv)[0]
        hv = hv[0]
        step = 0
        rows.append([o, 0, api.REPAIR_NO_VARIANT, w.copy(), int(degeneracy(w, start, stop)), 0, int(hs.sum()), int(n_sites[hv].sum()),
                     int(hv.sum()), total, 0, 0])
        while True:
            if int(hs.sum()) == total:
                rows[-1][-1] = api.REPAIR_COMPLETE
                break
            if step == max_steps:
                rows[-1][-1] = api.REPAIR_STEPS
                break
            open_ = np.nonzero(single & ~hv)[0]
            unions = foot[open_] | w[None, :]
            n_exp = degeneracy(unions, start, stop)
            keep = n_exp <= max_degeneracy
            cand, unions, n_exp = open_[keep][:max_candidates], unions[keep][:max_candidates], n_exp[keep][:max_candidates]
            if len(cand) == 0:
                rows[-1][-1] = api.REPAIR_DEGENERACY if len(open_) else api.REPAIR_NO_GAIN
                break
            hv2 = held_by(unions)
            gain = (sequences_of(hv2) & ~hs[None, :]).sum(axis=1)
            held_sites = (hv2 * n_sites[None, :]).sum(axis=1)
            best = np.lexsort((cand, n_exp, -held_sites, -gain))[0]
            if gain[best] == 0:
                rows[-1][-1] = api.REPAIR_NO_GAIN
                break
            step += 1
            w, hv = unions[best], hv2[best]
            hs = sequences_of(hv[None, :])[0]
            rows.append([o, step, first + int(cand[best]), w.copy(), int(n_exp[best]), len(cand), int(hs.sum()), int(held_sites[best]),
                         int(hv.sum()), total, int(gain[best]), 0])
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--family", type=int, default=50, help="sequences per family; 10000 makes the C2 targets one family: a conserved set")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--max-degeneracy", type=int, default=16)
    ap.add_argument("--max-candidates", type=int, default=256)
    ap.add_argument("--max-steps", type=int, default=12)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_site_repair: no GPU")
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale, family=a.family)
    panel = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(panel), thr2, 18)
    rule = (a.max_degeneracy, 0, 0, a.max_candidates, a.max_steps)
    kw = dict(max_degeneracy=rule[0], max_mismatch=rule[1], clamp3=rule[2], max_candidates=rule[3], max_steps=rule[4])

    ids, steps = d.site_repair(panel, a.threshold, **kw)
    _, var, smap = d.site_variants(panel, a.threshold, thermo=False, site_map=True)
    cap, vcap = len(steps), max(len(var), 1)
    oligo_words = {}
    for i, (f, r) in enumerate(panel):
        oligo_words[int(ids[2 * i])], oligo_words[int(ids[2 * i + 1])] = (int(f[0]), int(f[1])), (int(r[0]), int(r[1]))
    oligo_words = [oligo_words[o] for o in range(len(oligo_words))]
    host = [None]

    def host_route():
        _, v, m = d.site_variants(panel, a.threshold, thermo=False, site_map=True, cap=vcap)
        _, s = d.site_tm(panel, a.threshold, cap=len(m))
        rows = host_greedy(api, v, m, s, oligo_words, rule)
        words = []
        for r in rows:
            sl = [int(sum(((int(r[3][b]) >> k) & 1) << b for b in range(4))) for k in range(32)]
            words.append(W.word_from_slots(sl))
        host[0] = (rows, words, d.is_valid(words, True, flags=True))

    legs = [("site_repair", lambda: d.site_repair(panel, a.threshold, cap=cap, **kw)),
            ("site_repair_cold", lambda: d.site_repair(panel, a.threshold, thermo=False, cap=cap, **kw)),
            ("site_variants_cold", lambda: d.site_variants(panel, a.threshold, thermo=False, cap=vcap)),
            ("host_route", host_route)]
    ts = {name: [] for name, _ in legs}
    for k in range(a.warmup + a.repeats):
        for name, call in legs:
            t0 = time.perf_counter()
            call()
            if k >= a.warmup:
                ts[name].append((time.perf_counter() - t0) * 1e3)
    # the check that comes for free: the host route's steps are the device's
    rows, words, valid = host[0]
    assert len(rows) == len(steps), (len(rows), len(steps))
    for r, wd, ok, s in zip(rows, words, valid, steps):
        got = (int(s["oligo"]), int(s["step"]), int(s["variant"]), (int(s["word"][0]), int(s["word"][1])), int(s["n_expansions"]),
               int(s["candidates"]), int(s["sequences_held"]), int(s["sites_held"]), int(s["variants_held"]), int(s["sequences_total"]),
               int(s["gain"]), int(s["flags"]), int(s["valid"]))
        want = (r[0], r[1], r[2], wd, r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], int(ok))
        assert got == want, (got, want)
    last = steps[steps["flags"] != 0]
    common = dict(config=a.config, scale=a.scale, family=a.family, targets=int(wl["T"]), pairs=len(panel), threshold=a.threshold,
                  entries=int(n_entries), sites=int(len(smap)), variants=int(len(var)), records=int(len(steps)),
                  steps_taken=int(len(steps) - len(last)), sequences_won=int(steps["gain"].sum()),
                  complete=int((last["flags"] == api.REPAIR_COMPLETE).sum()), rounds=a.repeats, host_equals_device=True)
    for name, _ in legs:
        print(json.dumps(dict(call=name, median_ms=round(statistics.median(ts[name]), 3), min_ms=round(min(ts[name]), 3),
                              max_ms=round(max(ts[name]), 3), **common)), flush=True)
    d.close()


if __name__ == "__main__":
    main()
