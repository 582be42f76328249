"""Times pcr_pool_amplicons beside the host path it replaces (stand-alone; bench.py is untouched).

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %), its pool's products from
Screener.pool_products after select_sites(pool, float32(0.9)**2): every product of every two oligos of the panel at 0.81
(--tile N repeats the records N times: a larger input with the same classes).  Every line is the median of --repeats host-clock
timings of the synchronous call on warm buffers, with the minimum and maximum.

  amplicons_info   pcr_pool_amplicons with info alone: length, gc, other and the classes of every record.
  amplicons_texts  the same call with the class tables and the packed unique amplicons too, buffers sized beforehand.
  host             what a caller without the call does: words.unpack_codes of each sequence's host copy, one slice per record
                   (reverse-complemented where smaller, with --canonical), np.unique over the slices' bytes.

The script fails unless the device's classes are the host's: the same partition of the records, the same set of unique
spellings.

    python profiles/bench_pool_amplicons.py
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_pool_amplicons.py --only amplicons_info   # the share of each kernel

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


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def intervals(api, rec, region):
    if region == api.REGION_PRODUCT:
        return rec["begin"].astype(np.int64), rec["end"].astype(np.int64) - rec["begin"] + 1
    if region == api.REGION_INSERT:
        return rec["inner_start"].astype(np.int64) + 4, rec["inner_length"].astype(np.int64) - 12
    return rec["inner_start"].astype(np.int64), rec["inner_length"].astype(np.int64)


def host_classes(api, W, wl, rec, region, canonical):
    """-> (class of every record, numbered in np.unique's order; the unique spellings as bytes, one code per byte)."""
    start, length = intervals(api, rec, region)
    width = int(length.max()) if len(rec) else 0
    rows = np.zeros((len(rec), width + 4), np.uint8)                          # the codes, zero-padded, then the length
    rows[:, width:] = length.astype("<u4").view(np.uint8).reshape(-1, 4)
    codes = {}
    nb = (np.asarray(wl["lengths"], np.int64) + 1) // 2
    for k in range(len(rec)):
        s = int(rec["sequence"][k])
        if s not in codes:
            o = int(wl["byte_offsets"][s])
            codes[s] = W.unpack_codes(wl["packed"][o:o + int(nb[s])], int(wl["lengths"][s]))
        f = codes[s][start[k]:start[k] + length[k]]
        if canonical:
            rc = W.revcomp_codes(f)
            if rc.tobytes() < f.tobytes():
                f = rc
        rows[k, :length[k]] = f
    uniq, inverse = np.unique(rows, axis=0, return_inverse=True)
    return inverse.reshape(-1), {u[:int(u[width:].view("<u4")[0])].tobytes() for u in uniq}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--tile", type=int, default=1, help="the products repeated this many times: more records, the same classes")
    ap.add_argument("--threshold", type=float, default=0.9)
    ap.add_argument("--region", type=int, default=0, choices=[0, 1, 2])
    ap.add_argument("--canonical", action="store_true")
    ap.add_argument("--only", choices=["amplicons_info", "amplicons_texts", "host"], default=None)
    a = ap.parse_args()

    import ctypes as C
    from pcramp_amd import api, synth
    W = api.W
    wl = synth.workload(a.config, 0, a.scale)
    pool = wl["pairs"]
    thr2 = float(np.float32(a.threshold) * np.float32(a.threshold))
    d = api.Screener(0)
    d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
    n_entries = d.select_sites(W.pairs_array(list(pool)), thr2, 18)
    _, prod = d.pool_products(pool, a.threshold, 80, 200, select=False, cap=1 << 20)
    if not len(prod):
        raise SystemExit("the pool forms no product: nothing is compared")
    prod = np.tile(prod, a.tile)
    info, texts = d.product_amplicons(prod, a.region, canonical=a.canonical, sequences=True)
    n_classes = len(texts)
    common = dict(config=a.config, scale=a.scale, tile=a.tile, targets=int(wl["T"]), pairs=len(pool), threshold=a.threshold, region=a.region,
                  canonical=bool(a.canonical), entries=int(n_entries), products=int(len(prod)), classes=n_classes,
                  bases=int(info["length"].sum()), launches=a.repeats + a.warmup + 1)
    line = lambda call, ts, **kw: print(json.dumps(dict(call=call, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                                                        max_ms=round(max(ts), 4), **kw, **common)), flush=True)
    # the same classes: the two labelings pair off one to one, and the unique spellings are the same set
    host_id, host_unique = host_classes(api, W, wl, prod, a.region, a.canonical)
    pairs = np.unique(np.stack([info["amplicon"].astype(np.int64), host_id.astype(np.int64)], 1), axis=0)
    if len(pairs) != n_classes or len(np.unique(pairs[:, 0])) != n_classes or len(np.unique(pairs[:, 1])) != n_classes:
        raise SystemExit("the device's classes are not the host's")
    if {W.codes_from_text(t).tobytes() for t in texts} != host_unique:
        raise SystemExit("the device's unique amplicons are not the host's")

    rec = np.ascontiguousarray(prod, api.PRODUCT_DTYPE)
    out = np.zeros(len(rec), api.AMPLICON_INFO_DTYPE)

    def info_only():
        n = d.L.pcr_pool_amplicons(d.h, api.TARGET, rec.ctypes.data, len(rec), a.region, int(a.canonical), out.ctypes.data, None, None, 0,
                                   None, 0, None)
        if n != n_classes:
            raise SystemExit("the info-only call returned %d, not %d" % (n, n_classes))

    off, ln = np.zeros(n_classes, np.uint64), np.zeros(n_classes, np.uint64)
    need = C.c_uint64(0)
    d.L.pcr_pool_amplicons(d.h, api.TARGET, rec.ctypes.data, len(rec), a.region, int(a.canonical), None, None, None, 0, None, 0, C.byref(need))
    packed = np.zeros(max(int(need.value), 1), np.uint8)

    def with_texts():
        n = d.L.pcr_pool_amplicons(d.h, api.TARGET, rec.ctypes.data, len(rec), a.region, int(a.canonical), out.ctypes.data,
                                   off.ctypes.data, ln.ctypes.data, n_classes, packed.ctypes.data, packed.size, None)
        if n != n_classes:
            raise SystemExit("the full call returned %d, not %d" % (n, n_classes))

    if a.only in (None, "amplicons_info"):
        ts = measure(info_only, a.repeats, a.warmup)
        if out.tobytes() != info.tobytes():
            raise SystemExit("the info-only call's info differs from Screener.product_amplicons'")
        out[:] = 0
        line("amplicons_info", ts)
    if a.only in (None, "amplicons_texts"):
        ts = measure(with_texts, a.repeats, a.warmup)
        if out.tobytes() != info.tobytes():
            raise SystemExit("the full call's info differs from Screener.product_amplicons'")
        line("amplicons_texts", ts, packed_bytes=int(need.value))
    if a.only in (None, "host"):
        line("host", measure(lambda: host_classes(api, W, wl, prod, a.region, a.canonical), a.host_repeats, 0))
    d.close()


if __name__ == "__main__":
    main()
