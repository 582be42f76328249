"""Times pcr_select_sites beside the bit-sliced pcr_select_words (stand-alone; bench.py is untouched).

Input: the C2 workload of pcramp_amd.synth (10 000 targets x 10 kb in families of 50 at 3 %, 50 pairs).  Every line is the
median of --repeats host-clock timings of the synchronous call on warm buffers (the calls before them grow the buckets and
allocate), with the minimum and maximum, and -- from a second run of the same calls with the scan bracketed by events
(pcr_profile_read) -- the scan kernels' time per call.

    python profiles/bench_select_sites.py      # select_sites at 0.81 and 0.9, bit-sliced select_words at 0.9

Copied into a checkout that has no pcr_select_sites yet (the commit before it), it reports the select_words line only: the
baseline the call is compared with.  Prints one JSON object per line.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()

    from pcramp_amd import api, synth
    wl = synth.workload(a.config, 0, a.scale)
    pairs = api.W.pairs_array(wl["pairs"])
    have_sites = hasattr(api.Screener, "select_sites")

    def screener(scan=None):
        old = os.environ.get("PCRAMP_SCAN")
        if scan is not None:
            os.environ["PCRAMP_SCAN"] = str(scan)
        try:
            d = api.Screener(0)
        finally:
            if scan is not None:
                if old is None:
                    os.environ.pop("PCRAMP_SCAN", None)
                else:
                    os.environ["PCRAMP_SCAN"] = old
        d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"], np.ones(wl["T"], np.float32))
        return d

    lines = []
    if have_sites:
        lines += [("select_sites", 0.81, None), ("select_sites", 0.9, None)]
    lines.append(("select_words", 0.9, 2))
    for name, thr, scan in lines:
        d = screener(scan)
        if name == "select_sites":
            call = lambda: d.select_sites(pairs, thr, 18, count=False)
        else:
            call = lambda: d.select_words(pairs, thr, 18, count=False)
        ts = measure(call, a.repeats, a.warmup)
        d.profile(True)
        d.profile_read(True)
        for _ in range(a.repeats):
            call()
        scan_ms, launches = d.profile_read(True)
        d.profile(False)
        n = d.L.pcr_get_entries(d.h, api.TARGET, None, 0)
        print(json.dumps(dict(call=name, threshold=thr, scan="bit-sliced" if (scan == 2 or name == "select_sites") else "default",
                              config=a.config, scale=a.scale, targets=int(wl["T"]), pairs=int(pairs.shape[0]), entries=int(n),
                              median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                              scan_kernels_ms_per_call=round(scan_ms / max(launches, 1), 4), scan_brackets=int(launches))), flush=True)
        d.close()


if __name__ == "__main__":
    main()
