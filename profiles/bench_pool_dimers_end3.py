"""Times pcr_pool_dimers_end3 beside pcr_pool_dimers on the same pool in the same run (stand-alone; bench.py is untouched).

Pools: the 50-pair panel of the C2 workload of pcramp_amd.synth (100 oligos, 10 000 cells) and tests/pool_dimer_cases.full_pool
(1 024 pairs of distinct plain oligos, 2 048 oligos, 4.2 * 10^6 cells).  Settings: min_run = 4, min_extension = 1, rule POOL,
every placement kept.  Every line is the median of --repeats host-clock timings of the synchronous call on warm buffers
with the arrays sized beforehand, with the minimum and maximum.

  end3_cells       Screener.pool_dimers_end3(pool, cap=(cells, 0)): cell records only.
  end3_placements  ... placements=True: cell and placement records.
  end3_count       the count call (cap 0, every placement kept): the scan alone, nothing is melted.
  pool_dimers      Screener.pool_dimers(pool, rule="pool", cap=cells): the whole-oligo duplexes of the same cells.

`jobs` are the placements melted, `jobs_per_duplex` their ratio to the duplexes pool_dimers melts.

    python profiles/bench_pool_dimers_end3.py
    rocprofv3 --kernel-trace --stats ... -- python profiles/bench_pool_dimers_end3.py   # k_dimer_end3_scan / _melt / _merge beside k_pool_dimer

Prints one JSON object per line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


class _Words:
    """What pool_dimer_cases' pools ask of the oracle: the centred word of a text."""

    @staticmethod
    def centered_word(text):
        from pcramp_amd import words as W
        return W.centered_word(W.codes_from_text(text))


def count_call(api, d, pool, min_run, min_extension):
    """The C call with cap 0 and place_cap 0 (the wrapper would go on to fetch the records) -> (cells, placements)."""
    import ctypes as C
    import numpy as np
    arr = api.W.pairs_array(pool)
    ids = np.zeros(max(2 * len(pool), 1), np.uint32)
    args = api.ThermoArgs(0.05, 9e-7, 0.0, 0.0, 0.0, 0.0)
    n_place = C.c_uint64(0)
    n = d.L.pcr_pool_dimers_end3(d.h, arr.ctypes.data, len(pool), C.byref(args), api.DIMER_RULE_POOL, min_run, min_extension,
                                 float("inf"), ids.ctypes.data, None, 0, None, 0, C.byref(n_place))
    assert n >= 0
    return int(n), int(n_place.value)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-run", type=int, default=4)
    ap.add_argument("--min-extension", type=int, default=1)
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()

    from pcramp_amd import api, synth
    import pool_dimer_cases as PC
    wl = synth.workload(a.config, 0, a.scale)
    pools = [("panel", wl["pairs"])]
    if not a.skip_full:
        pools.append(("full", PC.full_pool(_Words())))
    d = api.Screener(0)                                                     # no sequences, no word DB: the calls need neither
    kw = dict(min_run=a.min_run, min_extension=a.min_extension, rule="pool")
    for name, pool in pools:
        ids, rec, pl = d.pool_dimers_end3(pool, placements=True, **kw)
        n = int(ids.max()) + 1
        _, dim = d.pool_dimers(pool, rule="pool")
        duplexes = int(dim["n_duplexes"].sum())
        assert int(rec["n_placements"].sum()) == len(pl) and len(dim) == n * n
        common = dict(pool=name, pairs=len(pool), oligos=n, cells=n * n, duplexes=duplexes, jobs=int(len(pl)),
                      jobs_per_duplex=round(len(pl) / duplexes, 4), cell_records=int(len(rec)),
                      mutual=int((pl["flags"] & api.DIMER_END3_MUTUAL != 0).sum()), min_run=a.min_run, min_extension=a.min_extension)
        calls = (("end3_cells", lambda: d.pool_dimers_end3(pool, cap=(len(rec), 0), **kw)),
                 ("end3_placements", lambda: d.pool_dimers_end3(pool, placements=True, cap=(len(rec), len(pl)), **kw)),
                 ("end3_count", lambda: count_call(api, d, pool, a.min_run, a.min_extension)),
                 ("pool_dimers", lambda: d.pool_dimers(pool, rule="pool", cap=n * n)))
        for call, fn in calls:
            ts = measure(fn, a.repeats, a.warmup)
            print(json.dumps(dict(call=call, median_ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4),
                                  max_ms=round(max(ts), 4), **common)), flush=True)
    d.close()


if __name__ == "__main__":
    main()
