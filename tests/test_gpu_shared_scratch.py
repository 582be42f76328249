"""The scratch set that pcr_pool_products_tm, pcr_pool_probe_hits, pcr_pool_anneal_profile and pcr_pool_conflicts share on a
handle: a sequence of calls on ONE handle -- larger and smaller pools in turn, early returns between full calls -- answers each
call with the bytes a fresh handle gives for it.  Nothing is compared with a model here (the entry points' own tests do that):
a stale tail or a buffer another call still needed shows as a difference between the two handles.  (No call here sets the
error flag, so a stale flag is not something this comparison can see.)"""
import numpy as np
import pytest

import products_tm_cases as PC
import site_repair_cases as RC
import site_tm_cases as SC
from pcramp_amd import api

pytestmark = pytest.mark.gpu

TEMPS = np.array([0.0, 40.0, 50.0, 55.0, 60.0, 70.0], np.float32)


def _handle(case):
    d = api.Screener(0)
    d.load_texts(case["seqs"])
    d.select_sites(case["panel"], SC.SQ(case["thr"]))
    return d


def _bytes(out):
    return [np.ascontiguousarray(x).tobytes() for x in out]


def test_one_handle_answers_like_fresh_ones(oracle):
    case = PC.scenario(oracle, "random")                                     # 8 sequences x 2 kb, 6 pairs (two with IUPAC bases)
    lo, hi = PC.amp_of(case)
    thr, big, small = case["thr"], case["panel"], case["panel"][:2]
    probes = [big[(i + 1) % len(big)][0] for i in range(len(small))]         # oligos with sites in the DB: the next pair's F
    kw = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, amp_min=lo, amp_max=hi)
    melt = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
    # (what it is, the call, the least number of records it has to give to mean anything)
    calls = [
        ("products_tm, the whole pool", lambda d: d.pool_products_tm(big, thr, bits=True, **kw), 1),
        ("anneal_profile, a smaller pool", lambda d: d.anneal_profile(small, TEMPS, thr, melt=True, **kw), 1),
        ("probe_hits", lambda d: d.probe_hits(small, probes, thr, bits=True, **kw), 1),
        ("products_tm, an empty pool", lambda d: d.pool_products_tm([], thr, bits=True, **kw), 0),
        ("pool_conflicts, the whole pool", lambda d: d.pool_conflicts(big, thr, dimers="pool", **kw), 1),
        ("products_tm, a cap below the count, then the full call", lambda d: d.pool_products_tm(small, thr, bits=True, cap=1, **kw), 2),
        ("site_tm, a cap below the count, then the full call", lambda d: d.site_tm(big, thr, cap=1, **melt), 2),
        ("site_repair", lambda d: d.site_repair(small, thr, **RC.THERMO), 1),
        ("products_tm, the whole pool at a floor", lambda d: d.pool_products_tm(big, thr, tm_floor=45.0, bits=True, **kw), 1),
    ]
    one = _handle(case)
    try:
        got = [_bytes(call(one)) for _, call, _ in calls]
        n_items = {}
        for (what, call, least), mine in zip(calls, got):
            fresh = _handle(case)
            try:
                out = call(fresh)
            finally:
                fresh.close()
            n_items[what] = len(out[2] if what == "probe_hits" else out[1])
            assert n_items[what] >= least, what
            assert mine == _bytes(out), what
        # the whole pool has more items, jobs and products than its first two pairs (the same floor, 0): the sequence shrinks
        # its use of the shared buffers after a larger one (calls 2, 3 and 6) and grows it after a smaller one (calls 5 and 9)
        assert n_items["products_tm, the whole pool"] > n_items["products_tm, a cap below the count, then the full call"]
    finally:
        one.close()
