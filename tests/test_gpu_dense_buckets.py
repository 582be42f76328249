"""The word DB and every kernel that reads it at each size of the per-sequence hit buckets, on the dense scenarios of
tests/dense_buckets.py: the sequence with the long bucket holds labelled amplicons at the start, in the middle (across
~1 200 low-complexity entries) and at the end of its bucket, decoy amplicons inside and one base outside the window, and
amplicons cut by an EOS.  Everything is compared exactly with the oracle session and, where the planted geometry gives
one, with the label.  Every test asserts the bucket size it ran at (the library's "pass done" / "scan plan" debug
lines), so that a change of the growth rule cannot move it silently into another class:

    class   bucket slots   finalisation          move_coverage        optimize
    4k      4 096          k_finalize<1>         k_pair_moves_seq     k_pair_moves_lds<true>  (s4k)
    8k      8 192          k_finalize<1>, 64 KB  k_pair_moves         k_pair_moves_batch      (s8k)
    32k     32 768         k_finalize_big        k_pair_moves
    64k     65 536         k_finalize_big        k_pair_moves
    (s4k / s8k: the classes selected with optimize_5 = optimize_3 = 1, three words per site, as the local search needs)

find_background_match runs at every class, but without the low-complexity pair: the oracle aligns every candidate
amplicon of a pair on the CPU, and that pair alone forms ~10^5 of them in the poly-A stretch.  The capacity edges are the
library's own refusals (PCR_ERR_CAPACITY with the documented message), each followed by a pass on the same handle."""
import re

import numpy as np
import pytest

import amplicon_edges as AE
import dense_buckets as DB
from pcramp_amd import api, words as W
from testdata import move_variants, rand_seq

pytestmark = pytest.mark.gpu

PCR_ERR_CAPACITY = -4
CASES = [("4k", False), ("8k", False), ("8k", True), ("32k", False), ("32k", True), ("64k", False), ("64k", True)]
_id = lambda c: c[0] + ("-two" if c[1] else "")


def _session(oracle, sc, pairs=None, **opts):
    so = oracle.session(**dict(sc.opts, **opts))
    for s, w in zip(sc.seqs, sc.weights):
        so.add_target(s, w)
    for i in sc.inactive:
        so.set_active(i, False)
    for i, pos in sc.splits:
        so.split(i, pos)
    so.select(sc.pairs if pairs is None else pairs)
    return so


_BUILT = {}


def _case(oracle, key):
    """(scenario, oracle session selected for it), built once per module run."""
    if key not in _BUILT:
        d = DB.build(oracle, *key)
        _BUILT[key] = (d, _session(oracle, d.sc))
    return _BUILT[key]


@pytest.fixture(params=CASES, ids=_id)
def case(request, oracle):
    return _case(oracle, request.param)


def _open(sc, monkeypatch, **env):
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = api.Screener(0)
    d.load_texts(sc.seqs, sc.weights)
    act = np.ones(len(sc.seqs), np.uint8)
    act[list(sc.inactive)] = 0
    d.set_active(act)
    for i, pos in sc.splits:
        d.split(i, pos)
    return d


def _thr(o):
    return float(np.float32(o["target_threshold"]) * np.float32(o["search_multiplier"]))


def _select(d, sc, shift=0):
    return d.select_words(sc.pairs, _thr(sc.opts), sc.opts["min_primer"], shift, shift)


def _passes(capfd):
    """(slots, largest fill) of every synchronous pass since the last read, and the slots of every scan plan."""
    err = capfd.readouterr().err
    done = [(int(a), int(b)) for a, b in re.findall(r"pass done: (\d+)-slot buckets, largest fill (\d+)", err)]
    plans = [int(x) for x in re.findall(r"scan plan: .*, (\d+)-slot buckets", err)]
    return done, plans


def _ran_at(capfd, cap):
    done, _ = _passes(capfd)
    print("pass done (slots, largest fill):", done)
    assert done and done[-1][0] == cap and cap // 2 < done[-1][1] <= cap, (done, cap)


def _check_bits(d_sc, so, fr, rf):
    """Device bits == the oracle's == the labels', per pair and orientation, under the window of d_sc."""
    sc = d_sc
    so.set_options(amp_min=sc.opts["amp_min"], amp_max=sc.opts["amp_max"])
    want_fr, want_rf = AE.expected(sc)
    for p, pair in enumerate(sc.pairs):
        _, ori = so.target_match(pair, orient=True)
        assert np.array_equal(np.asarray(fr[p]), (ori & 1) != 0), (sc.name, p, "FR")
        assert np.array_equal(np.asarray(rf[p]), (ori & 2) != 0), (sc.name, p, "RF")
        assert np.array_equal(np.asarray(fr[p]), want_fr[p]) and np.array_equal(np.asarray(rf[p]), want_rf[p]), (sc.name, p)
    for l in sc.labels:
        assert bool((fr if l.orient == "FR" else rf)[l.pair][l.seq]) == l.admitted, (sc.name, l)


# ---------------------------------------------------------------------------------------------- select
@pytest.mark.parametrize("scan", [None, "2"])
def test_select(oracle, case, capfd, monkeypatch, scan):
    """The word DB: count and entries == oracle, sorted, no duplicates, exactly the planted sites in the dense sequences
    (no near-copy), on the default handle and with the bit-sliced scan alone (PCRAMP_SCAN=2), which ends one bucket size
    lower: 2 048, 4 096, 16 384 and 32 768 slots."""
    dn, so = case
    sc = dn.sc
    d = _open(sc, monkeypatch, **({"PCRAMP_SCAN": scan} if scan else {}))
    try:
        capfd.readouterr()
        n = _select(d, sc)
        # (the seed scan records every hit of these scenarios twice, the bit-sliced scan once: half the fill, half the slots)
        _ran_at(capfd, DB.CLASSES[dn.cls].cap // (2 if scan else 1))
        ent = d.entries()
        assert n == len(ent) and ent == so.db_entries()
        assert ent == sorted(set(ent))
        for i in dn.dense:
            b = DB.bucket(ent, i)
            assert [(e[2], e[4]) for e in b] == sorted((s.loc, 1 if s.role == "P" else 2) for s in sc.sites[i])
    finally:
        d.close()


@pytest.mark.parametrize("cls", ["s4k", "s8k"])
def test_select_every_shift(oracle, capfd, monkeypatch, cls):
    """optimize_5 = optimize_3 = 1: several candidate words per site and tens of tied hits per entry for the dedupe."""
    dn = DB.build(oracle, cls)
    sc = dn.sc
    so = _session(oracle, sc, optimize_5=1, optimize_3=1)
    d = _open(sc, monkeypatch)
    try:
        capfd.readouterr()
        n = _select(d, sc, 1)
        _ran_at(capfd, DB.CLASSES[cls].cap)
        ent = d.entries()
        assert n == len(ent) and ent == so.db_entries() and ent == sorted(set(ent))
        lo, hi = DB.CLASSES[cls].entries
        assert lo <= AE.largest_bucket(ent) <= hi
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- k_pair
def test_pairing(oracle, case, capfd, monkeypatch):
    """amplify / find_target_match / compute_coverage under the scenario's window and the wide one: the positive across the
    low-complexity stretch (wide only), the positives at both ends of the bucket, the pair whose only candidates lie one
    base outside the window, the EOS and split negatives."""
    dn, so = case
    d = _open(dn.sc, monkeypatch)
    try:
        capfd.readouterr()
        _select(d, dn.sc)
        _ran_at(capfd, DB.CLASSES[dn.cls].cap)
        for sc in (dn.sc, DB.wide(dn.sc)):
            o = sc.opts
            bits, fr, rf, _ = d.amplify(sc.pairs, o["target_threshold"], o["target_threshold"], o["amp_min"], o["amp_max"], 0)
            _check_bits(sc, so, fr, rf)
            assert np.array_equal(d.find_target_match(sc.pairs, o["target_threshold"], o["amp_min"], o["amp_max"], 0), bits)
            cov = d.compute_coverage(sc.pairs, o["target_threshold"], o["search_multiplier"], o["amp_min"], o["amp_max"], 0)
            for p, pair in enumerate(sc.pairs):
                assert cov[p] == np.float32(so.target_coverage(pair)), (sc.name, p)
            for i in dn.dense:
                assert fr[0][i] and rf[2][i] and fr[dn.k["d"]][i] and rf[dn.k["d"]][i]
                assert not fr[dn.k["cut"]][i] and not rf[dn.k["cut"]][i]
                assert bool(fr[1][i]) == (o["amp_max"] == 2000)
                if o["amp_max"] == 200:
                    assert not fr[dn.k["out"]][i] and not rf[dn.k["out"]][i]
    finally:
        so.set_options(**DB.NARROW)
        d.close()


# ---------------------------------------------------------------------------------------------- the asynchronous pass
def _screen(d, sc, torch):
    o = sc.opts
    words = int(d.bitset_words())
    out = torch.full((2, len(sc.pairs), words), -1, dtype=torch.int64, device="cuda:0")
    d.screen_device(sc.pairs, _thr(o), out[0].data_ptr(), out[1].data_ptr(), o["target_threshold"], o["target_threshold"],
                    o["amp_min"], o["amp_max"], False, o["min_primer"])
    d.synchronize()
    torch.cuda.synchronize()
    a = out.cpu().numpy().view(np.uint64)
    return ([api.bits_to_bool(a[0, p], len(sc.seqs)) for p in range(len(sc.pairs))],
            [api.bits_to_bool(a[1, p], len(sc.seqs)) for p in range(len(sc.pairs))])


def test_screen_device_cycle(oracle, case, capfd, monkeypatch):
    """screen_device three times on a freshly loaded set (the first overflows the 64-slot buckets and is replayed by
    synchronize(), the others start at the grown size); a sparse batch on the same handle, which shrinks the buckets; the
    dense batch again: grow, shrink, grow, as a design run does."""
    import torch
    dn, so = case
    sc = dn.sc
    cap = DB.CLASSES[dn.cls].cap
    sparse = [sc.pairs[dn.k["sparse"]]]
    ss = _session(oracle, sc, pairs=sparse)
    d = _open(sc, monkeypatch)
    try:
        capfd.readouterr()
        for rep in range(3):
            fr, rf = _screen(d, sc, torch)
            _check_bits(sc, so, fr, rf)
            assert d.entries() == so.db_entries(), rep
        _, plans = _passes(capfd)
        assert plans[0] == 64 and max(plans) == cap and plans[-1] == cap, plans
        n = d.select_words(sparse, _thr(sc.opts), sc.opts["min_primer"])
        assert n == len(ss.db_entries()) and d.entries() == ss.db_entries() and 0 < n <= 8
        _, fr, rf, _ = d.amplify(sparse, 1.0, 1.0, 80, 200, 0)
        _, ori = ss.target_match(sparse[0], orient=True)
        assert np.array_equal(fr[0], (ori & 1) != 0) and np.array_equal(rf[0], (ori & 2) != 0) and ori.any()
        done, plans = _passes(capfd)
        assert plans == [cap] and done[-1][0] == 64, (plans, done)            # planned at the grown size, repeated at 64 slots
        fr, rf = _screen(d, sc, torch)
        _check_bits(sc, so, fr, rf)
        assert d.entries() == so.db_entries()
        _, plans = _passes(capfd)
        assert plans[0] == 64 and plans[-1] == cap, plans
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- the move kernels
def _variants(pair, side):
    out = []
    for kind in ("trim5", "trim3", "grow5", "grow3", "inc"):
        out += move_variants(W, pair[side], kind)[:3]
    return out


def test_move_coverage(oracle, case, capfd, monkeypatch):
    """move_coverage of the labelled pairs and the decoy pair, both sides, variants that change the edited oligo's length:
    k_pair_moves_seq up to 4 096 slots, k_pair_moves with a thread per slot beyond."""
    dn, so = case
    d = _open(dn.sc, monkeypatch)
    try:
        capfd.readouterr()
        _select(d, dn.sc)
        _ran_at(capfd, DB.CLASSES[dn.cls].cap)
        n_hit = 0
        for sc in (dn.sc, DB.wide(dn.sc)):
            o = sc.opts
            so.set_options(amp_min=o["amp_min"], amp_max=o["amp_max"])
            for p in (0, 1, 2, dn.k["d"]):
                pair = sc.pairs[p]
                for side in (0, 1):
                    var = [pair[side]] + _variants(pair, side)
                    cov, fr, rf = d.move_coverage(pair, side, var, o["target_threshold"], o["search_multiplier"], o["amp_min"],
                                                  o["amp_max"], False)
                    ocov, ori = so.move_coverage(pair, side, var, orient=True)
                    assert np.array_equal(cov, ocov), (sc.name, p, side)
                    assert np.array_equal(fr, (ori & 1) != 0) and np.array_equal(rf, (ori & 2) != 0), (sc.name, p, side)
                    for i in dn.dense:                         # the unmodified oligo: the dense sequence answers as labelled
                        want = {0: (1, 0), 1: (int(o["amp_max"] == 2000), 0), 2: (0, 1), dn.k["d"]: (1, 1)}[p]
                        assert (int(fr[0][i]), int(rf[0][i])) == want, (sc.name, p, side)
                    n_hit += int(np.count_nonzero(ori[:, dn.dense]))
        assert n_hit > 20
    finally:
        so.set_options(**DB.NARROW)
        d.close()


@pytest.mark.parametrize("cls,env", [("s4k", {}), ("s8k", {}), ("s4k", {"PCRAMP_OPT_PM": "g"})], ids=["s4k", "s8k", "s4k-global"])
def test_optimize(oracle, capfd, monkeypatch, cls, env):
    """The local search over assays of the labelled and decoy pairs == the oracle's loop: k_pair_moves_lds<true> at 4 096
    slots, k_pair_moves_batch at 8 192, and k_pair_moves_batch forced at 4 096 (PCRAMP_OPT_PM=g)."""
    from oracle_lib import optimize as oracle_optimize
    from pcramp_amd import moves
    dn = DB.build(oracle, cls)
    sc = dn.sc
    to = _session(oracle, sc, optimize_5=1, optimize_3=1)
    kw = dict(degen=4, tm_min=30.0, tm_max=90.0, max_hairpin=90.0)
    d = _open(sc, monkeypatch, **env)
    try:
        capfd.readouterr()
        _select(d, sc, 1)
        _ran_at(capfd, DB.CLASSES[cls].cap)
        base = [sc.pairs[0], sc.pairs[2], sc.pairs[dn.k["d"]], (sc.pairs[0][0], sc.pairs[dn.k["d"]][1])]
        want = [oracle_optimize(oracle, to, None, p, **kw) for p in base]
        for p, (po, so_) in zip(base, want):
            pd, sd = moves.optimize(d, p, have_background=False, **kw)
            assert pd == po and tuple(float(x) for x in sd) == so_, p
        print("assays changed by the search:", sum(po != p for p, (po, _) in zip(base, want)))
        bp, bs, _ = moves.optimize_batch(d, base, have_background=False, **kw)
        for k, (po, so_) in enumerate(want):
            assert bp[k] == po and tuple(float(x) for x in bs[k]) == so_, k
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- amplicon records
def test_collect_amplicons(oracle, case, monkeypatch, capfd):
    """k_collect_amplicons for the decoy pair and the labelled pairs: the (sequence, begin, end) multiset == oracle, its
    set == the labels; pair 1 under the wide window (its amplicon spans the low-complexity stretch)."""
    dn, so = case
    d = _open(dn.sc, monkeypatch)
    try:
        capfd.readouterr()
        _select(d, dn.sc)
        _ran_at(capfd, DB.CLASSES[dn.cls].cap)
        for sc, which in ((dn.sc, (0, 2, dn.k["d"], dn.k["out"], dn.k["cut"])), (DB.wide(dn.sc), (1, 0))):
            o = sc.opts
            for p in which:
                bo, _ = so.collect_amplicons(sc.pairs[p], o["target_threshold"], o["amp_min"], o["amp_max"])
                rec = d.collect_amplicons(sc.pairs[p], o["target_threshold"], o["amp_min"], o["amp_max"])
                got = sorted((r["sequence"], r["begin"] & 0xFFFFFFFF, r["end"]) for r in rec)
                assert got == sorted(bo), (sc.name, p)
                assert sorted(set(got)) == AE.expected_bounds(sc, p), (sc.name, p)
                if p in (0, 1, 2, dn.k["d"]):
                    assert all(any(g[0] == i for g in got) for i in dn.dense), (sc.name, p)
    finally:
        d.close()


def test_pool_products(oracle, case, monkeypatch, capfd):
    """pool_products for the decoy pair and the labelled pairs: the records of every oligo combination == the oracle's
    collect_amplicons for that combination, as test_gpu_pool_products::test_amplicon_edges composes them."""
    import test_gpu_pool_products as PP
    dn, so = case
    sc = dn.sc
    o = sc.opts
    pool = [sc.pairs[p] for p in (dn.k["d"], 0, 1, 2)]
    d = _open(sc, monkeypatch)
    try:
        capfd.readouterr()
        _select(d, sc)
        _ran_at(capfd, DB.CLASSES[dn.cls].cap)
        for lo, hi in ((80, 200), (0, 2000)):
            ids, rec = d.pool_products(pool, o["target_threshold"], lo, hi, select=False)
            PP._check_order(ids, rec)
            PP._intended_ok(pool, ids, rec)
            words = PP._distinct(pool, ids)
            by = PP._by_combo(rec)
            assert len(words) == 8
            for a in range(len(words)):
                for b in range(a, len(words)):
                    PP._check_oracle(so, words, by, a, b, o["target_threshold"], lo, hi)
            for i in dn.dense:
                assert any(s == i for s, *_ in by[(int(ids[0]), int(ids[1]))])          # the decoy pair, FR, in the dense bucket
                assert any(s == i for s, *_ in by[(int(ids[7]), int(ids[6]))])          # pair 2, RF: the end of the bucket
                assert any(s == i for s, *_ in by.get((int(ids[4]), int(ids[5])), [])) == (hi == 2000)
    finally:
        d.close()


@pytest.mark.parametrize("key", [("4k", False), ("8k", False), ("32k", False), ("64k", False)], ids=_id)
def test_background_match(oracle, monkeypatch, capfd, key):
    """find_background_match with the set loaded as the background, the reference's index mode and evaluate_all, under the
    background window and the scenario's (k_bg_emit<0>); without the low-complexity pair (see the module docstring).
    Ended at 1 024, 2 048 or 4 096, 16 384 and 32 768 slots when it was written."""
    dn, _ = _case(oracle, key)
    sc = dn.sc
    pairs = [p for k, p in enumerate(sc.pairs) if k != dn.k["lc"]]
    so = oracle.session()
    for s in sc.seqs:
        so.add_target(s)
    bt = 0.5
    thr = float(np.float32(bt) * np.float32(0.9))
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    d = api.Screener(0)
    try:
        d.load_texts(sc.seqs, which=api.BACKGROUND)
        capfd.readouterr()
        assert d.select_words(pairs, thr, 16, which=api.BACKGROUND) == so.select(pairs, threshold=thr, min_len_override=16)
        done, _ = _passes(capfd)
        print("pass done (slots, largest fill):", done)
        ent = d.entries(which=api.BACKGROUND)
        assert ent == so.db_entries()
        # At this threshold the scan records many hits below the final maximum of their candidate before it has seen the
        # maximum, as many as the order of its workgroups brings about (2 013 and 2 053 in two runs of the 8k class): the
        # fill lies between the entries of the dense sequence and a few times as many, and every such size is beyond the
        # 128 slots up to which k_bg_emit keeps a bucket in LDS
        np2 = 1
        while np2 < AE.largest_bucket(ent):
            np2 *= 2
        assert max(np2, 1024) <= done[-1][0] <= 4 * np2, (done, AE.largest_bucket(ent))
        hits = 0
        for amp in ((0, 2000), (80, 200)):
            for ev in (False, True):
                bits = d.find_background_match(pairs, bt, 0.9, amp[0], amp[1], False, evaluate_all=ev)
                for p, pair in enumerate(pairs):
                    ob, _ = so.background_match(pair, bt, 0.9, amp[0], amp[1], 0, emulate_index_bug=int(not ev))
                    assert np.array_equal(bits[p], ob.astype(bool)), (sc.name, amp, ev, p)
                    hits += int(ob[dn.dense].sum())
        assert hits > 0
    finally:
        d.close()


# ---------------------------------------------------------------------------------------------- capacity edges
def _still_works(d, oracle, sc, sparse):
    ss = _session(oracle, sc, pairs=sparse)
    n = d.select_words(sparse, _thr(sc.opts), sc.opts["min_primer"])
    assert n == len(ss.db_entries()) and d.entries() == ss.db_entries() and n > 0


def test_more_sites_than_a_bucket_holds(oracle, monkeypatch):
    """A dense sequence whose hits need more than 65 536 slots: PCR_ERR_CAPACITY from select_words, and from
    screen_device + synchronize(); the handle serves the next pass."""
    import torch
    dn = DB.build(oracle, "64k", n_sites=30000)
    sc = dn.sc
    sparse = [sc.pairs[dn.k["sparse"]]]
    d = _open(sc, monkeypatch)
    try:
        with pytest.raises(api.PcrError, match="more than 65536 candidate sites") as e:
            _select(d, sc)
        assert e.value.rc == PCR_ERR_CAPACITY
        _still_works(d, oracle, sc, sparse)
        with pytest.raises(api.PcrError, match="more than 65536 candidate sites") as e:
            _screen(d, sc, torch)
        assert e.value.rc == PCR_ERR_CAPACITY
        _still_works(d, oracle, sc, sparse)
    finally:
        d.close()


def test_buckets_that_would_not_fit(oracle, monkeypatch):
    """n sequences x 65 536 slots x 48 B beyond the 96 GB the hit buckets may take: the 64k scenario among 32 800 short
    sequences.  (The guard is evaluated before the buckets are allocated; what was allocated by then -- the 64-slot
    buckets of the first attempt, 100 MB, and the per-sequence tables -- is small.)"""
    dn, _ = _case(oracle, ("64k", False))
    import random
    r = random.Random(5)
    extra = [rand_seq(r, 40) for _ in range(32800)]
    assert (len(dn.sc.seqs) + len(extra)) * 65536 * 48 > 96 << 30 and (len(dn.sc.seqs) + len(extra)) * 65536 < 1 << 32
    sc = dn.sc._replace(seqs=list(dn.sc.seqs) + extra, weights=list(dn.sc.weights) + [1.0] * len(extra))
    sparse = [sc.pairs[dn.k["sparse"]]]
    d = _open(sc, monkeypatch)
    try:
        with pytest.raises(api.PcrError, match="would not fit") as e:
            _select(d, sc)
        assert e.value.rc == PCR_ERR_CAPACITY
        _still_works(d, oracle, sc, sparse)
    finally:
        d.close()
