"""pcr_pool_products / Screener.pool_products: every amplicon any two oligos of a primer pool form, against planted labels,
against per-combination collect_amplicons on the same word DB, against the oracle and (where it was built) the reference."""
import random
from collections import Counter, defaultdict

import numpy as np
import pytest

import amplicon_edges as AE
from pcramp_amd import api, synth, words as W
from testdata import rand_seq, revcomp

pytestmark = pytest.mark.gpu

PCR_ERR_ARG, PCR_ERR_STATE = -1, -3


def _primer(rng, n=20):
    while True:
        s = rand_seq(rng, n)
        if all(s[j:j + 4] != s[j] * 4 for j in range(n - 3)):
            return s


def _word(s):
    return W.centered_word(W.codes_from_text(s))


def _by_combo(rec):
    """records -> {(plus, minus): sorted [(sequence, begin, end, inner_start, inner_length)]}"""
    out = defaultdict(list)
    for r in rec:
        out[(int(r["plus_oligo"]), int(r["minus_oligo"]))].append(
            (int(r["sequence"]), int(r["begin"]), int(r["end"]), int(r["inner_start"]), int(r["inner_length"])))
    return out


def _distinct(pool, ids):
    words = {}
    for s, i in enumerate(ids):
        words.setdefault(int(i), pool[s // 2][s % 2])
    return [words[i] for i in range(len(words))]


def _check_order(ids, rec):
    key = [(int(r["plus_oligo"]), int(r["minus_oligo"]), int(r["sequence"]), int(r["begin"]), int(r["end"])) for r in rec]
    assert key == sorted(set(key)), "records are not unique and in key order"
    return key


def _intended_ok(pool, ids, rec):
    want = {frozenset((int(ids[2 * i]), int(ids[2 * i + 1]))) for i in range(len(pool))}
    for r in rec:
        assert bool(r["intended"]) == (frozenset((int(r["plus_oligo"]), int(r["minus_oligo"]))) in want)


def _collect(d, pair, thr, amp_min, amp_max, which):
    rec = d.collect_amplicons(pair, thr, amp_min, amp_max, which=which)
    t = lambda r: (r["sequence"], r["begin"], r["end"], r["inner_start"], r["inner_length"])
    return sorted(set(t(r) for r in rec if r["orientation"] == 0)), sorted(set(t(r) for r in rec if r["orientation"] == 1))


def _check_combo(d, words, by, a, b, thr, amp_min, amp_max, which):
    """The pool's products (a, b) and (b, a) == collect_amplicons((a, b)) orientation 0 / 1 on the same DB."""
    o0, o1 = _collect(d, (words[a], words[b]), thr, amp_min, amp_max, which)
    assert o0 == by.get((a, b), []), (a, b)
    assert o1 == by.get((b, a), []), (b, a)


def _bounds(by, a, b):
    return [(s, bg & 0xFFFFFFFF, e) for s, bg, e, _, _ in by.get((a, b), [])]


def _check_oracle(so, words, by, a, b, thr, amp_min, amp_max):
    """The oracle's AmpliconBounds for the pair (a, b): the same (sequence, begin, end) set as the products (a, b) and (b, a);
    for a = b it lists every product once per orientation."""
    mine = _bounds(by, a, b) + ([] if a == b else _bounds(by, b, a))
    try:
        bo, _ = so.collect_amplicons((words[a], words[b]), thr, amp_min, amp_max)
    except RuntimeError:
        # the reference keeps begin unsigned: a product whose plus primer hangs off the 5' end makes it throw
        # (AmpliconBounds: begin > end), where the oracle and the device report begin < 0
        assert b"begin > amplicon end" in so.f("session_error")(so.h), (a, b)
        assert any(x[1] >= 1 << 31 for x in mine), (a, b)
        return
    assert set(bo) == set(mine), (a, b)
    if a == b:
        cnt = Counter(bo)
        assert all(cnt[x] >= 2 for x in mine), (a, b)


# ------------------------------------------------------------------ 1. a planted pool with labels written by hand
def _planted():
    rng = random.Random(7301)
    F1, R1, F2, R2, F3, F4, R4, R5, F6, R6 = (_primer(rng) for _ in range(10))
    F5_inst = _primer(rng)
    F5 = F5_inst[:5] + ("R" if F5_inst[5] in "AG" else "Y") + F5_inst[6:12] + ("Y" if F5_inst[12] in "CT" else "R") + F5_inst[13:]
    seqs = []

    def seq(L, sites):
        s = list(rand_seq(rng, L))
        for pos, text in sites:
            s[pos:pos + len(text)] = list(text)
        seqs.append("".join(s))

    seq(1200, [(100, F1), (160, F2), (260, revcomp(R1)), (320, revcomp(R2))])   # 0: overlapping assays 1 and 2
    seq(1000, [(50, F3), (180, revcomp(R1))])                                  # 1: assay 3 shares R1 with assay 1
    seq(1500, [(300, F4), (410, revcomp(F4))])                                 # 2: F4 with itself
    seq(1000, [(200, F5_inst), (280, revcomp(R5))])                            # 3: degenerate F5
    seq(1000, [(100, F1), (260, revcomp(R1))])                                 # 4: inactive
    seq(1000, [(100, F1), (260, revcomp(R1))])                                 # 5: EOS split at 200
    for e in (178, 179, 299, 300):                                             # 6-9: lengths 79, 80, 200, 201
        seq(1000, [(100, F6), (e - 19, revcomp(R6))])
    pool = [(_word(f), _word(r)) for f, r in [(F1, R1), (F2, R2), (F3, R1), (F4, R4), (F5, R5), (F6, R6)]]
    return seqs, pool


PLANTED_IDS = [0, 1, 2, 3, 4, 1, 5, 6, 7, 8, 9, 10]
# (plus, minus, sequence, begin, end, intended) at 80..200; all primers are 20 bases
PLANTED_200 = [(0, 1, 0, 100, 279, 1), (2, 1, 0, 160, 279, 0), (2, 3, 0, 160, 339, 1), (4, 1, 1, 50, 199, 1), (5, 5, 2, 300, 429, 0),
               (7, 8, 3, 200, 299, 1), (9, 10, 7, 100, 179, 1), (9, 10, 8, 100, 299, 1)]
PLANTED_2000 = sorted(PLANTED_200 + [(0, 3, 0, 100, 339, 0), (9, 10, 9, 100, 300, 1)])


def _planted_screener(seqs, which, idx):
    d = api.Screener(0)
    d.load_texts([seqs[i] for i in idx], which=which)
    act = np.array([0 if i == 4 else 1 for i in idx], np.uint8)
    d.set_active(act, which=which)
    if 5 in idx:
        d.split(idx.index(5), 200, which=which)
    return d


@pytest.mark.parametrize("which", [api.TARGET, api.BACKGROUND])
def test_planted_pool(which):
    seqs, pool = _planted()
    idx = list(range(len(seqs))) if which == api.TARGET else [4, 0, 5, 2]    # the background: a few of them, renumbered
    d = _planted_screener(seqs, which, idx)
    try:
        for amp_max, want in ((200, PLANTED_200), (2000, PLANTED_2000)):
            ids, rec = d.pool_products(pool, 1.0, 80, amp_max, which=which)
            assert ids.tolist() == PLANTED_IDS
            exp = [(p, m, idx.index(s), b, e, it) for p, m, s, b, e, it in want if s in idx]
            got = [(int(r["plus_oligo"]), int(r["minus_oligo"]), int(r["sequence"]), int(r["begin"]), int(r["end"]), int(r["intended"]))
                   for r in rec]
            assert got == sorted(exp), amp_max
            for r in rec:                                                       # the padded inner stretch, 20-base primers
                assert r["inner_start"] == r["begin"] + 20 - 4 and r["inner_length"] == (r["end"] - 19) - r["inner_start"] + 8
    finally:
        d.close()


# ------------------------------------------------------------------ 2. the planted amplicon edges, every combination
@pytest.fixture(scope="module")
def cases(oracle):
    return AE.scenarios(oracle)


def _session(lib, sc):
    so = lib.session(**sc.opts)
    for s, w in zip(sc.seqs, sc.weights):
        so.add_target(s, w)
    for i in sc.inactive:
        so.set_active(i, False)
    for i, pos in sc.splits:
        so.split(i, pos)
    so.select(sc.pairs)
    return so


@pytest.mark.parametrize("k", range(AE.N_SCENARIOS))
def test_amplicon_edges(oracle, cases, k):
    from oracle_lib import Reference
    sc = cases[k]
    o = sc.opts
    thr, lo, hi = o["target_threshold"], o["amp_min"], o["amp_max"]
    sessions = [_session(oracle, sc)]
    if Reference.available():
        sessions.append(_session(Reference(), sc))
    d = api.Screener(0)
    try:
        d.load_texts(sc.seqs, sc.weights)
        act = np.ones(len(sc.seqs), np.uint8)
        act[list(sc.inactive)] = 0
        d.set_active(act)
        for i, pos in sc.splits:
            d.split(i, pos)
        d.select_words(sc.pairs, float(np.float32(thr) * np.float32(o["search_multiplier"])), o["min_primer"], o["optimize_5"], o["optimize_3"])
        ids, rec = d.pool_products(sc.pairs, thr, lo, hi, select=False)
        _check_order(ids, rec)
        _intended_ok(sc.pairs, ids, rec)
        words = _distinct(sc.pairs, ids)
        by = _by_combo(rec)
        for a in range(len(words)):
            for b in range(a, len(words)):
                _check_combo(d, words, by, a, b, thr, lo, hi, api.TARGET)
                for so in sessions:
                    _check_oracle(so, words, by, a, b, thr, lo, hi)
    finally:
        d.close()


# ------------------------------------------------------------------ 3. a synthetic mid-size pool
@pytest.fixture(scope="module")
def midsize():
    packed, off, lens = synth.make_sequences(1000, 10000, 4242)
    pool = synth.make_pairs(packed, off, lens, 32, 4243, degenerate=2)
    return packed, off, lens, pool


@pytest.mark.parametrize("which,amp_min,amp_max", [(api.TARGET, 80, 200), (api.BACKGROUND, 0, 2000)])
def test_midsize_pool(oracle, midsize, which, amp_min, amp_max):
    packed, off, lens, pool = midsize
    d = api.Screener(0)
    try:
        d.load_sequences(packed, off, lens, which=which)
        ids, rec = d.pool_products(pool, 0.9, amp_min, amp_max, which=which)
        _check_order(ids, rec)
        _intended_ok(pool, ids, rec)
        words = _distinct(pool, ids)
        by = _by_combo(rec)
        assert len(rec) > len(pool) and any(not r["intended"] for r in rec)    # cross products are there to be found
        combos = [(a, b) for a in range(len(words)) for b in range(a, len(words))]
        for a, b in combos:
            _check_combo(d, words, by, a, b, 0.9, amp_min, amp_max, which)
        # a seeded sample against the oracle, on the sequences those combos touch
        rng = random.Random(5 + which)
        have = sorted({(min(a, b), max(a, b)) for a, b in by})
        sample = rng.sample(have, min(8, len(have))) + rng.sample(combos, 4)
        seqs = sorted({s for a, b in sample for k in ((a, b), (b, a)) for s, *_ in by.get(k, [])})[:40]
        so = oracle.session(target_threshold=0.9)
        nb = 5000
        for s in seqs:
            so.add_target_packed(packed[int(off[s]):int(off[s]) + nb], 10000)
        so.select(pool, float(np.float32(0.9) * np.float32(0.9)))
        remap = {s: i for i, s in enumerate(seqs)}
        sub = defaultdict(list)
        for key, v in by.items():
            sub[key] = [(remap[x[0]],) + x[1:] for x in v if x[0] in remap]
        for a, b in sample:
            _check_oracle(so, words, sub, a, b, 0.9, amp_min, amp_max)
    finally:
        d.close()


# ------------------------------------------------------------------ 4. C2 scale, a 100-pair pool
def test_c2_pool():
    wl = synth.workload("C2")
    pool = synth.make_pairs(wl["packed"], wl["byte_offsets"], wl["lengths"], 100, 9100)
    d = api.Screener(0)
    try:
        d.load_sequences(wl["packed"], wl["byte_offsets"], wl["lengths"])
        ids, rec = d.pool_products(pool, 1.0, 80, 200)
        _check_order(ids, rec)
        _intended_ok(pool, ids, rec)
        words = _distinct(pool, ids)
        by = _by_combo(rec)
        for i, (f, r) in enumerate(pool):
            x, y = int(ids[2 * i]), int(ids[2 * i + 1])
            o0, o1 = _collect(d, (f, r), 1.0, 80, 200, api.TARGET)
            assert (o0, o1) == (by.get((x, y), []), by.get((y, x), [])), i
        have = {(min(a, b), max(a, b)) for a, b in by}
        for a, b in sorted(have):
            _check_combo(d, words, by, a, b, 1.0, 80, 200, api.TARGET)
        empty = [(a, b) for a in range(len(words)) for b in range(a, len(words)) if (a, b) not in have]
        for a, b in random.Random(2000).sample(empty, min(2000, len(empty))):
            assert _collect(d, (words[a], words[b]), 1.0, 80, 200, api.TARGET) == ([], []), (a, b)
    finally:
        d.close()


# ------------------------------------------------------------------ 5. cap, determinism, state, errors
def _raw(d, pool, which, cap, out=None, ids=None, n=None, threshold=1.0, amp=(80, 200)):
    a = W.pairs_array(pool)
    ids = np.zeros(max(2 * len(pool), 1), np.uint32) if ids is None else ids
    return d.L.pcr_pool_products(d.h, which, a.ctypes.data if n != -1 else None, len(pool) if n is None or n == -1 else n,
                                 threshold, amp[0], amp[1], ids.ctypes.data, None if out is None else out.ctypes.data, cap)


def test_cap_determinism_state(midsize):
    import torch
    packed, off, lens, pool = midsize
    d = api.Screener(0)
    try:
        d.load_sequences(packed, off, lens)
        pool = pairs = pool[:8]
        thr = float(np.float32(0.9) * np.float32(0.9))
        words = int(d.bitset_words())

        def screen():
            out = torch.full((2, len(pairs), words), -1, dtype=torch.int64, device="cuda:0")
            d.screen_device(pairs, thr, out[0].data_ptr(), out[1].data_ptr(), 0.9, 0.9, 80, 200, False)
            d.synchronize()
            torch.cuda.synchronize()
            return out.cpu().numpy()

        def state():
            return (d.find_target_match(pairs, 0.9), [d.collect_amplicons(p, 0.9) for p in pairs])

        s0 = screen()
        bits0, col0 = state()
        ids, rec = d.pool_products(pool, 0.9, 80, 200, select=False)
        ids2, rec2 = d.pool_products(pool, 0.9, 80, 200, select=False)
        assert ids.tobytes() == ids2.tobytes() and rec.tobytes() == rec2.tobytes()
        total = len(rec)
        assert total > 2
        assert _raw(d, pool, api.TARGET, 0, threshold=0.9) == total                  # count only
        small = np.zeros(total - 1, api.PRODUCT_DTYPE)
        assert _raw(d, pool, api.TARGET, total - 1, small, threshold=0.9) == total
        ids3, rec3 = d.pool_products(pool, 0.9, 80, 200, select=False, cap=1)       # retried internally
        assert rec3.tobytes() == rec.tobytes()
        big = np.zeros(total + 100, api.PRODUCT_DTYPE)
        assert _raw(d, pool, api.TARGET, total + 100, big, threshold=0.9) == total
        assert big[:total].tobytes() == rec.tobytes()
        bits1, col1 = state()
        assert np.array_equal(bits0, bits1) and col0 == col1
        assert np.array_equal(s0, screen())
        # errors
        assert _raw(d, pool, api.MULTIPLEX, 0) == PCR_ERR_ARG
        assert _raw(d, pool, api.TARGET, 0, n=-1) == PCR_ERR_ARG                     # pool = NULL
        assert _raw(d, pool, api.TARGET, 5) == PCR_ERR_ARG                           # out = NULL with cap > 0
        assert _raw(d, pool * 129, api.TARGET, 0) == PCR_ERR_ARG                     # 1 032 pairs
        assert _raw(d, pool * 128, api.TARGET, 0, threshold=0.9) == total            # 1 024 pairs, the same 16 oligos
        assert _raw(d, pool, api.TARGET, 0, n=0) == 0
        assert _raw(d, pool, api.BACKGROUND, 0) == PCR_ERR_STATE                     # no word DB there
        with pytest.raises(api.PcrError):
            d.pool_products(pool, 1.0, select=False, which=api.BACKGROUND)
    finally:
        d.close()
