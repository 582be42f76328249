"""The planted amplicon edges of tests/amplicon_edges.py through every pairing kernel the entry points reach, against
the oracle and the labels: amplify / find_target_match / compute_coverage (k_pair), the fused pass at each bucket class
(k_post, k_post_big<256>, and the unfused tail beyond), move_coverage at small and large buckets
(k_pair_moves, k_pair_moves_seq), collect_amplicons (k_collect_amplicons) and find_background_match (k_bg_emit<64>, <128>, <0>).
Bits per orientation and coverage floats are compared exactly.  Every test asserts the bucket band it was built for, so that it shows which form ran."""
import re

import numpy as np
import pytest

import amplicon_edges as AE
from pcramp_amd import api, words as W
from testdata import move_variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(oracle):
    return AE.scenarios(oracle)


def _oracle(oracle, sc, splits_first=False):
    so = oracle.session(**sc.opts)
    for s, w in zip(sc.seqs, sc.weights):
        so.add_target(s, w)
    for i in sc.inactive:
        so.set_active(i, False)
    if splits_first:
        for i, pos in sc.splits:
            so.split(i, pos)
    so.select(sc.pairs)
    if not splits_first:
        for i, pos in sc.splits:
            so.split(i, pos)
    return so


def _load(d, sc):
    d.load_texts(sc.seqs, sc.weights)
    act = np.ones(len(sc.seqs), np.uint8)
    act[list(sc.inactive)] = 0
    d.set_active(act)


def _load_split(d, sc):
    """Load, deactivate, split: split() drops the word DB, so on the device the EOS go in before the selection (the oracle
    with splits_first=True does the same; the labels assume splits after it, so they are checked where a scenario has none)."""
    _load(d, sc)
    for i, pos in sc.splits:
        d.split(i, pos)


def _thr(o):
    return float(np.float32(o["target_threshold"]) * np.float32(o["search_multiplier"]))


def _select(d, sc):
    o = sc.opts
    return d.select_words(sc.pairs, _thr(o), o["min_primer"], o["optimize_5"], o["optimize_3"])


def _check_bits(sc, so, fr, rf, labels=True):
    """Device bits == the oracle's (splits made before the selection, as on the device); and == the labels: all bits where
    the scenario has no splits, the labelled (sequence, pair, orientation) bits through split_first_answer where it has."""
    want_fr, want_rf = AE.expected(sc)
    for p, pair in enumerate(sc.pairs):
        _, ori = so.target_match(pair, orient=True)
        assert np.array_equal(np.asarray(fr[p]), (ori & 1) != 0), (sc.name, p, "FR")
        assert np.array_equal(np.asarray(rf[p]), (ori & 2) != 0), (sc.name, p, "RF")
        if labels and not sc.splits:
            assert np.array_equal(np.asarray(fr[p]), want_fr[p]) and np.array_equal(np.asarray(rf[p]), want_rf[p]), (sc.name, p)
    if labels and sc.splits:
        for l in sc.labels:
            got = (fr if l.orient == "FR" else rf)[l.pair][l.seq]
            assert bool(got) == AE.split_first_answer(l), (sc.name, l)


# the identity scenarios: 6-17, each threshold exactly at a score, one float above and one below
EXACT = list(range(6, AE.N_SCENARIOS))


@pytest.mark.parametrize("k", range(AE.N_SCENARIOS))
def test_k_pair(oracle, cases, k):
    """amplify / find_target_match / compute_coverage."""
    sc = cases[k]
    o = sc.opts
    so = _oracle(oracle, sc, splits_first=True)
    d = api.Screener(0)
    try:
        _load_split(d, sc)
        n = _select(d, sc)
        assert d.entries() == so.db_entries() and n == len(so.db_entries())
        assert AE.largest_bucket(d.entries()) <= 64
        bits, fr, rf, _ = d.amplify(sc.pairs, o["target_threshold"], o["target_threshold"], o["amp_min"], o["amp_max"],
                                    o["use_taq_mama"])
        _check_bits(sc, so, fr, rf)
        ft = d.find_target_match(sc.pairs, o["target_threshold"], o["amp_min"], o["amp_max"], o["use_taq_mama"])
        assert np.array_equal(ft, bits)
        cov = d.compute_coverage(sc.pairs, o["target_threshold"], o["search_multiplier"], o["amp_min"], o["amp_max"],
                                 o["use_taq_mama"])
        for p, pair in enumerate(sc.pairs):
            assert cov[p] == np.float32(so.target_coverage(pair)), (sc.name, p)
    finally:
        d.close()


# (decoy copies, largest bucket fill, bucket slots the set ends with, from the PCRAMP_DEBUG scan plan lines): k_post at 64
# slots, k_post_big<256> (an overflowing 64-slot pass grows the buckets straight to 256 for a fill of 65-128), and the
# unfused k_finalize + k_match + k_pair path beyond 256
BUCKETS = [(0, (1, 64), (64, 64)), (100, (65, 128), (256, 256)), (300, (257, 4096), (512, 1 << 20))]


# (scenarios 4 and 15-17 grow their buckets to 512 slots at 100 decoy copies: they run at 64 and beyond 256 only)
GROW_512 = (4, 15, 16, 17)


@pytest.mark.parametrize("k,copies,band,line", [(k,) + b for k in [0, 1, 2, 3, 4] + EXACT for b in BUCKETS
                                                if not (k in GROW_512 and b[0] == 100)])
def test_fused_pass(oracle, cases, capfd, monkeypatch, k, copies, band, line):
    """screen_device, three passes over one loaded set (the later ones lean), at each bucket class of the fused tail;
    EOS set by split() before the pass."""
    import torch
    sc = cases[k]
    if copies:
        sc = AE.padded(sc, oracle, copies)
    if len(sc.pairs) % 2:
        sc = AE.padded(sc, oracle, 0, seed=11)                   # an even pair count: 16-byte rows for the fused tail
    o = sc.opts
    so = _oracle(oracle, sc, splits_first=True)
    assert band[0] <= AE.largest_bucket(so.db_entries()) <= band[1]
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    d = api.Screener(0)
    try:
        _load(d, sc)
        for i, pos in sc.splits:
            d.split(i, pos)
        words = int(d.bitset_words())
        capfd.readouterr()
        for rep in range(3):
            out = torch.full((2, len(sc.pairs), words), -1, dtype=torch.int64, device="cuda:0")
            d.screen_device(sc.pairs, _thr(o), out[0].data_ptr(), out[1].data_ptr(), o["target_threshold"], o["target_threshold"],
                            o["amp_min"], o["amp_max"], bool(o["use_taq_mama"]), o["min_primer"], bool(o["optimize_5"]),
                            bool(o["optimize_3"]))
            d.synchronize()
            torch.cuda.synchronize()
            a = out.cpu().numpy().view(np.uint64)
            fr = [api.bits_to_bool(a[0, p], len(sc.seqs)) for p in range(len(sc.pairs))]
            rf = [api.bits_to_bool(a[1, p], len(sc.seqs)) for p in range(len(sc.pairs))]
            _check_bits(sc, so, fr, rf)
            assert d.entries() == so.db_entries(), rep
        err = capfd.readouterr().err
        caps = [int(x) for x in re.findall(r"scan plan: .*, (\d+)-slot buckets", err)]
        assert len(caps) >= 3, err[-2000:]                 # one plan per pass, and one per replay after an overflow
        lo, hi = line
        assert lo <= max(caps) <= hi, caps                 # buckets only grow within a loaded set
    finally:
        d.close()


def test_fused_pass_many_pairs(oracle, cases):
    """More than 64 pairs: the unfused tail of screen_device."""
    import torch
    sc = cases[4]
    extra = [AE.padded(sc, oracle, 0, seed=100 + j).pairs[-1] for j in range(66)]
    sc = sc._replace(pairs=list(sc.pairs) + extra)
    o = sc.opts
    so = _oracle(oracle, sc, splits_first=True)
    d = api.Screener(0)
    try:
        _load(d, sc)
        for i, pos in sc.splits:
            d.split(i, pos)
        words = int(d.bitset_words())
        for rep in range(2):
            out = torch.full((2, len(sc.pairs), words), -1, dtype=torch.int64, device="cuda:0")
            d.screen_device(sc.pairs, _thr(o), out[0].data_ptr(), out[1].data_ptr(), o["target_threshold"], o["target_threshold"],
                            o["amp_min"], o["amp_max"], bool(o["use_taq_mama"]), o["min_primer"])
            d.synchronize()
            torch.cuda.synchronize()
            a = out.cpu().numpy().view(np.uint64)
            fr = [api.bits_to_bool(a[0, p], len(sc.seqs)) for p in range(len(sc.pairs))]
            rf = [api.bits_to_bool(a[1, p], len(sc.seqs)) for p in range(len(sc.pairs))]
            _check_bits(sc, so, fr, rf, labels=False)
    finally:
        d.close()


def _variants(pair, side):
    out = []
    for kind in ("trim5", "trim3", "grow5", "grow3", "inc"):
        out += move_variants(W, pair[side], kind)[:3]
    return out


@pytest.mark.parametrize("copies,band", [(0, (1, 64)), (300, (257, 4096))])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4] + EXACT)
def test_move_coverage(oracle, cases, k, copies, band):
    """move_coverage with variants that change the edited oligo's length, at 64-slot buckets (k_pair_moves) and at
    buckets of 256 slots or more (k_pair_moves_seq)."""
    sc = cases[k]
    if copies:
        sc = AE.padded(sc, oracle, copies)
    o = sc.opts
    so = _oracle(oracle, sc, splits_first=True)
    d = api.Screener(0)
    try:
        _load_split(d, sc)
        _select(d, sc)
        assert band[0] <= AE.largest_bucket(d.entries()) <= band[1]
        n_hit = 0
        for p, pair in enumerate(sc.pairs):
            for side in (0, 1):
                var = _variants(pair, side)
                cov, fr, rf = d.move_coverage(pair, side, var, o["target_threshold"], o["search_multiplier"], o["amp_min"],
                                              o["amp_max"], bool(o["use_taq_mama"]))
                ocov, ori = so.move_coverage(pair, side, var, orient=True)
                assert np.array_equal(cov, ocov), (sc.name, p, side)
                assert np.array_equal(fr, (ori & 1) != 0) and np.array_equal(rf, (ori & 2) != 0), (sc.name, p, side)
                n_hit += int(np.count_nonzero(ori))
        assert n_hit > 0
    finally:
        d.close()


@pytest.mark.parametrize("k", range(AE.N_SCENARIOS))
def test_collect_amplicons(oracle, cases, k):
    """k_collect_amplicons: the same AmpliconBounds as the oracle and as the labels (padded inner stretch, no end clamp)."""
    sc = cases[k]
    o = sc.opts
    so = _oracle(oracle, sc, splits_first=True)
    d = api.Screener(0)
    try:
        _load_split(d, sc)
        _select(d, sc)
        for p, pair in enumerate(sc.pairs):
            bo, _ = so.collect_amplicons(pair, o["target_threshold"], o["amp_min"], o["amp_max"])
            rec = d.collect_amplicons(pair, o["target_threshold"], o["amp_min"], o["amp_max"])
            got = sorted((r["sequence"], r["begin"] & 0xFFFFFFFF, r["end"]) for r in rec)
            assert got == sorted(bo), (sc.name, p)
            if not sc.splits:
                assert sorted(set(got)) == AE.expected_bounds(sc, p), (sc.name, p)
    finally:
        d.close()


# (decoy copies, fewest entries of the largest bucket) per scenario for 128-slot buckets.  The buckets grow with the HITS of a
# pass, and at the background selection's low threshold a pass records hits that a later, better one supersedes, in numbers that
# depend on the order its workgroups ran in.  Measured on an MI355X the largest fill of these sets lies 20 to 35 above the entries
# of the largest bucket and varies by about 10 between runs (at 70 entries: 90 to 105), so 65 or more entries still end at 128
# slots; the partner scenario (1) and the one selected with shift candidates (4) record 45 to 57 hits more than they keep entries
# (66 entries: a fill of 123; 75: 122 to 126, and 256 slots in one run of two), so they stay at 46 and 48 entries (fills of 97 to 98).
MID_COPIES = {0: (44, 65), 1: (32, 40), 2: (60, 65), 3: (32, 65), 4: (36, 40), 6: (60, 65), 9: (60, 65), 12: (50, 65)}


@pytest.mark.parametrize("copies,band", [(0, (1, 64)), (200, (129, 4096)), ("mid", (65, 128))])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 6, 9, 12])
def test_background_match(oracle, cases, capfd, monkeypatch, k, copies, band):
    """find_background_match on the planted sequences as a background set, the reference's index mode and evaluate_all,
    under the background window and the scenario's: k_bg_emit<64> at 64-slot buckets, k_bg_emit<128> at 128 slots (asserted
    from the library's debug line), k_bg_emit<0> beyond 128 slots."""
    sc = cases[k]
    mid = copies == "mid"
    if mid:
        copies, lo = MID_COPIES[k]
        band = (lo, band[1])
    if copies:
        sc = AE.padded(sc, oracle, copies)
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    so = oracle.session()
    for s in sc.seqs:
        so.add_target(s)
    bt = 0.5                                   # a same-strand times an opposite-strand score: 0.8 almost never fires here
    thr = float(np.float32(bt) * np.float32(0.9))
    d = api.Screener(0)
    try:
        d.load_texts(sc.seqs, which=api.BACKGROUND)
        assert d.select_words(sc.pairs, thr, 16, which=api.BACKGROUND) == so.select(sc.pairs, threshold=thr, min_len_override=16)
        assert band[0] <= AE.largest_bucket(d.entries(which=api.BACKGROUND)) <= band[1]
        hits = 0
        for amp in ((0, 2000), (sc.opts["amp_min"], sc.opts["amp_max"])):
            for ev in (False, True):
                bits = d.find_background_match(sc.pairs, bt, 0.9, amp[0], amp[1], False, evaluate_all=ev)
                for p, pair in enumerate(sc.pairs):
                    ob, _ = so.background_match(pair, bt, 0.9, amp[0], amp[1], 0, emulate_index_bug=int(not ev))
                    assert np.array_equal(bits[p], ob.astype(bool)), (sc.name, amp, ev, p)
                    hits += int(ob.sum())
        assert hits > 0
        if mid:
            forms = re.findall(r"background_match: attempt \d+, (emit<\d+>), (\d+)-slot buckets", capfd.readouterr().err)
            assert len(forms) >= 4 and set(forms) == {("emit<128>", "128")}, forms
    finally:
        d.close()
