"""pcr_select_sites on the GPU: the all-sites word DB against select_sites_cases.expected_entries (the oracle's pack + a numpy
restatement of Word::operator&), entry for entry; against pcr_select_words through the arg-max filter; the handle's state
around it; and the consumers of the word DB on it."""
import random

import numpy as np
import pytest

from pcramp_amd import api
from select_sites_cases import (FLOOR_SITES, N_RUN_SITES, argmax_filter, blind_spot_case, border_case, counts_matrix,
                                expected_entries, floor_case, groups_case, has_entry, iupac_case, oligos_of, packed_entries,
                                plant, pool_case, short_case, single_site_case, sites_per_oligo_and_sequence, substitute,
                                window_loc)
from testdata import family_targets, mutate, rand_seq, revcomp, sample_pair

pytestmark = pytest.mark.gpu

PCR_ERR_CAPACITY = -4
SQ = lambda t: float(np.float32(t) * np.float32(t))


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _sites(d, pairs, thr, min_len=18, which=api.TARGET):
    n = d.select_sites(pairs, thr, min_len, which=which)
    e = d.entries(which)
    assert len(e) == n
    return e


def _words(d, pairs, thr, min_len=18, which=api.TARGET):
    n = d.select_words(pairs, thr, min_len, which=which)
    e = d.entries(which)
    assert len(e) == n
    return e


# ---------------------------------------------------------------------------- 1. tile and block edges
@pytest.fixture(scope="module")
def border(oracle):
    seqs, pairs = border_case(random.Random(991), oracle)
    packed = packed_entries(oracle, seqs)
    return seqs, pairs, packed, counts_matrix(packed, oligos_of(pairs))


@pytest.mark.parametrize("thr", [1.0, 0.9, 0.85, 0.81, 0.7])
def test_tile_and_block_edges(dev, oracle, border, thr):
    seqs, pairs, packed, counts = border
    dev.load_texts(seqs)
    exp = expected_entries(oracle, seqs, pairs, thr, packed=packed, counts=counts)
    assert len(exp) > 100
    assert _sites(dev, pairs, thr) == exp


def test_edges_argmax_equals_select_words(dev, border):
    seqs, pairs, _, _ = border
    dev.load_texts(seqs)
    for thr in (0.9, 0.7):
        sites = _sites(dev, pairs, thr)
        words = _words(dev, pairs, thr)
        assert argmax_filter(sites, pairs, thr) == words
        assert len(sites) > len(words) > 0


# ---------------------------------------------------------------------------- 2. floor boundary
def test_floor_boundary(dev, oracle):
    seqs, pairs = floor_case(random.Random(3), oracle)
    dev.load_texts(seqs)
    for thr, present in ((0.85, [True, True, True, False]), (0.8, [True, True, True, True])):
        exp = expected_entries(oracle, seqs, pairs, thr)
        assert [has_entry(exp, 0, window_loc(at, 20), 1) for at, _ in FLOOR_SITES] == present
        assert len(exp) == sum(present)
        assert _sites(dev, pairs, thr) == exp


# ---------------------------------------------------------------------------- 3. short sequences
@pytest.mark.parametrize("min_len,min_n", [(18, 18), (15, 15)])
def test_short_sequences(dev, oracle, min_len, min_n):
    """Irregular words only, or a handful of regular windows (odd / even tail rule of the partial words)."""
    seqs, pairs = short_case(random.Random(4), oracle, min_n)
    dev.load_texts(seqs)
    for thr in (1.0, 0.8):
        exp = expected_entries(oracle, seqs, pairs, thr, min_len=min_len)
        assert len(exp) >= len(pairs)
        assert _sites(dev, pairs, thr, min_len) == exp


# ---------------------------------------------------------------------------- 4. IUPAC and pack's filters
def test_iupac_and_degeneracy_filter(dev, oracle):
    seqs, pairs = iupac_case(random.Random(5), oracle)
    dev.load_texts(seqs)
    for thr in (1.0, 0.9, 0.8):
        exp = expected_entries(oracle, seqs, pairs, thr)
        # the site over a run of 5 N is dropped by pack_max_degen, the one over 4 N is kept
        assert [has_entry(exp, 2, window_loc(at, 22), 1) for at, _ in N_RUN_SITES] == [False, True]
        assert set(e[3] for e in exp) == {0, 1, 2, 3}
        assert _sites(dev, pairs, thr) == exp


def test_gc_filter(oracle):
    seqs, pairs = iupac_case(random.Random(5), oracle)
    d = api.Screener(0, pack_min_gc=0.3, pack_max_gc=0.7)
    try:
        d.load_texts(seqs)
        for thr in (0.9, 0.6):
            exp = expected_entries(oracle, seqs, pairs, thr, min_gc=0.3, max_gc=0.7)
            assert 0 < len(exp) < len(expected_entries(oracle, seqs, pairs, thr))
            assert _sites(d, pairs, thr) == exp
    finally:
        d.close()


# ---------------------------------------------------------------------------- 5. orientation groups
@pytest.fixture(scope="module")
def groups(oracle):
    seqs, pairs = groups_case(random.Random(6), oracle)
    return seqs, pairs, packed_entries(oracle, seqs)


@pytest.mark.parametrize("n_pairs", [1, 64, 65, 130])
def test_orientation_groups(dev, oracle, groups, n_pairs):
    """1 counter word; 256 orientations = exactly one group of 8 words; one more; three groups -- with duplicated pairs."""
    seqs, pairs, packed = groups
    dev.load_texts(seqs)
    exp = expected_entries(oracle, seqs, pairs[:n_pairs], 0.8, packed=packed)
    assert len(exp) >= 2
    assert _sites(dev, pairs[:n_pairs], 0.8) == exp


# ---------------------------------------------------------------------------- 6. dense buckets
def test_poly_a_grows_the_buckets(dev, oracle):
    rng = random.Random(7)
    normal = [rand_seq(rng, 2000), rand_seq(rng, 1800)]
    seqs = [normal[0], "A" * 3000, normal[1]]
    w = oracle.centered_word
    pairs = [(w("A" * 18), w(revcomp(normal[0][700:720]))), (w(normal[1][100:122]), w(revcomp(normal[1][230:250])))]
    dev.load_texts(seqs)
    exp = expected_entries(oracle, seqs, pairs, 0.9)
    assert len(exp) > 2900                                # every window of the poly-A sequence, far beyond 64 ... 2 048 slots
    assert _sites(dev, pairs, 0.9) == exp
    # and back: the same handle on a sparse batch (the buckets shrink again)
    exp = expected_entries(oracle, seqs, pairs[1:], 0.9)
    assert _sites(dev, pairs[1:], 0.9) == exp


def test_low_threshold_many_hits_per_wave(dev, oracle):
    rng = random.Random(8)
    seqs = [rand_seq(rng, 10000) for _ in range(10)]
    pairs = []
    while len(pairs) < 20:
        p = sample_pair(rng, rng.choice(seqs))
        if p:
            pairs.append((oracle.centered_word(p[0]), oracle.centered_word(p[1])))
    dev.load_texts(seqs)
    exp = expected_entries(oracle, seqs, pairs, 0.5)
    per_seq = np.bincount([e[3] for e in exp])
    assert per_seq.min() >= 100                           # hundreds of entries per sequence
    assert _sites(dev, pairs, 0.5) == exp


def test_capacity_refusal_and_recovery(dev, oracle):
    rng = random.Random(9)
    normal = rand_seq(rng, 1500)
    seqs = [normal, "A" * 70000]
    w = oracle.centered_word
    dense = [(w("A" * 18), w(revcomp(normal[300:320])))]
    sparse = [(w(normal[200:221]), w(revcomp(normal[330:352])))]
    dev.load_texts(seqs)
    with pytest.raises(api.PcrError) as err:
        dev.select_sites(dense, 0.9)
    assert err.value.rc == PCR_ERR_CAPACITY and "pcr_select_sites" in str(err.value)
    exp = expected_entries(oracle, seqs, sparse, 0.8)
    assert len(exp) >= 2
    assert _sites(dev, sparse, 0.8) == exp
    assert _words(dev, sparse, 0.8) == argmax_filter(exp, sparse, 0.8)


# ---------------------------------------------------------------------------- differential: splits, inactive sequences
def test_splits_and_inactive_against_select_words(dev, oracle):
    rng = random.Random(12)
    seqs = family_targets(rng, 3, 5, 1200, div=0.04)
    pairs, where, f_txt = [], [], []
    for fam in range(3):
        root = seqs[5 * fam]
        for _ in range(3):
            a = rng.randrange(50, 900)
            f, r = root[a:a + rng.randint(18, 25)], revcomp(root[a + 120:a + 120 + rng.randint(18, 25)])
            pairs.append((oracle.centered_word(f), oracle.centered_word(r)))
            where.append((5 * fam, a))
            f_txt.append(f)
    for (s, a), f in zip(where, f_txt):
        seqs[s] = plant(seqs[s], a + 300 if a + 330 < 1200 else a - 300, substitute(rng, f, 2))   # a weaker second site
    dev.load_texts(seqs)
    for k, (s, a) in enumerate(where):
        for member in (s, s + 1 + k % 4):
            dev.split(member, a + (10 if k % 2 else -3))  # inside a site / just beside it
    active = [i % 4 != 1 for i in range(len(seqs))]
    dev.set_active(active)
    for thr in (0.9, 0.75):
        sites = _sites(dev, pairs, thr)
        assert sites and all(active[e[3]] for e in sites)
        words = _words(dev, pairs, thr)
        assert argmax_filter(sites, pairs, thr) == words
        assert len(sites) > len(words) > 0
    dev.set_active([True] * len(seqs))


# ---------------------------------------------------------------------------- state
def _state_case(rng, oracle):
    root = rand_seq(rng, 2500)
    seqs = [root] + [mutate(rng, root, 0.03) for _ in range(20)] + [rand_seq(rng, 1500) for _ in range(3)]
    batches = []
    for _ in range(3):
        pairs = []
        for _ in range(8):
            a = rng.randrange(0, 2200)
            pairs.append((oracle.centered_word(root[a:a + rng.randint(18, 25)]),
                          oracle.centered_word(revcomp(root[a + 100:a + 100 + rng.randint(18, 25)]))))
        batches.append(pairs)
    return seqs, batches


def test_select_words_after_select_sites(oracle):
    seqs, batches = _state_case(random.Random(13), oracle)
    pairs, thr = batches[0], SQ(0.9)
    fresh, used = api.Screener(0), api.Screener(0)
    try:
        for d in (fresh, used):
            d.load_texts(seqs)
        used.select_words(batches[1], thr)                # best[] holds an earlier pass
        assert len(_sites(used, pairs, 0.7)) > 0
        want, got = _words(fresh, pairs, thr), _words(used, pairs, thr)
        assert got == want and len(want) > 0
        b_want, b_got = fresh.find_target_match(pairs, 0.9), used.find_target_match(pairs, 0.9)
        assert np.array_equal(b_got, b_want) and b_want.any()
    finally:
        fresh.close()
        used.close()


def test_pending_screen_passes_are_final_after_select_sites(oracle):
    import torch
    seqs, batches = _state_case(random.Random(14), oracle)
    thr = SQ(0.9)
    d = api.Screener(0)
    try:
        d.load_texts(seqs)
        want = []
        for p in batches:
            d.select_words(p, thr)
            _, fr, rf, _ = d.amplify(p, 0.9, 0.9, 80, 200, False)
            want.append((np.array(fr), np.array(rf)))
        assert sum(int(w[0].sum()) + int(w[1].sum()) for w in want) > 0
        words = int(d.bitset_words())
        outs = [torch.full((2, len(p), words), -1, dtype=torch.int64, device="cuda:0") for p in batches]
        for p, o in zip(batches, outs):
            d.screen_device(p, thr, o[0].data_ptr(), o[1].data_ptr(), 0.9, 0.9, 80, 200, False)
        exp = expected_entries(oracle, seqs, batches[0], 0.8)
        assert _sites(d, batches[0], 0.8) == exp         # no synchronize() in between: the call drains the passes itself
        torch.cuda.synchronize()
        for w, o in zip(want, outs):
            a = o.cpu().numpy().view(np.uint64)
            for k in range(2):
                got = np.stack([api.bits_to_bool(a[k, i], len(seqs)) for i in range(a.shape[1])])
                assert np.array_equal(got, w[k])
    finally:
        d.close()


def test_empty_inputs(dev, oracle):
    seqs, pairs = floor_case(random.Random(3), oracle)
    dev.load_texts(seqs)
    assert dev.select_sites([], 0.9) == 0 and dev.entries() == []
    with pytest.raises(api.PcrError) as err:
        dev.select_sites(pairs, 0.9, which=2)
    assert err.value.rc == -1


# ---------------------------------------------------------------------------- consumers on the all-sites DB
def test_blind_spot_amplify_and_collect(dev, oracle):
    """A weaker site beside a better one of the same oligo: invisible after select_words, used after select_sites."""
    seqs, pair, (begin, end) = blind_spot_case(random.Random(15), oracle)
    dev.load_texts(seqs)
    thr = SQ(0.9)
    dev.select_words([pair], thr)
    assert dev.amplify([pair], 0.9, 0.9, 80, 200)[0][0].tolist() == [False, True]
    on1 = [(a["begin"], a["end"]) for a in dev.collect_amplicons(pair, 0.9, 80, 200) if a["sequence"] == 1]
    assert on1 == [(begin, end)]
    dev.select_sites([pair], thr)
    assert dev.amplify([pair], 0.9, 0.9, 80, 200)[0][0].tolist() == [True, True]
    amps = dev.collect_amplicons(pair, 0.9, 80, 200)
    assert [(a["sequence"], a["begin"], a["end"], a["orientation"]) for a in amps] == [(0, begin, end, 0), (1, begin, end, 0)]


def test_pool_products_select_all(dev, oracle):
    seqs, pool, (begin, end) = pool_case(random.Random(16), oracle)
    dev.load_texts(seqs)
    ids_t, rec_t = dev.pool_products(pool, 0.9, 80, 200, select=True)
    ids_a, rec_a = dev.pool_products(pool, 0.9, 80, 200, select="all")
    assert ids_t.tolist() == ids_a.tolist() == [0, 1, 2, 3]
    spurious = lambda r: r[(r["plus_oligo"] == 0) & (r["minus_oligo"] == 3) & (r["sequence"] == 0)]
    assert len(spurious(rec_t)) == 0
    got = spurious(rec_a)
    assert [(int(r["begin"]), int(r["end"]), int(r["intended"])) for r in got] == [(begin, end, 0)]
    assert rec_t[rec_t["intended"] == 1].tolist() == rec_a[rec_a["intended"] == 1].tolist()
    assert len(rec_t[rec_t["intended"] == 1]) == 4
    # select=False reads the DB select="all" left
    assert dev.pool_products(pool, 0.9, 80, 200, select=False)[1].tolist() == rec_a.tolist()
    with pytest.raises(ValueError):
        dev.pool_products(pool, 0.9, 80, 200, select="every")


def test_consumers_identical_where_sites_are_single(dev, oracle):
    """No sequence holds two sites of one oligo: the two DBs are the same, and so is everything read from them."""
    seqs, pairs = single_site_case(random.Random(11), oracle)
    thr = SQ(0.9)
    assert sites_per_oligo_and_sequence(oracle, seqs, pairs, thr) == 1
    exp = expected_entries(oracle, seqs, pairs, thr)
    variants = api.host_move_trials(pairs[0][0], 4, 1, 18, 25)
    out = []
    for which in (api.TARGET, api.BACKGROUND):
        dev.load_texts(seqs, which=which)
    for fill in (dev.select_words, dev.select_sites):
        fill(pairs, thr)
        fill(pairs, thr, which=api.BACKGROUND)
        assert dev.entries() == exp
        bits, fr, rf, cov = dev.amplify(pairs, 0.9, 0.9, 80, 200)
        amps = [dev.collect_amplicons(p, 0.9, 80, 200) for p in pairs]
        ids, rec = dev.pool_products(pairs, 0.9, 80, 200, select=False)
        bg = [dev.find_background_match(pairs, t, m, 0, 2000, evaluate_all=ev).tolist()
              for t, m in ((0.9, 1.0), (0.45, 1.6)) for ev in (False, True)]       # (the lower threshold sets bits)
        mc, mfr, mrf = dev.move_coverage(pairs[0], 0, variants, 0.9, 1.0, 80, 200)
        out.append((bits.tolist(), fr.tolist(), rf.tolist(), cov.tolist(), amps, ids.tolist(), rec.tolist(), bg,
                    mc.tolist(), mfr.tolist(), mrf.tolist()))
    assert out[0] == out[1]
    assert np.array(out[0][0]).any() and len(out[0][6]) > 0 and np.array(out[0][7][3]).any()
