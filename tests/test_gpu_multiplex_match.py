"""pcr_multiplex_match (find_multiplex_background_match on the device: k_seq_codes, k_mx_jobs, the streaming k_sw<false>,
k_mx_score) against the oracle on the scenarios of tests/multiplex_templates.py: templates of 1 to 32 766 bases with
sites at both ends and across the 32-column chunk edges, repeated sites whose tie decides the bit, thresholds on
attainable scores, IUPAC / N / EOS, sets of 1 to 70 001 sequences, batches of 1 to 300 pairs; the cached code strings,
the three sets, the refusals, and pcr_multiplex_screen with amplicons of up to 1 500 bases.  Every comparison is exact.
The oracle's bits are held to the compiled reference in tests/test_multiplex_templates_host.py.  Run with `-m gpu`."""
import random

import numpy as np
import pytest

import multiplex_templates as MT
from pcramp_amd import api
from test_gpu_multiplex_screen import _expected
from testdata import family_targets, rand_seq, revcomp, sample_pair

pytestmark = pytest.mark.gpu

POISON = np.uint64(0xA5A5A5A5A5A5A5A5)
PAD = 16                                                                      # poisoned words behind the ones the call owns
ERR_CAPACITY = -4                                                             # PCR_ERR_CAPACITY
SMALL = [n for n in MT.NAMES if n not in ("big", "batches")]


@pytest.fixture(scope="module")
def dev():
    s = api.Screener(0)
    yield s
    s.close()


def raw_call(dev, which, pairs, thr, taq):
    """pcr_multiplex_match through the ABI into a poisoned array -> (rc, the words the call owns, the words behind them)."""
    a = api.W.pairs_array(pairs) if len(pairs) else np.zeros((0, 4), np.uint64)
    own = len(pairs) * int(dev.bitset_words(which))
    buf = np.full(own + PAD, POISON, np.uint64)
    rc = dev.L.pcr_multiplex_match(dev.h, which, a.ctypes.data if len(pairs) else None, len(pairs), thr, int(taq), buf.ctypes.data)
    return rc, buf[:own], buf[own:]


def want_words(sc, pairs_idx, thr, taq):
    return np.concatenate([api.bool_to_bits(sc.want[(p, thr, taq)]) for p in pairs_idx])


def check_scenario(dev, sc, which=api.BACKGROUND, load=True):
    """Every threshold and TaqMAMA setting through the Python surface, and one call through the ABI into a poisoned array:
    all n_pairs x ceil(n / 64) words written, bits at or past n zero, nothing behind them touched."""
    if load:
        dev.load_texts(sc.seqs, sc.weights, which=which)
    assert dev.num_sequences(which) == len(sc.seqs)
    rows = list(sc.cpu_pairs)
    for thr in sc.thresholds:
        for taq in sc.taq:
            bits = dev.find_multiplex_background_match(sc.pairs, thr, taq, which=which)
            assert bits.shape == (len(sc.pairs), len(sc.seqs))
            for p in rows:
                want = sc.want[(p, thr, taq)]
                bad = np.nonzero(bits[p] != want)[0]
                assert bad.size == 0, (sc.name, p, thr, taq, bad[:8], [sc.labels[i] for i in bad[:4]])
    thr, taq = sc.thresholds[len(sc.thresholds) // 2], sc.taq[0]
    rc, own, behind = raw_call(dev, which, [sc.pairs[p] for p in rows], thr, taq)
    assert rc == 0, api._err(dev.L)
    assert np.array_equal(own, want_words(sc, rows, thr, taq)), sc.name
    assert (behind == POISON).all()


@pytest.mark.parametrize("name", SMALL)
def test_scenario_equals_oracle(dev, oracle, name):
    check_scenario(dev, MT.scenario(oracle, name))


@pytest.mark.parametrize("n", MT.SMALL_SIZES + MT.BIG_SIZES)
def test_set_sizes(dev, oracle, n):
    """1 .. 129 sequences around the 64-bit words of a row, then 65 535, 65 536 and 70 001: more sequences than one extent
    of a launch grid holds.  The marked hits (index 0, 63, 64, 65 534, 65 535, 65 536, the last) are where they belong."""
    sc = MT.prefix(MT.scenario(oracle, "sizes" if n <= 129 else "big"), n)
    check_scenario(dev, sc)
    if n > 129:
        hits = np.nonzero(dev.find_multiplex_background_match(sc.pairs, 0.95, 0)[0])[0]
        marked = [i for i, l in enumerate(sc.labels) if l.what == "hit at a marked index"]
        assert list(hits) == marked and {0, 63, 64, n - 1} <= set(marked)


def test_batches(dev, oracle):
    """1, 2, 65 and 300 pairs over the ladder set: the row of pair k does not depend on the batch it came in, and the rows
    the oracle answered (the last of each batch) are the oracle's."""
    sc = MT.scenario(oracle, "batches")
    dev.load_texts(sc.seqs, sc.weights, which=api.BACKGROUND)
    thr = sc.thresholds[0]
    for taq in sc.taq:
        full = dev.find_multiplex_background_match(sc.pairs, thr, taq)
        assert full.shape == (300, len(sc.seqs))
        for b in MT.BATCHES:
            got = dev.find_multiplex_background_match(sc.pairs[:b], thr, taq)
            assert np.array_equal(got, full[:b]), (b, taq)
            assert np.array_equal(got[b - 1], sc.want[(b - 1, thr, taq)]), (b, taq)
        for k in (1, 64, 150, 299):
            assert np.array_equal(dev.find_multiplex_background_match([sc.pairs[k]], thr, taq)[0], full[k]), (k, taq)
        assert len({sc.want[(p, thr, taq)].tobytes() for p in sc.cpu_pairs}) == len(sc.cpu_pairs)   # a row taken from another pair shows


def _oracle_session(oracle, seqs, weights):
    so = oracle.session()
    for s, w in zip(seqs, weights):
        so.add_target(s, w)
    return so


def test_cached_code_strings(dev, oracle):
    """The code strings of a set are built by the first call and kept: a split(), a reload with another set of the same
    count and lengths, and a change of the active flags (which this search ignores, as the reference does) must each be
    answered from the set as it then is.  Every state is compared with an oracle session brought into the same state."""
    sc = MT.scenario(oracle, "equality")
    pair, thr = sc.pairs[0], MT.equality_threshold(2 * 18, 18)
    dev.load_texts(sc.seqs, sc.weights, which=api.BACKGROUND)
    so = _oracle_session(oracle, sc.seqs, sc.weights)
    call = lambda taq: dev.find_multiplex_background_match([pair], thr, taq)[0]
    before = call(0)
    assert np.array_equal(before, so.multiplex_match(pair, thr, 0).astype(bool))
    # an EOS split into the whole-primer sites of F: each of them loses its perfect score
    cut = [i for i, l in enumerate(sc.labels) if l.what == "suffix 0" and l.lane == 0]
    assert len(cut) == 3 and all(before[i] for i in cut)
    for i in cut:
        pos = int(sc.labels[i].place.split()[1]) + 9
        dev.split(i, pos, which=api.BACKGROUND)
        so.split(i, pos)
    for taq in (0, 1):
        want = so.multiplex_match(pair, thr, taq).astype(bool)
        assert np.array_equal(call(taq), want)
        assert not any(want[i] for i in cut)
    # another set, same count, same lengths: every text reversed
    seqs2 = [s[::-1] for s in sc.seqs]
    dev.load_texts(seqs2, sc.weights, which=api.BACKGROUND)
    so2 = _oracle_session(oracle, seqs2, sc.weights)
    low = sc.thresholds[len(sc.thresholds) // 2]
    for t in (thr, low):
        want = so2.multiplex_match(pair, t, 1).astype(bool)
        assert np.array_equal(dev.find_multiplex_background_match([pair], t, 1)[0], want)
    assert not np.array_equal(want, sc.want[(0, low, 1)])
    # back to the scenario, then active flags off for every other sequence
    dev.load_texts(sc.seqs, sc.weights, which=api.BACKGROUND)
    assert np.array_equal(call(1), sc.want[(0, thr, 1)])
    so3 = _oracle_session(oracle, sc.seqs, sc.weights)
    flags = np.array([i % 2 for i in range(len(sc.seqs))], np.uint8)
    dev.set_active(flags, which=api.BACKGROUND)
    for i, f in enumerate(flags):
        so3.set_active(i, bool(f))
    want = so3.multiplex_match(pair, thr, 1).astype(bool)
    assert np.array_equal(call(1), want) and want[::2].any()
    dev.set_active(1 - flags, which=api.BACKGROUND)
    assert np.array_equal(call(1), want)


def test_the_three_sets_answer_alike(oracle):
    """The same sequences loaded as TARGET, BACKGROUND and MULTIPLEX give the same bits: the oracle's."""
    sc = MT.scenario(oracle, "alphabet")
    d = api.Screener(0)
    try:
        for which in (api.TARGET, api.BACKGROUND, api.MULTIPLEX):
            check_scenario(d, sc, which=which)
        for which in (api.TARGET, api.BACKGROUND, api.MULTIPLEX):             # all three loaded: none has disturbed another
            check_scenario(d, sc, which=which, load=False)
    finally:
        d.close()


def test_refusals(oracle):
    """A template of 32 767 bases -- one past what the reference can align -- is refused with PCR_ERR_CAPACITY and a
    message naming the limit; bits is then all zero (include/pcramp_hip.h), nothing behind it is touched, and the handle
    answers the next call.  32 766 bases are accepted (the ladders).  An empty set and zero pairs return OK and write nothing."""
    sc = MT.scenario(oracle, "sizes")
    rng = random.Random(5)
    d = api.Screener(0)
    try:
        rc, own, behind = raw_call(d, api.MULTIPLEX, sc.pairs, 0.6, 0)          # a set that was never loaded
        assert rc == 0 and own.size == 0 and (behind == POISON).all()
        seqs = [sc.seqs[0], rand_seq(rng, 32767), sc.seqs[1]]
        d.load_texts(seqs, which=api.BACKGROUND)
        rc, own, behind = raw_call(d, api.BACKGROUND, sc.pairs, 0.6, 0)
        assert rc == ERR_CAPACITY and "32766" in api._err(d.L)
        assert own.size == 2 and not own.any() and (behind == POISON).all()
        seqs[1] = seqs[1][:32766]
        d.load_texts(seqs, which=api.BACKGROUND)
        so = _oracle_session(oracle, seqs, [1.0] * 3)
        got = d.find_multiplex_background_match(sc.pairs, 0.6, 0)
        for p, pair in enumerate(sc.pairs):
            assert np.array_equal(got[p], so.multiplex_match(pair, 0.6, 0).astype(bool))
        assert got[0, 0]
        check_scenario(d, sc)
        rc, own, behind = raw_call(d, api.BACKGROUND, [], 0.6, 0)               # zero pairs
        assert rc == 0 and own.size == 0 and (behind == POISON).all()
    finally:
        d.close()


def _screen_case(oracle, amp_min, amp_max, taq):
    """Targets of 2 500 bases in three families, a pool of 3 assays with amplicons of 300 .. 1 450 bases, 70 accepted
    amplicons (the pool's, stretches of the targets, unrelated text) with weights 1 + 0.25 (i mod 7), and trials whose own
    amplicons run from 80 to 1 500 bases -> (targets, amplicons, weights, pool, trials, oracle target session, oracle amplicon session)."""
    rng = random.Random(20261017)
    seqs = family_targets(rng, 3, 4, 2500, div=0.03)

    def pick(amplicon):
        while True:
            t = rng.choice(seqs)
            p = sample_pair(rng, t, amplicon=amplicon)
            if p:
                i, j = t.find(p[0]), t.find(revcomp(p[1]))
                if 30 <= i < j and j + len(p[1]) + 30 <= len(t):
                    return p, t[i + len(p[0]) - 5:j + 5], (t, i, j + len(p[1]))
    pool_txt, amps, around = [], [], []
    for amplicon in ((300, 600), (700, 1000), (1100, 1450)):
        p, a, (t, i, e) = pick(amplicon)
        pool_txt.append(p)
        amps.append(a)
        around.append((t[i - 24:i - 4], revcomp(t[e + 4:e + 24])))             # a trial whose amplicon holds this assay's whole footprint
    cands = [pick(amplicon)[0] for amplicon in ((80, 200), (200, 500), (500, 900), (900, 1300), (1300, 1500), (1400, 1500))]
    cands += around[:2]
    a = amps[1]
    cands.append((a[40:60], revcomp(a[len(a) - 70:len(a) - 50])))              # sits on a pooled amplicon
    cands.append((revcomp(pool_txt[0][0]), cands[0][1]))                       # cannot share a tube with the pool
    while len(amps) < 70:                                                      # stretches of the targets and unrelated text
        t = rng.choice(seqs)
        n = rng.randint(80, 1500)
        k = rng.randrange(0, len(t) - n)
        amps.append(t[k:k + n] if len(amps) % 3 else rand_seq(rng, n))
    weights = MT.weights_for(len(amps))
    w = oracle.centered_word
    pool, trials = [(w(f), w(r)) for f, r in pool_txt], [(w(f), w(r)) for f, r in cands]
    o = dict(target_threshold=THR_T, search_multiplier=MULT, amp_min=amp_min, amp_max=amp_max, use_taq_mama=taq, pack_max_degen=256,
             pack_min_gc=0.0, pack_max_gc=1.0, min_primer=18, optimize_5=0, optimize_3=0)
    ts = oracle.session(**o)
    for q in seqs:
        ts.add_target(q, 1.0)
    ams = oracle.session(use_taq_mama=taq)
    for s, wt in zip(amps, weights):
        ams.add_target(s, wt)
    ts.select(trials + pool)
    return seqs, amps, weights, pool, trials, ts, ams


THR_T, MULT, BG_THR = 0.9, 0.9, 0.8


def test_multiplex_screen_long_amplicons(oracle):
    """pcr_multiplex_screen with a target amplicon range of 80 .. 1 500: the amplicon stretches that become the scratch
    set span dozens of 32-column chunks; 3 pooled assays; a MULTIPLEX set of more than 64 sequences with weights other than
    1.  multiplex_cover and pool_cover equal the composition from oracle pieces of test_gpu_multiplex_screen._expected."""
    amp_min, amp_max, taq = 80, 1500, 1
    seqs, amps, weights, pool, trials, ts, ams = _screen_case(oracle, amp_min, amp_max, taq)
    wc, wm, wp = _expected(oracle, ts, ams, pool, trials, THR_T, BG_THR, taq, amp_min=amp_min, amp_max=amp_max)
    # the case is what it claims: one trial cannot join the pool; the covers are weighted sums (not counts); the pool's primers
    # reach several trials' amplicons; the stretches that form the scratch set are long
    assert not all(wc) and sum(wc) >= 7, wc
    assert any(x > 0 and x != int(x) for x in wm), wm
    assert sum(1 for x in wp if x > 0) >= 3, wp
    assert max(len(a) for t in trials[:6] for a in ts.collect_amplicons(t, THR_T, amp_min, amp_max)[1]) > 1200
    assert len(amps) > 64 and len(set(weights)) == 7
    thr = float(np.float32(THR_T) * np.float32(MULT))
    d = api.Screener(0)
    try:
        d.load_texts(seqs, [1.0] * len(seqs))
        d.load_texts(amps, weights, which=api.MULTIPLEX)
        d.select_words(trials + pool, thr, 18)
        comp, mcov, pcov = d.multiplex_screen(trials, pool, background_threshold=BG_THR, use_taq_mama=bool(taq), target_threshold=THR_T,
                                              amp_min=amp_min, amp_max=amp_max)
        assert list(comp) == wc
        assert [float(x) for x in mcov] == wm
        assert [float(x) for x in pcov] == wp
        assert d.num_sequences() == len(seqs) and d.num_sequences(api.MULTIPLEX) == len(amps)
    finally:
        d.close()
