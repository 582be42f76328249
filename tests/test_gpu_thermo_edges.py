"""thermo::k_thermo_wave at the edges of its input space, against the CPU oracle (pinned to the reference on the same inputs by
tests/test_thermo_cases_host.py): oligos of 1..11 and 31..32 nt, dimers with sides of 1..32 nt, every filter threshold placed on
the computed value, the 16 MiB switch of the job upload, and the validity form (pcr_valid_words: the path of the local search's
trial words) verdict by verdict, expansion by expansion and record by record.  Values are compared as float32 bits; every test
prints how many it compared."""
import functools
import random

import numpy as np
import pytest

import thermo_cases as TC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu
SALT, STRAND = 0.05, 9e-7
NARROW = dict(tm_min=45.0, tm_max=70.0, max_hairpin=35.0)
OPEN = dict(tm_min=-1.0, tm_max=1.0e9, max_hairpin=1.0e9, max_dimer=1.0e9)       # no Tm is below 0 (evaluate() clamps)


@pytest.fixture(scope="module")
def dev():
    s = api.Screener(0)
    yield s
    s.close()


def f32(x):
    return np.float32(x)


def same_bits(a, b):
    return f32(a).view(np.uint32) == f32(b).view(np.uint32)


def up(x):
    return float(np.nextafter(f32(x), f32(np.inf)))


def down(x):
    return float(np.nextafter(f32(x), f32(-np.inf)))


def window_ok(o, check_homo_dimer, tm_min=50.0, tm_max=75.0, max_hairpin=40.0, max_dimer=40.0):
    """valid_pcr.cpp:19-41 on one expansion's oracle values."""
    ok = not (o[0] < f32(tm_min) or o[0] > f32(tm_max)) and not (o[4] > f32(max_hairpin))
    return ok and not (check_homo_dimer and o[7] > f32(max_dimer))


def centered(text):
    return TC.word_at(text, (33 - len(text)) // 2)


# ------------------------------------------------------------------------------------------------ oligos
def test_short_and_full_oligos(dev, oracle):
    seqs = TC.short_oligos()
    words = [centered(s) for s in seqs]
    want = [oracle.thermo_full(s, SALT, STRAND) for s in seqs]
    exact = tot = 0
    for chk in (True, False):
        res = dev.is_valid(words, chk)
        for s, r, o in zip(seqs, res, want):
            got = [r["tm"], r["dH"], r["dS"], r["dG"], r["hairpin_tm"], r["homodimer_tm"]]
            exp = [o[0], o[1], o[2], o[3], o[4], o[7] if chk else f32(0.0)]
            same = [bool(same_bits(g, w)) for g, w in zip(got, exp)]
            exact += sum(same); tot += len(same)
            assert all(same), (s, chk, got, exp)
            assert r["n"] == 1 and r["valid"] == window_ok(o, chk), (s, chk)
            tot += 1; exact += 1
    print("short and full oligos: %d of %d values bit-identical (%d oligos, with and without the homodimer test)" % (exact, tot, len(seqs)))
    assert exact == tot and tot == 2 * 7 * len(seqs)


# ------------------------------------------------------------------------------------------------ dimers
def test_dimers_of_full_and_lopsided_sizes(dev, oracle):
    texts = TC.dimer_pairs()
    pairs = [(centered(a), centered(b)) for a, b in texts]
    swapped = [(b, a) for a, b in pairs]
    exact = tot = nz = 0
    for batch in (pairs, swapped):
        got = dev.max_dimer_tm(batch)
        for p, t, g in zip(batch, texts, got):
            w = oracle.max_dimer_tm(p)
            assert same_bits(g, w), (t, batch is swapped, g, w)
            exact += 1; tot += 1; nz += int(w > 0)
    assert nz >= len(pairs) // 2                                          # (a quarter of the pairs, both ways round)
    n = len(pairs)
    other = [pairs[(7 * i + 3) % n] for i in range(n)]
    verdicts = set()
    for md in (10.0, 25.0, 40.0):
        ok = dev.multiplex_compatible(pairs, other, max_dimer=md)
        for x, y, g in zip(pairs, other, ok):
            w = oracle.multiplex_compatible(x, y, max_dimer=md)
            assert int(g) == w, (x, y, md)
            exact += 1; tot += 1; verdicts.add(w)
    assert verdicts == {0, 1}
    print("dimers: %d of %d values identical (%d max_dimer_tm as float bits, %d of them above zero; %d multiplex verdicts)"
          % (exact, tot, 2 * n, nz, 3 * n))
    assert exact == tot


def test_dimers_of_unequal_degeneracy(dev, oracle):
    """1 x 4, 4 x 1, 2 x 3, 3 x 2 expansions: both branches of the strand term ca > cb ? ca - cb/2 : cb - ca/2."""
    pairs = list(TC.unequal_pairs())
    got = dev.max_dimer_tm(pairs)
    n = nz = 0
    for p, g in zip(pairs, got):
        w = oracle.max_dimer_tm(p)
        assert same_bits(g, w), (p, g, w)
        n += 1; nz += int(w > 0)
    assert 2 * nz >= len(pairs)
    other = pairs[1:] + pairs[:1]
    for md in (10.0, 25.0, 40.0):
        for x, y, g in zip(pairs, other, dev.multiplex_compatible(pairs, other, max_dimer=md)):
            assert int(g) == oracle.multiplex_compatible(x, y, max_dimer=md), (x, y, md)
            n += 1
    print("dimers of unequal degeneracy: %d of %d values identical (%d max_dimer_tm as float bits, %d above zero)" % (n, n, len(pairs), nz))


# ------------------------------------------------------------------------------------------------ thresholds
@functools.lru_cache(maxsize=None)
def threshold_oligos():
    from oracle_lib import Oracle
    orc = Oracle()
    out = []
    for s in TC.threshold_candidates():
        o = orc.thermo_full(s, SALT, STRAND)
        if o[0] > 0 and o[4] > 0 and o[7] > 0:
            out.append((s, o))
        if len(out) == 200:
            break
    return out


def test_is_valid_thresholds_on_the_value(dev, oracle):
    """Each bound at the oracle's float, one float below and one above, the others wide open: `<`, `>` and `>` of
    valid_pcr.cpp:19-41 -- a value equal to its bound passes."""
    oligos = threshold_oligos()
    assert len(oligos) == 200
    # bound -> (index of the value in thermo_full, verdicts at (value, below, above))
    plan = {"tm_min": (0, (True, True, False)), "tm_max": (0, (True, False, True)),
            "max_hairpin": (4, (True, False, True)), "max_dimer": (7, (True, False, True))}
    n = 0
    for s, o in oligos:
        w = centered(s)
        for bound, (idx, expect) in plan.items():
            v = float(o[idx])
            for thr, exp in zip((v, down(v), up(v)), expect):
                kw = dict(OPEN); kw[bound] = thr
                got = bool(dev.is_valid([w], True, flags=True, **kw)[0])
                assert got == bool(oracle.is_valid(w, check_homo_dimer=True, **kw)) and got == exp, (s, bound, thr, v, got)
                n += 1
    print("is_valid thresholds: %d of %d verdicts identical" % (n, n))
    assert n == 200 * 4 * 3


def test_multiplex_compatible_threshold_on_the_value(dev, oracle):
    """max_dimer at the highest of the four heterodimer Tm of two assays: `>=` of pcr_assay.cpp:841 rejects at equality."""
    oligos = threshold_oligos()
    c = float(f32(STRAND))
    n = 0
    for k in range(0, 200, 2):
        a = (oligos[k][0], oligos[k + 1][0])
        b = (TC.revcomp(oligos[(k + 7) % 200][0])[2:], oligos[(k + 12) % 200][0])
        # multiplex_compatible melts at strand = primer_strand (no degeneracy or two-strand correction): 2c - c/2*2 = c exactly
        worst = max(float(oracle.heterodimer_full(q, s, SALT, 2 * c, 2 * c)[0]) for q in a for s in b)
        if not worst > 0:
            continue
        x, y = (centered(a[0]), centered(a[1])), (centered(b[0]), centered(b[1]))
        for md, exp in ((worst, False), (down(worst), False), (up(worst), True)):
            want = oracle.multiplex_compatible(x, y, max_dimer=md)
            got = bool(dev.multiplex_compatible([x], [y], max_dimer=md)[0])
            assert got == bool(want) and got == exp, (a, b, md, worst, got, want)
            n += 1
    print("multiplex_compatible thresholds: %d of %d verdicts identical" % (n, n))
    assert n >= 3 * 80


# ------------------------------------------------------------------------------------------------ 16 MiB of job records
def test_job_records_above_16_mib(dev, oracle):
    """240 000 jobs of 72 bytes: the records go to the device by a copy instead of through the mapped input buffer."""
    rng = random.Random(7106)
    seqs = [TC.rand_seq(rng, 12) if k % 3 else "".join(rng.choice("GGCCAT") for _ in range(12)) for k in range(1200)]
    words = [centered(s) for s in seqs]
    k = 200
    assert len(words) * k * 72 > (16 << 20)
    full = dev.is_valid(words, False)
    n = 0
    for s, r in list(zip(seqs, full))[::25]:
        o = oracle.thermo_full(s, SALT, STRAND)
        got, exp = [r["tm"], r["dH"], r["dS"], r["hairpin_tm"]], [o[0], o[1], o[2], o[4]]
        assert all(same_bits(g, w) for g, w in zip(got, exp)), (s, got, exp)
        n += 4
    for kw in (dict(), dict(tm_min=38.0)):
        small = dev.is_valid(words, False, flags=True, **kw)
        big = dev.is_valid(words * k, False, flags=True, **kw)
        assert big.shape == (1200 * k,) and np.array_equal(np.tile(small, k), big)
        for s, w, g in list(zip(seqs, words, small))[::25]:
            assert bool(g) == bool(oracle.is_valid(w, check_homo_dimer=False, **kw)), (s, kw)
            n += 1
        if kw:
            assert 100 < int(small.sum()) < 1100                              # both verdicts, so a tile out of place shows
    print("above 16 MiB: 2 x %d verdicts equal the small call's, %d of %d sampled values identical to the oracle's" % (1200 * k, n, n))


# ------------------------------------------------------------------------------------------------ the validity form
def test_valid_words_verdicts(dev, oracle):
    words = list(TC.degenerate_words())
    n = 0
    for kw in (dict(), NARROW):
        got = dev.valid_words(words, **kw)
        plain = dev.is_valid(words, False, flags=True, **kw)                   # expansions spelt on the host, a result per expansion
        want = np.array([oracle.is_valid(w, check_homo_dimer=False, **kw) for w in words])
        assert set(want.tolist()) <= {0, 1}
        bad = [W.word_text(w) for w, g, p, x in zip(words, got, plain, want) if not (bool(g) == bool(p) == bool(x))]
        assert not bad, (kw, bad)
        n += 2 * len(words)
        if kw:
            assert int(want.sum()) >= 5 and int((1 - want).sum()) >= 5
    print("validity form, verdicts: %d of %d identical (%d words, two windows, against the oracle and the plain form)" % (n, n, len(words)))


@functools.lru_cache(maxsize=None)
def expansion_values(text):
    """-> (tm, hairpin Tm) float32 arrays over TC.expand(text), at is_valid's strand = primer_strand / degeneracy."""
    from oracle_lib import Oracle
    orc = Oracle()
    strand = float(f32(float(f32(STRAND)) / TC.degeneracy(text)))
    vals = [orc.thermo_full(e, SALT, strand) for e in TC.expand(text)]
    return np.array([v[0] for v in vals], np.float32), np.array([v[4] for v in vals], np.float32)


def test_valid_words_visit_every_expansion(dev, oracle):
    """A bound between the two most extreme expansions must fail the word, the bound on the most extreme one must pass it:
    the verdict then hangs on ONE expansion, wherever the mixed-radix decode puts it."""
    separable = n = 0
    for text in TC.degenerate_texts():
        assert TC.degeneracy(text) <= 4096
        tm, hp = expansion_values(text)
        hi, lo, hh = np.sort(tm)[::-1], np.sort(tm), np.sort(hp)[::-1]
        cases = []
        if float(hi[0]) - float(hi[1]) > 1e-3:
            cases.append(("tm_max", float(f32((float(hi[0]) + float(hi[1])) / 2)), float(hi[0])))
        if float(lo[1]) - float(lo[0]) > 1e-3:
            cases.append(("tm_min", float(f32((float(lo[0]) + float(lo[1])) / 2)), float(lo[0])))
        if float(hh[0]) - float(hh[1]) > 1e-3:
            cases.append(("max_hairpin", float(f32((float(hh[0]) + float(hh[1])) / 2)), float(hh[0])))
        for first in TC.positions(len(text)):
            w = TC.word_at(text, first)
            for bound, between, on in cases:
                for thr, exp in ((between, False), (on, True)):
                    kw = dict(tm_min=-1.0, tm_max=1.0e9, max_hairpin=1.0e9); kw[bound] = thr
                    got = bool(dev.valid_words([w], **kw)[0])
                    assert got == exp and got == bool(oracle.is_valid(w, check_homo_dimer=False, **kw)), (text, first, bound, thr, got)
                    n += 1
                separable += 1
    print("validity form, every expansion: %d (word, bound) combinations separable, %d of %d verdicts identical" % (separable, n, n))
    assert separable >= 20


def test_valid_words_records_do_not_leak(dev, oracle):
    rng = random.Random(7107)
    big = [w for w in TC.degenerate_words() if oracle.word_degeneracy(w) == TC.BIG_TEXT_DEGENERACY]
    assert big
    plain = [centered(TC.rand_seq(rng, rng.randint(16, 26))) for _ in range(600)]
    batch = big[:1] + plain + list(TC.degenerate_words())
    assert sum(int(oracle.word_degeneracy(w)) for w in batch) > 4 * 256 * 12   # more jobs than waves resident on any GPU of the family
    want = np.array([bool(oracle.is_valid(w, check_homo_dimer=False, **NARROW)) for w in batch])
    assert 50 < int(want.sum()) < len(batch) - 50
    base = dev.valid_words(batch, **NARROW)
    assert np.array_equal(base, want)
    n = len(batch)
    for seed in (1, 2, 3):
        perm = list(range(len(batch)))
        random.Random(seed).shuffle(perm)
        got = dev.valid_words([batch[i] for i in perm], **NARROW)
        assert np.array_equal(got, want[perm]), seed
        n += len(batch)
    words = list(TC.degenerate_words())
    tenfold = dev.valid_words(words * 10, **NARROW).reshape(10, len(words))
    assert (tenfold == tenfold[0]).all() and np.array_equal(tenfold[0], want[1 + len(plain):])
    n += tenfold.size
    print("validity form, records: %d of %d verdicts identical (three permutations, every word ten times)" % (n, n))


def test_valid_words_errors(dev, oracle):
    good = centered("AGAAGGCTCGCCAAAATAAACG")
    for bad in ((0, 0), W.word_from_slots([0] * 8 + [1, 2, 0, 4, 8] + [0] * 19), centered("ACGTNNNNNNNNNACGTACG")):
        with pytest.raises(api.PcrError):
            dev.valid_words([good, bad])
        kw = dict(tm_min=55.0)
        assert dev.valid_words([good], **kw).tolist() == [bool(oracle.is_valid(good, check_homo_dimer=False, **kw))] == [True]
        assert dev.valid_words([good], tm_min=60.0).tolist() == [False]
    assert dev.valid_words([]).shape == (0,)
