"""The independent expectation for pcr_pool_products_tm, and the inputs its tests share.

The sites come from site_tm_cases.expected_sites (the oracle's word DB, the target rule restated in Python, oracle.word_expand
and oracle.heterodimer_full).  The products are
  * on an all-sites DB: the join of those site records by the rule written in include/pcramp_hip.h -- p3 < m5,
    amp_min <= m3 - p5 + 1 <= amp_max, the inner stretch inside the sequence (these scenarios have no EOS);
  * on a select_words DB or with EOS splits: what the oracle session's collect_amplicons reports for every pair of distinct
    oligos (the comparison tests/test_gpu_pool_products.py::_check_oracle makes), each bound attributed to the orientation
    whose two site records stand at its begin and end.
Floor and bitsets are restated from the definition on those records.  Nothing here touches the library under test.
"""
import functools
import random

import numpy as np

import site_tm_cases as SC
from select_sites_cases import plant
from site_tm_cases import PLACEMENT_VARIANTS, SQ, _primer, _sub
from testdata import rand_seq, revcomp

PRODUCT_TM = np.dtype([("plus_oligo", np.uint32), ("minus_oligo", np.uint32), ("sequence", np.uint32), ("begin", np.int32),
                       ("end", np.int32), ("inner_start", np.int32), ("inner_length", np.int32), ("intended", np.uint32),
                       ("tm_plus", np.float32), ("tm_minus", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])
PLUS_NO_TM, MINUS_NO_TM = 1, 2
FIELDS8 = ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "inner_start", "inner_length", "intended")
AMP = (80, 200)


def amp_of(case):
    return case.get("amp", AMP)


def as_bits(rec):
    """Records -> rows of twelve uint32: every field, the floats as their bit patterns (the comparison the tests make)."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 12).tolist()


def _session(oracle, case):
    """An oracle session holding the scenario's DB (asserted to be the one db_of() expects)."""
    active = case.get("active")
    so = oracle.session()
    for i, s in enumerate(case["seqs"]):
        so.add_target(s, 1.0, True if active is None else bool(active[i]))
    for s, p in case.get("splits", ()):
        so.split(s, p)
    so.select(case["panel"], SQ(case["thr"]))
    assert so.db_entries() == SC.db_of(oracle, case)
    return so


def _pairs_of(sites, lens, amp_min, amp_max, by_rule):
    """Every (plus site, minus site) on one sequence -> index arrays (into sites) of the pairs the header's rule admits
    (by_rule), or of all pairs with the plus site's 3' end before the minus site's 5' end."""
    pi, mi = [], []
    plus = np.nonzero(sites["strand"] == 1)[0]
    minus = np.nonzero(sites["strand"] == 2)[0]
    for s in np.unique(sites["sequence"][plus]):
        P = plus[sites["sequence"][plus] == s]
        M = minus[sites["sequence"][minus] == s]
        if not len(M):
            continue
        p5, p3 = sites["loc5"][P].astype(np.int64)[:, None], sites["loc3"][P].astype(np.int64)[:, None]
        m5, m3 = sites["loc5"][M].astype(np.int64)[None, :], sites["loc3"][M].astype(np.int64)[None, :]
        ok = p3 < m5
        if by_rule:
            n = m3 - p5 + 1
            in_start = p3 + 1 - 4
            in_len = m5 - in_start + 8
            ok = ok & (n >= amp_min) & (n <= amp_max) & (in_start >= 0) & (in_len >= 0) & (in_start + in_len <= int(lens[s]))
        a, b = np.nonzero(ok)
        pi.append(P[a])
        mi.append(M[b])
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(pi), cat(mi)


@functools.lru_cache(None)
def _all_products(oracle, key):
    case = scenario(oracle, key)
    amp_min, amp_max = amp_of(case)
    ids, sites, n_jobs = SC.expectation(oracle, case)
    lens = [len(s) for s in case["seqs"]]
    by_rule = case["select"] == "all" and not case.get("splits")
    pi, mi = _pairs_of(sites, lens, amp_min, amp_max, by_rule)
    if not by_rule:
        # the oracle decides which of the candidates are products
        so = _session(oracle, case)
        _, words = SC.distinct_oligos(case["panel"])
        admitted = set()
        for a in range(len(words)):
            for b in range(a, len(words)):
                bo, _ = so.collect_amplicons((words[a], words[b]), case["thr"], amp_min, amp_max)
                for s, bg, e in bo:
                    admitted.add((min(a, b), max(a, b), s, bg, e))
        x, y = sites["oligo"][pi].astype(np.int64), sites["oligo"][mi].astype(np.int64)
        cand = list(zip(np.minimum(x, y).tolist(), np.maximum(x, y).tolist(), sites["sequence"][pi].tolist(),
                        (sites["loc5"][pi].astype(np.int64) & 0xFFFFFFFF).tolist(), sites["loc3"][mi].tolist()))
        keep = np.array([c in admitted for c in cand], bool)
        assert admitted <= set(cand), "an amplicon of the oracle has no pair of site records"
        pi, mi = pi[keep], mi[keep]
    rec = np.zeros(len(pi), PRODUCT_TM)
    rec["plus_oligo"], rec["minus_oligo"], rec["sequence"] = sites["oligo"][pi], sites["oligo"][mi], sites["sequence"][pi]
    rec["begin"], rec["end"] = sites["loc5"][pi], sites["loc3"][mi]
    rec["inner_start"] = sites["loc3"][pi] + 1 - 4
    rec["inner_length"] = sites["loc5"][mi] - rec["inner_start"] + 8
    pool = {frozenset((ids[2 * i], ids[2 * i + 1])) for i in range(len(case["panel"]))}
    rec["intended"] = [frozenset((int(a), int(b))) in pool for a, b in zip(rec["plus_oligo"], rec["minus_oligo"])]
    rec["tm_plus"], rec["tm_minus"] = sites["tm_max"][pi], sites["tm_max"][mi]
    rec["flags"] = (np.where(sites["flags"][pi] & SC.NO_TM, PLUS_NO_TM, 0) | np.where(sites["flags"][mi] & SC.NO_TM, MINUS_NO_TM, 0))
    rec = rec[np.argsort(rec, order=("plus_oligo", "minus_oligo", "sequence", "begin", "end"), kind="stable")]
    rec.setflags(write=False)
    return ids, rec, sites, n_jobs


_CASES = {}


def register(name, case):
    _CASES[name] = case
    return name


def all_products(oracle, name):
    """-> (oligo_id list, every product of the scenario as PRODUCT_TM records in order, the site records, job count)."""
    return _all_products(oracle, name)


def min_tm(rec):
    return np.minimum(rec["tm_plus"], rec["tm_minus"])


def kept(rec, tm_floor):
    """The floor: tm_floor <= 0, or min(tm_plus, tm_minus) >= tm_floor in float."""
    if not (np.float32(tm_floor) > 0):
        return rec
    return rec[min_tm(rec) >= np.float32(tm_floor)]


def bits_of(rec, ids, n_seq):
    """(fr, rf): uint64 [n_pool, ceil(n_seq / 64)] from the kept records, by the definition."""
    n_pool, words = len(ids) // 2, (n_seq + 63) // 64
    fr, rf = np.zeros((n_pool, words), np.uint64), np.zeros((n_pool, words), np.uint64)
    have = set(zip(rec["plus_oligo"].tolist(), rec["minus_oligo"].tolist(), rec["sequence"].tolist()))
    for i in range(n_pool):
        f, r = ids[2 * i], ids[2 * i + 1]
        for s in range(n_seq):
            if (f, r, s) in have:
                fr[i, s >> 6] |= np.uint64(1 << (s & 63))
            if (r, f, s) in have:
                rf[i, s >> 6] |= np.uint64(1 << (s & 63))
    return fr, rf


def expectation(oracle, name, tm_floor=0.0):
    """-> (oligo_id list, kept records, fr, rf) of a scenario at a floor."""
    ids, rec, _, _ = all_products(oracle, name)
    k = kept(rec, tm_floor)
    fr, rf = bits_of(k, ids, len(scenario(oracle, name)["seqs"]))
    return ids, k, fr, rf


def floors_of(rec):
    """The floors the tests use for a scenario: from the sorted distinct min-Tm values v -- the lowest, a middle and the
    highest positive one, each as itself (>= keeps it) and as nextafter above it (drops it); one below all, one above all,
    and a negative one."""
    v = np.unique(min_tm(rec))
    pos = v[v > 0]
    assert len(pos) >= 1
    pick = sorted({float(pos[0]), float(pos[len(pos) // 2]), float(pos[-1])})
    out = []
    for x in pick:
        out += [np.float32(x), np.nextafter(np.float32(x), np.float32(np.inf))]
    out += [np.float32(pos[0]) * np.float32(0.5), np.float32(pos[-1]) + np.float32(5.0), np.float32(-10.0)]
    return [float(f) for f in out]


# ---------------------------------------------------------------------------------------------------------------- scenarios
# site_tm_cases' format, with an optional amp = (amp_min, amp_max); the call's default elsewhere.

LADDER_PLUS = (10, 38, 66, 94, 122)
LADDER_MINUS = (200, 228, 256, 284, 312)
LADDER_AMP = (80, 340)


@functools.lru_cache(None)
def ladder_case(oracle):
    """One pair (F, R), a 21- and a 22-mer.  Sequence 0 (400 bases) holds five variants of F's plus site and five of R's minus
    site (PLACEMENT_VARIANTS), every one of the 25 combinations within 80..340.  Sequence 1 holds only the weakest plus and
    the weakest minus variant, sequence 2 only the strongest of each (by the oracle's Tm: a substitution at an end can melt
    above the exact site) -- each copied from sequence 0 with two flanking bases, so that the duplexes are the same ones."""
    rng = random.Random(5201)
    f, r = _primer(rng, 21), _primer(rng, 22)
    s0 = rand_seq(rng, 400)
    for at, v in zip(LADDER_PLUS, PLACEMENT_VARIANTS):
        s0 = plant(s0, at, _sub(f, v))
    for at, v in zip(LADDER_MINUS, PLACEMENT_VARIANTS):
        s0 = plant(s0, at, revcomp(_sub(r, v)))
    w = oracle.centered_word
    panel = [(w(f), w(r))]
    thr = float(np.sqrt(np.float32(0.8)))
    _, sites, _ = SC.expected_sites(oracle, SC.db_of(oracle, dict(seqs=[s0], panel=panel, thr=thr, select="all")), panel, thr,
                                    seqs=[s0], cache=SC._CACHE)
    tm_at = lambda strand, at: float(sites[(sites["strand"] == strand) & (sites["loc5"] == at)]["tm_max"][0])
    weak_p = min(LADDER_PLUS, key=lambda at: tm_at(1, at))
    weak_m = min(LADDER_MINUS, key=lambda at: tm_at(2, at))
    seqs = [s0]
    strong_p = max(LADDER_PLUS, key=lambda at: tm_at(1, at))
    strong_m = max(LADDER_MINUS, key=lambda at: tm_at(2, at))
    for p_at, m_at in ((weak_p, weak_m), (strong_p, strong_m)):
        s = rand_seq(rng, 400)
        s = plant(s, 48, s0[p_at - 2:p_at + len(f) + 2])
        s = plant(s, 198, s0[m_at - 2:m_at + len(r) + 2])
        seqs.append(s)
    return dict(seqs=seqs, panel=panel, thr=thr, select="all", amp=LADDER_AMP)


WORDS_N = 131
WORDS_INACTIVE = (7, 65)
WORDS_NO_SITE = (20, 100)
WORDS_MUTATED = (3, 64, 90)
WORDS_BLOCK = 130                                # the sequence with the repeated site block: 8 x 8 products of pair 0
WORDS_AMP = (80, 420)


@functools.lru_cache(None)
def words_case(oracle):
    """131 sequences of 300 bases (the last one 460), three pairs; sequence i holds one intended product of pair i % 3.  Three
    of them have a substitution in the minus site (the weaker of the two), two are inactive, two hold no site at all, and the last holds eight plus and
    eight minus sites of pair 0: 64 intended products on one sequence, one bit.  Bits land in three u64 words."""
    rng = random.Random(5202)
    pr = [(_primer(rng, 20), _primer(rng, 21)) for _ in range(3)]
    seqs = []
    for i in range(WORDS_N - 1):
        f, r = pr[i % 3]
        s = rand_seq(rng, 300)
        if i not in WORDS_NO_SITE:
            s = plant(s, 60, f)
            s = plant(s, 190, revcomp(_sub(r, (9,)) if i in WORDS_MUTATED else r))
        seqs.append(s)
    f, r = pr[0]
    s = rand_seq(rng, 460)
    for k in range(8):
        s = plant(s, 10 + 21 * k, f)
        s = plant(s, 238 + 22 * k, revcomp(r))
    seqs.append(s)
    w = oracle.centered_word
    active = tuple(i not in WORDS_INACTIVE for i in range(WORDS_N))
    return dict(seqs=seqs, panel=[(w(f), w(r)) for f, r in pr], thr=0.95, select="all", active=active, amp=WORDS_AMP)


@functools.lru_cache(None)
def pairs_case(oracle):
    """A pool (A, B), (C, C), (A, D), (A, B) again, (B, A): a duplicated pair, a pair with F = R, pairs sharing an oligo, and a
    pair that is another one exchanged.  Four sequences hold products of some of them; the last holds none."""
    rng = random.Random(5203)
    a, b, c, d = (_primer(rng, n) for n in (20, 21, 22, 20))
    seqs = []
    for sites in (((50, a), (170, revcomp(b)), (300, c), (420, revcomp(c))),
                  ((60, a), (190, revcomp(d))),
                  ((40, b), (150, revcomp(a)), (300, a), (410, revcomp(b)), (440, revcomp(d))),
                  ((100, c), (230, revcomp(c)), (350, d))):
        s = rand_seq(rng, 520)
        for at, text in sites:
            s = plant(s, at, text)
        seqs.append(s)
    seqs.append(rand_seq(rng, 520))
    w = oracle.centered_word
    A, B, C_, D = w(a), w(b), w(c), w(d)
    return dict(seqs=seqs, panel=[(A, B), (C_, C_), (A, D), (A, B), (B, A)], thr=0.95, select="all")


SPLIT_AMP = (80, 260)                            # split_case's sites stand 220 bases apart: no product at 80..200


def split_wide_case(oracle):
    """site_tm_cases.split_case at 80..260: the whole copy's product on sequence 1, and on sequence 0 the products of the
    weaker sites the words over the split at 110 are (the split is outside their inner stretch)."""
    return dict(SC.split_case(oracle), amp=SPLIT_AMP)


def split_inner_case(oracle):
    """The same sequences split at 200, between the two sites: the EOS is inside the inner stretch, sequence 0 has no product."""
    return dict(SC.split_case(oracle), splits=[(0, 200)], amp=SPLIT_AMP)


NEW_SCENARIOS = ("ladder", "words", "pairs", "split_wide", "split_inner")
SITE_SCENARIOS = ("placement", "placement_words", "ids", "ambiguity", "split", "expansions_0", "expansions_1", "expansions_2", "random")
SCENARIO_NAMES = NEW_SCENARIOS + SITE_SCENARIOS
FLOOR_SCENARIOS = ("ladder", "ids", "random")


def scenario(oracle, name):
    """name -> scenario (registered for all_products / expectation)."""
    if name not in _CASES:
        if name in NEW_SCENARIOS:
            register(name, {"ladder": ladder_case, "words": words_case, "pairs": pairs_case, "split_wide": split_wide_case,
                            "split_inner": split_inner_case}[name](oracle))
        else:
            register(name, SC.gpu_scenarios(oracle)[name])
    return _CASES[name]
