"""The independent expectation for pcr_site_tm, and the inputs its tests share.

expected_sites() restates the call's definition (include/pcramp_hip.h) from a list of word-DB entries the CPU oracle produced
(Sequence::pack through select_sites_cases, or an oracle session where the input has EOS splits), a Python restatement of the
target rule on the (w0, w1) words, oracle.word_expand and oracle.heterodimer_full.  Where a site's entry is a full window of
a sequence it also cuts the target from the sequence text and asserts that both spellings agree.  Nothing here touches the
library under test.
"""
import functools
import random

import numpy as np

from select_sites_cases import argmax_filter, expected_entries, floor_of, plant, word_and_np
from testdata import family_targets, mutate, rand_seq, revcomp, sample_pair

SITE = np.dtype([("oligo", np.uint32), ("sequence", np.uint32), ("loc5", np.int32), ("loc3", np.int32),
                 ("strand", np.uint32), ("matches", np.uint32), ("n_expansions", np.uint32), ("flags", np.uint32),
                 ("tm_max", np.float32), ("tm_min", np.float32), ("dH", np.float32), ("dS", np.float32)])
NO_TM = 1
SALT, PRIMER_STRAND = 0.05, 9e-7
BASE = {1: "A", 2: "C", 4: "G", 8: "T"}
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
SQ = lambda t: float(np.float32(t) * np.float32(t))


def slots_of(w):
    """The 32 slot nibbles of a word (word.cpp:11-16: slot k is nibble 15 - k % 16 of block k / 16)."""
    return [(int(w[k >> 4]) >> ((15 - (k & 15)) * 4)) & 0xF for k in range(32)]


def planes_of(sl):
    """Slot masks (A, C, G, T): the tie-break key among entries sharing a site."""
    return tuple(sum(((v >> b) & 1) << k for k, v in enumerate(sl)) for b in range(4))


def spell(sl):
    return "".join(BASE[v] for v in sl if v)


def distinct_oligos(panel):
    """ids in order of first appearance -> (oligo_id list over F0, R0, F1, R1, ..., distinct words)."""
    ids, words, seen = [], [], {}
    for f, r in panel:
        for w in ((int(f[0]), int(f[1])), (int(r[0]), int(r[1]))):
            if w not in seen:
                seen[w] = len(words)
                words.append(w)
            ids.append(seen[w])
    return ids, words


def target_of(entry_slots, start, stop):
    """The target rule: slots start - 1 .. stop + 1 clipped to the word, empty ends dropped; None where a slot left is empty
    or ambiguous; else (complement of the bases, highest slot first; lowest slot; highest slot)."""
    lo, hi = max(start - 1, 0), min(stop + 1, 31)
    while lo <= hi and not entry_slots[lo]:
        lo += 1
    while hi >= lo and not entry_slots[hi]:
        hi -= 1
    if lo > hi:
        return None
    if any(entry_slots[k] not in BASE for k in range(lo, hi + 1)):
        return None
    return "".join(COMP[BASE[entry_slots[k]]] for k in range(hi, lo - 1, -1)), lo, hi


def occupied_in_window(entry_slots, start, stop):
    return sum(1 for k in range(max(start - 1, 0), min(stop + 1, 31) + 1) if entry_slots[k])


def strand_rule(ca, cb):
    """NucCruc::strand(a, b), nuc_cruc.h:832-837, in float32."""
    ca, cb = np.float32(ca), np.float32(cb)
    return ca - np.float32(0.5) * cb if ca > cb else cb - np.float32(0.5) * ca


def melt_cached(oracle, cache, key, salt):
    """oracle.heterodimer_full of key = (query, target, strand_a, strand_b) at a salt, kept in cache under (salt,) + key."""
    k = (float(salt),) + key
    if k not in cache:
        cache[k] = oracle.heterodimer_full(key[0], key[1], salt, key[2], key[3])
    return cache[k]


def expected_sites(oracle, entries, panel, thr, salt=SALT, primer_strand=PRIMER_STRAND, template_strand=0.0, active=None,
                   seqs=None, jobs=None, cache=None, tamper=None):
    """-> (oligo_id list, SITE array sorted by (oligo, sequence, loc5, strand), number of (site, expansion) jobs).
    entries: the word DB as sorted (w0, w1, loc, index, strand) tuples.  seqs: the sequence texts, for the second spelling of
    full-window targets (leave None where the sequences were split).  jobs: a set that receives every
    (query, target, strand_a, strand_b) the thermodynamics were asked for.  cache: {(salt, query, target, a, b): result}.
    tamper(oligo id, expansions) -> the expansions melted in their place: what a wrong decode of the expansion index would
    report (tests/test_melt_conditions_host.py asks whether the records could tell)."""
    ids, words = distinct_oligos(panel)
    cache = {} if cache is None else cache
    thr2 = np.float32(thr) * np.float32(thr)
    w0 = np.array([e[0] for e in entries], dtype=np.uint64)
    w1 = np.array([e[1] for e in entries], dtype=np.uint64)
    rows, n_jobs = [], 0
    for oid, c in enumerate(words):
        csl = slots_of(c)
        start, stop = oracle.word_start(c), oracle.word_stop(c)
        exps = [spell(slots_of(x)) for x in oracle.word_expand(c)]
        degen = oracle.word_degeneracy(c)
        assert len(exps) == int(degen)
        if tamper is not None:
            exps = tamper(oid, exps)
        ca = np.float32(float(np.float32(primer_strand)) / degen)
        cb = np.float32(template_strand)
        hit = np.nonzero(word_and_np(c, w0, w1) >= floor_of(c, thr2))[0] if len(entries) else []
        sites = {}
        for i in hit:
            _, _, loc, index, strand = entries[i]
            if strand not in (1, 2) or (active is not None and not active[index]):
                continue
            sites.setdefault((index, loc, strand), []).append(entries[i])
        for (index, loc, strand), group in sites.items():
            esl = [slots_of(e) for e in group]
            most = max(occupied_in_window(s, start, stop) for s in esl)
            sl = min((s for s in esl if occupied_in_window(s, start, stop) == most), key=planes_of)
            rec = np.zeros(1, SITE)
            rec["oligo"], rec["sequence"], rec["strand"] = oid, index, strand
            rec["loc5"] = loc + start if strand == 1 else loc - stop
            rec["loc3"] = loc + stop if strand == 1 else loc - start
            rec["matches"] = sum(1 for a, b in zip(sl, csl) if a & b)
            rec["n_expansions"] = len(exps)
            n_jobs += len(exps)
            tgt = target_of(sl, start, stop)
            if tgt is None:
                rec["flags"] = NO_TM
            else:
                target, lo, hi = tgt
                if seqs is not None and all(sl):             # a full window: the same target from the sequence text
                    text = seqs[index]
                    cut = revcomp(text[loc + lo:loc + hi + 1]) if strand == 1 else text[loc - hi:loc - lo + 1]
                    assert cut == target, (index, loc, strand, cut, target)
                res = []
                for q in exps:
                    key = (q, target, float(ca), float(cb))
                    res.append(melt_cached(oracle, cache, key, salt))
                    if jobs is not None:
                        jobs.add(key)
                tms = [r[0] for r in res]
                best = max(range(len(res)), key=lambda k: (tms[k], -k))     # the highest Tm, the lowest index on a tie
                rec["tm_max"], rec["tm_min"] = tms[best], min(tms)
                rec["dH"], rec["dS"] = res[best][1], res[best][2]
            rows.append(rec)
    out = np.concatenate(rows) if rows else np.zeros(0, SITE)
    out = out[np.argsort(out, order=("oligo", "sequence", "loc5", "strand"), kind="stable")]
    return ids, out, n_jobs


def as_bits(rec):
    """Records -> tuples with every float as its bit pattern (the comparison the tests make)."""
    f = lambda x: int(np.float32(x).view(np.uint32))
    return [(int(r["oligo"]), int(r["sequence"]), int(r["loc5"]), int(r["loc3"]), int(r["strand"]), int(r["matches"]),
             int(r["n_expansions"]), int(r["flags"]), f(r["tm_max"]), f(r["tm_min"]), f(r["dH"]), f(r["dS"])) for r in rec]


# ---------------------------------------------------------------------------------------------------------------- scenarios
# A scenario: dict(seqs, panel, thr, select ("all": select_sites, "words": select_words at thr squared), and optionally
# active, splits [(sequence, position)], template_strand, salt, primer_strand -- SALT and PRIMER_STRAND where it has none).
# db_of() gives the word DB the oracle expects for it.

_SUB = {"A": "C", "C": "A", "G": "T", "T": "G"}


def _primer(rng, n):
    while True:
        s = rand_seq(rng, n)
        if all(s[j:j + 4] != s[j] * 4 for j in range(n - 3)):
            return s


def _sub(s, places):
    out = list(s)
    for p in places:
        out[p] = _SUB[out[p]]
    return "".join(out)


def db_of(oracle, case):
    thr2 = SQ(case["thr"])
    active = case.get("active")
    if case.get("splits"):
        assert case["select"] == "words"
        so = oracle.session()
        for i, s in enumerate(case["seqs"]):
            so.add_target(s, 1.0, True if active is None else bool(active[i]))
        for s, p in case["splits"]:
            so.split(s, p)
        so.select(case["panel"], thr2)
        return so.db_entries()
    entries = expected_entries(oracle, case["seqs"], case["panel"], thr2, active=active)
    if case["select"] == "words":
        entries = argmax_filter(entries, case["panel"], thr2)
    return entries


_CACHE = {}


def conditions_of(case):
    """The salt and the primer concentration a scenario is melted at: its own keys, or the defaults."""
    return dict(salt=case.get("salt", SALT), primer_strand=case.get("primer_strand", PRIMER_STRAND))


def expectation(oracle, case, jobs=None, **kw):
    """expected_sites() of a scenario on the DB db_of() gives; the thermodynamic results are shared between calls."""
    args = dict(conditions_of(case), template_strand=case.get("template_strand", 0.0), active=case.get("active"),
                seqs=None if case.get("splits") else case["seqs"])
    args.update(kw)
    return expected_sites(oracle, db_of(oracle, case), case["panel"], case["thr"], jobs=jobs, cache=_CACHE, **args)


PLACEMENT_PLUS = (8, 36, 64, 92, 120)          # where the five variants sit as the oligo spells them (strand 1 sites)
PLACEMENT_MINUS = (150, 178, 206, 234, 262)    # ... and reverse-complemented (strand 2 sites)
PLACEMENT_VARIANTS = ((), (10,), (19,), (0, 1), (3, 9, 15))   # exact, middle, 3' base, two at the 5' end, three


@functools.lru_cache(None)
def placement_case(oracle, select="all"):
    """1. One 300-base sequence holding a 20-mer's site in five variants on each strand."""
    rng = random.Random(4101)
    p = _primer(rng, 20)
    s = rand_seq(rng, 300)
    for at, v in zip(PLACEMENT_PLUS, PLACEMENT_VARIANTS):
        s = plant(s, at, _sub(p, v))
    for at, v in zip(PLACEMENT_MINUS, PLACEMENT_VARIANTS):
        s = plant(s, at, revcomp(_sub(p, v)))
    other = _primer(rng, 21)
    w = oracle.centered_word
    return dict(seqs=[s], panel=[(w(p), w(other))], thr=float(np.sqrt(np.float32(0.8))), select=select)


@functools.lru_cache(None)
def ends_case(oracle):
    """2. Sites at base 0, ending at the last base (tail partial words), hanging over the end by 2 bases; oligos of 18, 25,
    30, 31 and 32 bases; sequences of 34, 35 and 77 bases.  Floor 0.85."""
    rng = random.Random(4102)
    a, b, c = rand_seq(rng, 77), rand_seq(rng, 35), rand_seq(rng, 34)
    w = oracle.centered_word
    hang = c[4:34] + _SUB[c[0]] + _SUB[c[1]]            # 32-mer: 30 bases of the tail, then 2 past the end
    panel = [(w(a[0:18]), w(revcomp(a[52:77]))), (w(a[47:77]), w(b[2:33])), (w(revcomp(b[1:33])), w(hang))]
    return dict(seqs=[c, b, a], panel=panel, thr=float(np.sqrt(np.float32(0.85))), select="all")


@functools.lru_cache(None)
def ambiguity_case(oracle):
    """3a. An N inside a site, an R on a site's flank slot, and exact copies of both oligos beside them."""
    rng = random.Random(4103)
    q1, q2 = _primer(rng, 22), _primer(rng, 21)
    s = rand_seq(rng, 600)
    s = plant(s, 50, q1[:9] + "N" + q1[10:])
    s = plant(s, 150, q1)
    s = plant(s, 299, "R" + revcomp(q2))                # q2's minus site; the slot after its 3' end holds R
    s = plant(s, 400, revcomp(q2))
    w = oracle.centered_word
    return dict(seqs=[s], panel=[(w(q1), w(q2))], thr=0.95, select="all")


@functools.lru_cache(None)
def split_case(oracle):
    """3b. A site straddling an EOS split (sequence 0) and the same site whole (sequence 1); the DB of select_words.
    Word::push_back writes the next base over an EOS (word.cpp:32-41), so the words over a split have no hole: they join the
    bases on either side, and the straddling site is a weaker site that is melted as its word spells it."""
    rng = random.Random(4104)
    q, r = _primer(rng, 22), _primer(rng, 20)
    seqs = []
    for _ in range(2):
        s = rand_seq(rng, 500)
        s = plant(s, 100, q)
        s = plant(s, 300, revcomp(r))
        seqs.append(s)
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(q), w(r))], thr=0.75, select="words", splits=[(0, 110)])


def _widen(s, places, code):
    holds = {"R": "AG", "Y": "CT", "N": "ACGT"}
    out = list(s)
    for p in places:
        out[p] = code if code == "N" else ("R" if out[p] in "AG" else "Y")
        assert s[p] in holds[out[p]]
    return "".join(out)


@functools.lru_cache(None)
def expansions_case(oracle, template_strand=0.0):
    """4. Oligos with 2, 4, 16 and 256 expansions on their exact sites, and a two-fold degenerate oligo whose degenerate
    5' base and the base after it both face a mismatch: the best alignment leaves the degenerate base unpaired."""
    rng = random.Random(4105)
    t = [_primer(rng, 22) for _ in range(5)]
    s = rand_seq(rng, 700)
    for k, x in enumerate(t):
        s = plant(s, 60 + 120 * k, x if k % 2 == 0 else revcomp(x))
    tie_site = t[4]
    first = "R" if tie_site[0] in "CT" else "Y"          # neither base of the code is the template's
    tie = first + _SUB[tie_site[1]] + tie_site[2:]
    txt = [_widen(t[0], (7,), "R"), _widen(t[1], (3, 15), "R"), _widen(t[2], (2, 8, 13, 19), "R"), _widen(t[3], (4, 9, 12, 17), "N"),
           tie, t[4]]
    w = oracle.centered_word
    return dict(seqs=[s], panel=[(w(txt[0]), w(txt[1])), (w(txt[2]), w(txt[3])), (w(txt[4]), w(txt[5]))],
                thr=float(np.sqrt(np.float32(0.8))), select="all", template_strand=template_strand)


def too_degenerate_oligo(oracle):
    """512 expansions."""
    return oracle.centered_word("ACGTNNNNRACGTACGTACG")


@functools.lru_cache(None)
def ids_case(oracle):
    """5. F of pair 0 is R of pair 2; sequence 1 is inactive."""
    rng = random.Random(4106)
    f0, r0, f1, r1, f2 = (_primer(rng, n) for n in (20, 21, 22, 20, 19))
    seqs = []
    for i in range(3):
        s = rand_seq(rng, 900 + 11 * i)
        s = plant(s, 100, f0)
        s = plant(s, 220, revcomp(r0))
        s = plant(s, 400, f1)
        s = plant(s, 530, revcomp(r1))
        s = plant(s, 650, f2)
        s = plant(s, 760, revcomp(f0))
        seqs.append(s)
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(f0), w(r0)), (w(f1), w(r1)), (w(f2), w(f0))], thr=0.9, select="all",
                active=(True, False, True))


GRID_SITES = 301


@functools.lru_cache(None)
def grid_case(oracle):
    """7. One sequence with the same site 301 times, a two-fold degenerate oligo: 602 jobs; and an oligo with one site."""
    rng = random.Random(4107)
    site, once, gap = _primer(rng, 22), _primer(rng, 21), rand_seq(rng, 9)
    s = (gap + site) * GRID_SITES + gap + once + gap
    w = oracle.centered_word
    return dict(seqs=[s], panel=[(w(_widen(site, (11,), "R")), w(once))], thr=1.0, select="all")


def grid_single(oracle):
    case = dict(grid_case(oracle))
    case["panel"] = [(case["panel"][0][1], case["panel"][0][1])]
    return case


STRIDE_SITES = 16


@functools.lru_cache(None)
def stride_case(oracle):
    """7b. More jobs than a grid capped at one 12-wave block per CU holds in one stride: a 256-expansion oligo on 16 copies of
    its site = 4 096 jobs (3 072 is a stride on 256 CUs), of few distinct duplexes."""
    rng = random.Random(4109)
    site, once, gap = _primer(rng, 22), _primer(rng, 21), rand_seq(rng, 9)
    s = (gap + site) * STRIDE_SITES + gap + once + gap
    w = oracle.centered_word
    return dict(seqs=[s], panel=[(w(_widen(site, (4, 9, 12, 17), "N")), w(once))], thr=1.0, select="all")


@functools.lru_cache(None)
def zero_tie_case(oracle):
    """4b. A two-fold degenerate 20-mer on a site with 8 substitutions: both expansions melt below 0 C, so both Tm are clamped
    to 0 and tie, with different dH and dS -- the record must carry those of expansion 0 (the lowest index wins a tie)."""
    rng = random.Random(5000)
    p = _primer(rng, 20)
    site = _sub(p, rng.sample([i for i in range(20) if i != 10], 8))
    s = plant(rand_seq(rng, 200), 90, site)
    other = _primer(rng, 21)
    w = oracle.centered_word
    return dict(seqs=[s], panel=[(w(_widen(p, (10,), "R")), w(other))], thr=0.75, select="all")


def zero_tie_expansions(oracle, case):
    """The two expansions' (tm, dH, dS) on the planted site's target, in expansion order."""
    _, rec, _ = expectation(oracle, case)
    c = case["panel"][0][0]
    exps = [spell(slots_of(x)) for x in oracle.word_expand(c)]
    text = case["seqs"][0]
    target = revcomp(text[89:111])                       # the 20 bases at 90 and one flank on either side
    ca = float(np.float32(float(np.float32(PRIMER_STRAND)) / 2.0))
    return [oracle.heterodimer_full(q, target, SALT, ca, 0.0) for q in exps]


@functools.lru_cache(None)
def random_case(oracle):
    """8. 8 sequences x 2 kb in two mutated families, 6 pairs sampled from them (two with IUPAC bases), every site at
    float32(0.75) squared."""
    rng = random.Random(4108)
    seqs = family_targets(rng, 2, 4, 2000, div=0.04)
    txt = []
    while len(txt) < 6:
        p = sample_pair(rng, rng.choice(seqs))
        if p:
            txt.append(p)
    txt[1] = (_widen(txt[1][0], (5,), "R"), _widen(txt[1][1], (3, 11), "R"))
    txt[4] = (_widen(txt[4][0], (8,), "R"), txt[4][1])
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(f), w(r)) for f, r in txt], thr=0.75, select="all")


def gpu_scenarios(oracle):
    """name -> scenario, every scenario tests/test_gpu_site_tm.py melts."""
    out = {"placement": placement_case(oracle), "placement_words": placement_case(oracle, "words"), "ends": ends_case(oracle),
           "ambiguity": ambiguity_case(oracle), "split": split_case(oracle), "ids": ids_case(oracle), "grid": grid_case(oracle),
           "grid_single": grid_single(oracle), "random": random_case(oracle), "stride": stride_case(oracle),
           "zero_tie": zero_tie_case(oracle)}
    for k, ts in enumerate(TEMPLATE_STRANDS):
        out["expansions_%d" % k] = expansions_case(oracle, ts)
    return out


TEMPLATE_STRANDS = (0.0, PRIMER_STRAND, 10 * PRIMER_STRAND)
SCENARIO_NAMES = ("placement", "placement_words", "ends", "ambiguity", "split", "ids", "grid", "grid_single", "random",
                  "expansions_0", "expansions_1", "expansions_2", "stride", "zero_tie")
