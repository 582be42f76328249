"""The independent expectation for pcr_pool_probe_hits, and the inputs its tests share.

A scenario is products_tm_cases' format with two more keys: probes (one (w0, w1) word or None per pool pair) and optionally
probe_strand.  Its word DB is the one the oracle expects for the pool plus one pair (P, P) per distinct probe.  On that DB
  * the products come from products_tm_cases' machinery over the pool (the join of site_tm_cases.expected_sites by the
    header's rule, or the oracle session's collect_amplicons on a select_words DB or with EOS splits);
  * the probe sites are site_tm_cases.expected_sites for the panel [(P, P) ...] at the probe concentration;
  * the hits are the geometry rule of include/pcramp_hip.h restated in numpy: p3 < probe_loc5 and probe_loc3 < m5 on one
    sequence, p3 = inner_start + 3, m5 = inner_start + inner_length - 8.
Floors, `intended` and `detected` are restated from the definitions.  Nothing here touches the library under test.
"""
import functools
import random

import numpy as np

import products_tm_cases as PC
import site_tm_cases as SC
from select_sites_cases import plant
from site_tm_cases import PLACEMENT_VARIANTS, _primer, _sub, _widen
from testdata import rand_seq, revcomp

HIT = np.dtype([("plus_oligo", np.uint32), ("minus_oligo", np.uint32), ("probe", np.uint32), ("sequence", np.uint32),
                ("begin", np.int32), ("end", np.int32), ("inner_start", np.int32), ("inner_length", np.int32),
                ("probe_loc5", np.int32), ("probe_loc3", np.int32), ("probe_strand", np.uint32), ("intended", np.uint32),
                ("tm_plus", np.float32), ("tm_minus", np.float32), ("tm_probe", np.float32), ("flags", np.uint32)])
ORDER = ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "probe", "probe_loc5", "probe_strand")
PRODUCT_INTENDED, PROBE_INTENDED, PROBE_NO_TM = 1, 2, 4
NO_PROBE = 0xFFFFFFFF
PROBE_STRAND = 2.5e-7


def as_bits(rec):
    """Records -> rows of sixteen uint32: every field, the floats as their bit patterns (the comparison the tests make)."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 16).tolist()


def probe_ids(probes):
    """-> (probe_id list with NO_PROBE for None / (0, 0), distinct probe words in order of first appearance)."""
    ids, words, seen = [], [], {}
    for p in probes:
        w = (0, 0) if p is None else (int(p[0]), int(p[1]))
        if w == (0, 0):
            ids.append(NO_PROBE)
            continue
        if w not in seen:
            seen[w] = len(words)
            words.append(w)
        ids.append(seen[w])
    return ids, words


def db_case(case):
    """The scenario whose word DB the call reads: the pool plus one pair (P, P) per distinct probe."""
    return dict(case, panel=list(case["panel"]) + [(p, p) for p in probe_ids(case["probes"])[1]])


def db_of(oracle, case):
    return SC.db_of(oracle, db_case(case))


_JOBS = {}


@functools.lru_cache(None)
def _everything(oracle, name):
    """-> (oligo_id list, probe_id list, every product as PC.PRODUCT_TM in order, the probes' SITE records, every hit as HIT
    records in order).  Every duplex melted on the way is added to _JOBS[name]."""
    case = scenario(oracle, name)
    entries = db_of(oracle, case)
    amp_min, amp_max = PC.amp_of(case)
    jobs = _JOBS.setdefault(name, set())
    cond = SC.conditions_of(case)
    kw = dict(salt=cond["salt"], template_strand=case.get("template_strand", 0.0), active=case.get("active"),
              seqs=None if case.get("splits") else case["seqs"], jobs=jobs, cache=SC._CACHE)
    ids, sites, _ = SC.expected_sites(oracle, entries, case["panel"], case["thr"], primer_strand=cond["primer_strand"], **kw)
    lens = [len(s) for s in case["seqs"]]
    by_rule = case["select"] == "all" and not case.get("splits")
    pi, mi = PC._pairs_of(sites, lens, amp_min, amp_max, by_rule)
    if not by_rule:
        # the oracle decides which of the candidates are products (as products_tm_cases._all_products, on this DB)
        so = PC._session(oracle, db_case(case))
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
    prod = np.zeros(len(pi), PC.PRODUCT_TM)
    prod["plus_oligo"], prod["minus_oligo"], prod["sequence"] = sites["oligo"][pi], sites["oligo"][mi], sites["sequence"][pi]
    prod["begin"], prod["end"] = sites["loc5"][pi], sites["loc3"][mi]
    prod["inner_start"] = sites["loc3"][pi] + 1 - 4
    prod["inner_length"] = sites["loc5"][mi] - prod["inner_start"] + 8
    pool = {frozenset((ids[2 * i], ids[2 * i + 1])) for i in range(len(case["panel"]))}
    prod["intended"] = [frozenset((int(a), int(b))) in pool for a, b in zip(prod["plus_oligo"], prod["minus_oligo"])]
    prod["tm_plus"], prod["tm_minus"] = sites["tm_max"][pi], sites["tm_max"][mi]
    prod["flags"] = (np.where(sites["flags"][pi] & SC.NO_TM, PC.PLUS_NO_TM, 0) | np.where(sites["flags"][mi] & SC.NO_TM, PC.MINUS_NO_TM, 0))
    prod = prod[np.argsort(prod, order=("plus_oligo", "minus_oligo", "sequence", "begin", "end"), kind="stable")]
    # the probes' sites: the panel (P, P) of the distinct probes, at the probe concentration
    pid, pwords = probe_ids(case["probes"])
    psites = np.zeros(0, SC.SITE)
    if pwords:
        _, psites, _ = SC.expected_sites(oracle, entries, [(p, p) for p in pwords], case["thr"],
                                         primer_strand=case.get("probe_strand", PROBE_STRAND), **kw)
    # the hits: the geometry rule
    assays = {(frozenset((ids[2 * i], ids[2 * i + 1])), pid[i]) for i in range(len(pid)) if pid[i] != NO_PROBE}
    rows = []
    for p in prod:
        p3, m5 = int(p["inner_start"]) + 3, int(p["inner_start"]) + int(p["inner_length"]) - 8
        for s in psites[(psites["sequence"] == p["sequence"]) & (psites["loc5"] > p3) & (psites["loc3"] < m5)]:
            h = np.zeros(1, HIT)
            for f in ("plus_oligo", "minus_oligo", "sequence", "begin", "end", "inner_start", "inner_length", "tm_plus", "tm_minus"):
                h[f] = p[f]
            h["probe"], h["probe_loc5"], h["probe_loc3"], h["probe_strand"] = s["oligo"], s["loc5"], s["loc3"], s["strand"]
            mine = (frozenset((int(p["plus_oligo"]), int(p["minus_oligo"]))), int(s["oligo"])) in assays
            h["intended"] = (PRODUCT_INTENDED if p["intended"] else 0) | (PROBE_INTENDED if mine else 0)
            h["tm_probe"] = s["tm_max"]
            h["flags"] = int(p["flags"]) | (PROBE_NO_TM if s["flags"] & SC.NO_TM else 0)
            rows.append(h)
    hits = np.concatenate(rows) if rows else np.zeros(0, HIT)
    hits = hits[np.argsort(hits, order=ORDER, kind="stable")]
    for a in (prod, psites, hits):
        a.setflags(write=False)
    return ids, pid, prod, psites, hits


def everything(oracle, name):
    return _everything(oracle, name)


def jobs_of(oracle, name):
    """Every (query, target, strand_a, strand_b) the scenario's expectation melted."""
    _everything(oracle, name)
    return _JOBS[name]


def kept(hits, tm_floor, probe_tm_floor):
    """Both floors: tm_floor <= 0 or min(tm_plus, tm_minus) >= tm_floor, and probe_tm_floor <= 0 or tm_probe >= probe_tm_floor."""
    ok = np.ones(len(hits), bool)
    if np.float32(tm_floor) > 0:
        ok &= np.minimum(hits["tm_plus"], hits["tm_minus"]) >= np.float32(tm_floor)
    if np.float32(probe_tm_floor) > 0:
        ok &= hits["tm_probe"] >= np.float32(probe_tm_floor)
    return hits[ok]


def detected_of(hits, prod, ids, pid, n_seq):
    """uint64 [n_pool, ceil(n_seq / 64)] from the kept hits and the kept products, by the definition."""
    n_pool, words = len(pid), (n_seq + 63) // 64
    out = np.zeros((n_pool, words), np.uint64)
    fr, rf = PC.bits_of(prod, ids, n_seq)
    have = {(frozenset((a, b)), q, s) for a, b, q, s in zip(hits["plus_oligo"].tolist(), hits["minus_oligo"].tolist(),
                                                            hits["probe"].tolist(), hits["sequence"].tolist())}
    for i in range(n_pool):
        if pid[i] == NO_PROBE:
            out[i] = fr[i] | rf[i]
            continue
        pair = frozenset((ids[2 * i], ids[2 * i + 1]))
        for s in range(n_seq):
            if (pair, pid[i], s) in have:
                out[i, s >> 6] |= np.uint64(1 << (s & 63))
    return out


def expectation(oracle, name, tm_floor=0.0, probe_tm_floor=0.0):
    """-> (oligo_id list, probe_id list, kept hits, detected) of a scenario at a pair of floors."""
    ids, pid, prod, _, hits = everything(oracle, name)
    k = kept(hits, tm_floor, probe_tm_floor)
    return ids, pid, k, detected_of(k, PC.kept(prod, tm_floor), ids, pid, len(scenario(oracle, name)["seqs"]))


def products_bits(oracle, name, tm_floor=0.0):
    """fr | rf of pcr_pool_products_tm's definition on the scenario's products."""
    ids, _, prod, _, _ = everything(oracle, name)
    fr, rf = PC.bits_of(PC.kept(prod, tm_floor), ids, len(scenario(oracle, name)["seqs"]))
    return fr | rf


def probe_floors_of(hits):
    """As products_tm_cases.floors_of, on tm_probe: the lowest, a middle and the highest positive value, each as itself (>=
    keeps it) and as nextafter above it (drops it); one below all, one above all, and a negative one."""
    v = np.unique(hits["tm_probe"])
    pos = v[v > 0]
    assert len(pos) >= 1
    pick = sorted({float(pos[0]), float(pos[len(pos) // 2]), float(pos[-1])})
    out = []
    for x in pick:
        out += [np.float32(x), np.nextafter(np.float32(x), np.float32(np.inf))]
    out += [np.float32(pos[0]) * np.float32(0.5), np.float32(pos[-1]) + np.float32(5.0), np.float32(-10.0)]
    return [float(f) for f in out]


def floor_pairs(oracle, name):
    """The (tm_floor, probe_tm_floor) pairs the tests use for a scenario: no floor; every probe floor of probe_floors_of alone;
    every product floor of products_tm_cases.floors_of alone (on the products that have a hit); the lowest product value with
    a higher probe value, and a higher product value with the lowest probe value."""
    _, _, prod, _, hits = everything(oracle, name)
    pf = probe_floors_of(hits)
    with_hit = {tuple(r) for r in hits[list(PC.FIELDS8[:5])].tolist()}
    tf = PC.floors_of(prod[[tuple(r) in with_hit for r in prod[list(PC.FIELDS8[:5])].tolist()]])
    out = [(0.0, 0.0)] + [(0.0, f) for f in pf] + [(f, 0.0) for f in tf]
    out += [(tf[0], pf[min(2, len(pf) - 1)]), (tf[min(2, len(tf) - 1)], pf[0])]
    return list(dict.fromkeys(out))


# ---------------------------------------------------------------------------------------------------------------- scenarios
EDGE_F, EDGE_R = 40, 180                        # F (20) at 40: p3 = 59; revcomp(R) (21) at 180: m5 = 180, m3 = 200
EDGE_P3, EDGE_M5 = 59, 180
EDGE_PROBE_LEN = 22
EDGES = dict(plus=0, minus=1, in_plus_side=2, out_plus_side=3, in_minus_side=4, out_minus_side=5, upstream=6, no_probe=7,
             no_product=8, inactive=9)            # what each sequence of the edges scenario holds


@functools.lru_cache(None)
def edges_case(oracle, select="all"):
    """One assay (F, R, P) on ten 300-base sequences, see EDGES.  P begins with F's last base and ends with the first base of
    revcomp(R), so that it can be planted one base into either primer site and leave the site as it is."""
    rng = random.Random(6101)
    f, r = _primer(rng, 20), _primer(rng, 21)
    p = f[-1] + _primer(rng, EDGE_PROBE_LEN - 2) + revcomp(r)[0]
    at = {"plus": (EDGE_F + 60, p), "minus": (EDGE_F + 60, revcomp(p)),
          "in_plus_side": (EDGE_P3 + 1, p), "out_plus_side": (EDGE_P3, p),
          "in_minus_side": (EDGE_M5 - EDGE_PROBE_LEN, p), "out_minus_side": (EDGE_M5 - EDGE_PROBE_LEN + 1, p),
          "upstream": (10, p), "no_probe": None, "no_product": (EDGE_F + 60, p), "inactive": (EDGE_F + 60, p)}
    seqs = [None] * len(EDGES)
    for what, i in EDGES.items():
        s = rand_seq(rng, 300)
        s = plant(s, EDGE_F, f)
        if what != "no_product":
            s = plant(s, EDGE_R, revcomp(r))
        if at[what] is not None:
            s = plant(s, at[what][0], at[what][1])
        assert s[EDGE_F:EDGE_F + 20] == f and (what == "no_product" or s[EDGE_R:EDGE_R + 21] == revcomp(r))
        seqs[i] = s
    w = oracle.centered_word
    active = tuple(i != EDGES["inactive"] for i in range(len(seqs)))
    return dict(seqs=seqs, panel=[(w(f), w(r))], probes=[w(p)], thr=0.95, select=select, active=active)


LADDER_PROBE_AT = (60, 100, 140, 180, 220)
LADDER_AMP = (80, 340)


@functools.lru_cache(None)
def ladder_case(oracle):
    """One assay; a 22-base probe inside its product on sequence 0 in the five PLACEMENT_VARIANTS, the odd ones
    reverse-complemented; sequence 1 holds the product alone."""
    rng = random.Random(6102)
    f, r, p = _primer(rng, 21), _primer(rng, 22), _primer(rng, 22)
    bare = rand_seq(rng, 400)
    bare = plant(bare, 20, f)
    bare = plant(bare, 300, revcomp(r))
    s = bare
    for k, (at, v) in enumerate(zip(LADDER_PROBE_AT, PLACEMENT_VARIANTS)):
        s = plant(s, at, revcomp(_sub(p, v)) if k % 2 else _sub(p, v))
    w = oracle.centered_word
    return dict(seqs=[s, bare], panel=[(w(f), w(r))], probes=[w(p)], thr=float(np.sqrt(np.float32(0.8))), select="all", amp=LADDER_AMP)


CROSS = dict(A=0, B=1, C=2, A_other_probe=3, A_again=4, E_shares_Pa=5, G_equal=6, D_primer_probe=7)   # the pool's rows


@functools.lru_cache(None)
def cross_case(oracle):
    """Eight pool pairs, see CROSS: A (Fa, Ra, Pa); B (Fb, Rb, Pb); C without a probe; A with Pb; A again; E with A's probe;
    G with F = R; D whose probe word is the primer Fa.  Sequence 1 holds B's product with Pb AND Pa inside; sequence 6 A's
    product without any probe site; sequence 5 nothing."""
    rng = random.Random(6103)
    fa, ra, fb, rb, fc, rc, fe, re_, fg, fd, rd = (_primer(rng, n) for n in (20, 21, 20, 22, 21, 20, 20, 21, 22, 20, 21))
    pa, pb, pg = (_primer(rng, n) for n in (24, 22, 23))
    layout = (((40, fa), (100, pa), (180, revcomp(ra))),
              ((40, fb), (90, pb), (130, pa), (180, revcomp(rb))),
              ((40, fc), (180, revcomp(rc)), (260, fa), (320, pb), (400, revcomp(ra))),
              ((40, fe), (100, revcomp(pa)), (180, revcomp(re_)), (260, fg), (320, pg), (400, revcomp(fg))),
              ((40, fd), (100, fa), (180, revcomp(rd))),
              (),
              ((40, fa), (180, revcomp(ra))))
    seqs = []
    for sites in layout:
        s = rand_seq(rng, 520)
        for at, text in sites:
            s = plant(s, at, text)
        seqs.append(s)
    w = oracle.centered_word
    Fa, Ra, Pa, Pb = w(fa), w(ra), w(pa), w(pb)
    panel = [(Fa, Ra), (w(fb), w(rb)), (w(fc), w(rc)), (Fa, Ra), (Fa, Ra), (w(fe), w(re_)), (w(fg), w(fg)), (w(fd), w(rd))]
    probes = [Pa, Pb, None, Pb, Pa, Pa, w(pg), Fa]
    return dict(seqs=seqs, panel=panel, probes=probes, thr=0.95, select="all")


WORDS_PROBE_AT = 110
WORDS_NO_PROBE_SITE = tuple(i for i in range(PC.WORDS_N - 1) if i % 7 == 5)     # a product and no probe site
WORDS_BLOCK_PROBES = (179, 199, 219)            # three sites of pair 0's probe between the block's plus and minus sites


@functools.lru_cache(None)
def words_case(oracle):
    """products_tm_cases.words_case with a 19-base probe per pair: inside the product of every sequence except every seventh,
    and three times inside the 64 products of the last sequence (192 hits on one sequence, one bit)."""
    base = PC.words_case(oracle)
    rng = random.Random(6104)
    pr = [_primer(rng, 19) for _ in range(3)]
    seqs = list(base["seqs"])
    for i in range(PC.WORDS_N - 1):
        if i in PC.WORDS_NO_SITE or i in WORDS_NO_PROBE_SITE:
            continue
        seqs[i] = plant(seqs[i], WORDS_PROBE_AT, pr[i % 3] if i % 2 else revcomp(pr[i % 3]))
    for at in WORDS_BLOCK_PROBES:
        seqs[PC.WORDS_BLOCK] = plant(seqs[PC.WORDS_BLOCK], at, pr[0])
    w = oracle.centered_word
    return dict(base, seqs=seqs, probes=[w(p) for p in pr])


@functools.lru_cache(None)
def degenerate_case(oracle):
    """The plus-strand sequence and the no-probe sequence of the edges scenario, the probe widened to 4 expansions."""
    rng = random.Random(6105)
    f, r, p = _primer(rng, 20), _primer(rng, 21), _primer(rng, 22)
    seqs = []
    for with_probe in (True, False):
        s = rand_seq(rng, 300)
        s = plant(s, EDGE_F, f)
        s = plant(s, EDGE_R, revcomp(r))
        if with_probe:
            s = plant(s, EDGE_F + 60, p)
        seqs.append(s)
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(f), w(r))], probes=[w(_widen(p, (4, 13), "R"))], thr=0.95, select="all")


@functools.lru_cache(None)
def ambiguity_case(oracle):
    """A product with two sites of its probe inside: one with an N under it (PROBE_NO_TM), one exact; the same product with
    only the N site (sequence 1) and alone (sequence 2)."""
    rng = random.Random(6106)
    f, r, p = _primer(rng, 20), _primer(rng, 21), _primer(rng, 22)
    bare = rand_seq(rng, 300)
    bare = plant(bare, EDGE_F, f)
    bare = plant(bare, EDGE_R, revcomp(r))
    only_n = plant(bare, 70, p[:9] + "N" + p[10:])
    s = plant(only_n, 120, p)
    w = oracle.centered_word
    return dict(seqs=[s, only_n, bare], panel=[(w(f), w(r))], probes=[w(p)], thr=0.95, select="all")


SPLIT_PROBE_AT = 150


@functools.lru_cache(None)
def split_case(oracle):
    """products_tm_cases.split_inner_case (an EOS at 200, inside the inner stretch of sequence 0's product) with a probe at 150
    of both sequences: sequence 0 holds the probe site and no product, sequence 1 the hit; sequence 2 is sequence 1 as it was."""
    base = PC.split_inner_case(oracle)
    rng = random.Random(6108)                   # (a probe whose best sites on sequence 2, 13 of 22 slots, lie outside the product)
    p = _primer(rng, 22)
    seqs = [plant(s, SPLIT_PROBE_AT, p) for s in base["seqs"]] + [base["seqs"][1]]
    return dict(base, seqs=seqs, probes=[oracle.centered_word(p)])


OFFSET_PRIMER_LEN, OFFSET_PROBE_LEN = 18, 14


def _word_at(oracle, text, first_slot):
    """The word holding `text` in slots first_slot .. first_slot + len(text) - 1 (site_tm_cases.slots_of's layout, inverted)."""
    code = {b: v for v, b in SC.BASE.items()}
    w = [0, 0]
    for k, b in enumerate(text, first_slot):
        w[k >> 4] |= code[b] << ((15 - (k & 15)) * 4)
    assert SC.spell(SC.slots_of(w)) == text and oracle.word_start(tuple(w)) == first_slot
    return (w[0], w[1])


@functools.lru_cache(None)
def offset_case(oracle):
    """Words that are not centred: both primers in slots 0 .. 17 of their words, the probe (14 bases) in slots 18 .. 31.  On
    sequence 0 the probe follows F's 3' base at once, so its site is read from the SAME 32-base window as F's: the probe's
    DB entry is the plus primer's, not one between the two primers' entries.  On sequence 1 the reverse-complemented probe
    ends one base before R's site begins: its entry is the minus primer's.  Sequence 2 holds the product alone."""
    rng = random.Random(6109)
    f, r, p = _primer(rng, OFFSET_PRIMER_LEN), _primer(rng, OFFSET_PRIMER_LEN), _primer(rng, OFFSET_PROBE_LEN)
    bare = rand_seq(rng, 300)
    bare = plant(bare, EDGE_F, f)
    bare = plant(bare, EDGE_R, revcomp(r))
    seqs = [plant(bare, EDGE_F + OFFSET_PRIMER_LEN, p), plant(bare, EDGE_R - OFFSET_PROBE_LEN, revcomp(p)), bare]
    return dict(seqs=seqs, panel=[(_word_at(oracle, f, 0), _word_at(oracle, r, 0))], probes=[_word_at(oracle, p, 18)], thr=0.95,
                select="all")


SCENARIO_NAMES = ("edges", "ladder", "cross", "words", "degenerate", "ambiguity", "words_db", "split", "offset")
_MAKERS = {"edges": edges_case, "offset": offset_case, "ladder": ladder_case, "cross": cross_case, "words": words_case, "degenerate": degenerate_case,
           "ambiguity": ambiguity_case, "words_db": lambda oracle: edges_case(oracle, "words"), "split": split_case}
_CASES = {}


def register(name, case):
    _CASES[name] = case
    return name


def scenario(oracle, name):
    if name not in _CASES:
        _CASES[name] = _MAKERS[name](oracle)
    return _CASES[name]
