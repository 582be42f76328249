"""The independent expectation for pcr_pool_products_end3, and the inputs its tests share.

expected() starts from products_tm_cases.all_products (the oracle's word DB and duplex Tm, the join restated in Python) and
annotates every site from the DB entry site_tm_cases' pick rule chooses: a slot matches iff oracle.word_and of the oligo's and
the entry's one-slot words is 1, the TaqMAMA factor is oracle.taq_mama of the four nibbles, every float is a numpy float32
product in the order the header gives.  Then the rule, restated.  Nothing here touches the library under test.

ends_case departs from its description in one number: sequence 0 is 1 660 bases long, not 400.  Seven 3'-end variants and the
5'-end variant of each of three forward and three reverse oligos (18 to 32 bases) are 48 sites that do not overlap; they do not
fit into 400 bases.  Its amplicon range (80, 1 700) admits every plus x minus combination on it.
"""
import functools
import random

import numpy as np

import products_tm_cases as PT
import site_tm_cases as SC
import site_variant_cases as SV
from oracle_lib import Oracle  # noqa: F401  (the fixtures hand one in; imported so that a missing oracle fails here)
from select_sites_cases import floor_of, plant, word_and_np
from site_tm_cases import PLACEMENT_VARIANTS, SQ, _primer, _sub, occupied_in_window, planes_of, slots_of
from testdata import rand_seq, revcomp

PRODUCT_END3 = np.dtype(PT.PRODUCT_TM.descr + [("clamp3_plus", np.uint8), ("clamp3_minus", np.uint8),
                                               ("end_mismatch_plus", np.uint8), ("end_mismatch_minus", np.uint8),
                                               ("id_plus", np.float32), ("id_minus", np.float32), ("reserved2", np.uint32)])
assert PRODUCT_END3.itemsize == 64

ZERO_RULE = dict(min_clamp3=0, window=0, max_end_mismatch=0, use_taq_mama=0, ident_threshold=0.0)
CLAMPS = (0, 1, 2, 3, 6, 32)
WINDOWS = ((0, 0), (1, 0), (5, 0), (5, 1), (32, 0))


def rule_of(**kw):
    r = dict(ZERO_RULE)
    r.update(kw)
    return r


def rule_grid():
    return [rule_of(min_clamp3=c, window=w, max_end_mismatch=m) for c in CLAMPS for w, m in WINDOWS]


def is_trivial(rule):
    return rule["min_clamp3"] == 0 and rule["window"] == 0 and rule["ident_threshold"] == 0.0


def as_bits(rec):
    """Records -> rows of sixteen uint32: every byte, the floats as their bit patterns."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 16).tolist()


def slot_word(v, k):
    """The word holding the nibble v in slot k and nothing else (word.cpp:11-16)."""
    w = [0, 0]
    w[k >> 4] = int(v) << ((15 - (k & 15)) * 4)
    return tuple(w)


# ---------------------------------------------------------------------------------------------------------------- the sites
@functools.lru_cache(None)
def _site_ends(oracle, name, use_taq):
    """(oligo, sequence, strand, loc5) -> dict(length, matches, miss: mismatch flags from the 3' slot downwards, clamp3, factor,
    id, hang: the entry's slot under the oligo's last base is empty, t1 / t2: the entry's nibbles under the last two bases)."""
    case = PT.scenario(oracle, name)
    entries = SC.db_of(oracle, case)
    active = case.get("active")
    _, words = SC.distinct_oligos(case["panel"])
    thr2 = np.float32(case["thr"]) * np.float32(case["thr"])
    w0 = np.array([e[0] for e in entries], dtype=np.uint64)
    w1 = np.array([e[1] for e in entries], dtype=np.uint64)
    out = {}
    for oid, c in enumerate(words):
        csl = slots_of(c)
        start, stop = oracle.word_start(c), oracle.word_stop(c)
        length = stop - start + 1
        assert length == oracle.word_size(c)
        norm = np.float32(1.0 / length)                                      # float(1.0 / length): a double quotient, rounded once
        hit = np.nonzero(word_and_np(c, w0, w1) >= floor_of(c, thr2))[0] if len(entries) else []
        sites = {}
        for i in hit:
            _, _, loc, index, strand = entries[i]
            if strand not in (1, 2) or (active is not None and not active[index]):
                continue
            sites.setdefault((index, loc, strand), []).append(entries[i])
        for (index, loc, strand), group in sites.items():
            esl = [slots_of(e) for e in group]                               # site_tm_cases' pick: most occupied in the window, lowest masks
            most = max(occupied_in_window(s, start, stop) for s in esl)
            sl = min((s for s in esl if occupied_in_window(s, start, stop) == most), key=planes_of)
            match = [oracle.word_and(slot_word(csl[k], k), slot_word(sl[k], k)) == 1 for k in range(start, stop + 1)]
            matches = sum(match)
            assert matches == oracle.word_and(c, SV.word_of_slots(sl))
            miss = [not ok for ok in reversed(match)]                        # index d: the slot d below the 3' end
            factor = np.float32(1.0)
            p1, p2 = (csl[stop - 1] if stop >= 1 else 0), csl[stop]
            t1, t2 = (sl[stop - 1] if stop >= 1 else 0), sl[stop]
            one = lambda v: v in (1, 2, 4, 8)
            if use_taq and one(p1) and one(p2) and one(t1) and one(t2):
                factor = np.float32(oracle.taq_mama(p1, p2, t1, t2))
                assert factor <= np.float32(1.0)
            ident = np.float32(matches) * norm
            if use_taq:
                ident = np.float32(ident * factor)
            loc5 = loc + start if strand == 1 else loc - stop
            out[(oid, index, strand, loc5)] = dict(length=length, matches=matches, miss=miss, factor=factor, id=np.float32(ident),
                                                   clamp3=next((d for d, bad in enumerate(miss) if bad), length),
                                                   hang=sl[stop] == 0, t1=t1, t2=t2)
    return out


def site_ends(oracle, name, use_taq=0):
    return _site_ends(oracle, name, int(bool(use_taq)))


def end_mismatch(site, window):
    return sum(site["miss"][:min(window, site["length"])])


def site_ok(site, rule):
    if site["clamp3"] < min(rule["min_clamp3"], site["length"]):
        return False
    return not (rule["window"] > 0 and end_mismatch(site, rule["window"]) > rule["max_end_mismatch"])


def score_of(a, b):
    """sqrtf(__fmul_rn(id_plus, id_minus)): a float32 product, its correctly rounded float32 root."""
    return np.sqrt(np.float32(np.float32(a) * np.float32(b)), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------- the records
def products_before_rule(oracle, name, tm_floor=0.0, thermo=True):
    """products_tm_cases' records past the floor, minus those whose inner stretch holds one of the scenario's EOS splits; without
    thermodynamics both Tm and the flags are 0 (and there is no floor)."""
    case = PT.scenario(oracle, name)
    ids, rec, sites, _ = PT.all_products(oracle, name)
    rec = rec.copy()
    for s, p in case.get("eos", ()):
        cut = (rec["sequence"] == s) & (rec["inner_start"] <= p) & (p < rec["inner_start"].astype(np.int64) + rec["inner_length"])
        assert cut.any(), "the split is inside no product"
        rec = rec[~cut]
    if thermo:
        rec = PT.kept(rec, tm_floor).copy()
    else:
        assert not (tm_floor > 0)
        rec["tm_plus"] = rec["tm_minus"] = 0
        rec["flags"] = 0
    return ids, rec, sites


def expected(oracle, name, rule, tm_floor=0.0, thermo=True):
    """-> (oligo_id list, kept PRODUCT_END3 records in order, fr, rf, n_before_rule)."""
    case = PT.scenario(oracle, name)
    ids, rec, sites = products_before_rule(oracle, name, tm_floor, thermo)
    ends = site_ends(oracle, name, rule["use_taq_mama"])
    len_of = {}
    for (oid, _, _, _), e in ends.items():
        len_of[oid] = e["length"]
    out = np.zeros(len(rec), PRODUCT_END3)
    keep = np.zeros(len(rec), bool)
    for f in PT.PRODUCT_TM.names:
        out[f] = rec[f]
    thr = np.float32(rule["ident_threshold"])
    for i, r in enumerate(rec):
        p = ends[(int(r["plus_oligo"]), int(r["sequence"]), 1, int(r["begin"]))]
        minus5 = int(r["end"]) - (len_of[int(r["minus_oligo"])] - 1)           # a minus site: loc5 = loc3 - (length - 1)
        m = ends[(int(r["minus_oligo"]), int(r["sequence"]), 2, minus5)]
        out["clamp3_plus"][i], out["clamp3_minus"][i] = p["clamp3"], m["clamp3"]
        out["end_mismatch_plus"][i], out["end_mismatch_minus"][i] = end_mismatch(p, rule["window"]), end_mismatch(m, rule["window"])
        out["id_plus"][i], out["id_minus"][i] = p["id"], m["id"]
        keep[i] = site_ok(p, rule) and site_ok(m, rule) and (thr == 0 or score_of(p["id"], m["id"]) >= thr)
    kept = out[keep]
    fr, rf = PT.bits_of(kept, ids, len(case["seqs"]))
    return ids, kept, fr, rf, len(rec)


# ---------------------------------------------------------------------------------------------------------------- ends_case
ENDS_AMP = (80, 1700)
ENDS_PLUS_AT, ENDS_PLUS_STEP = 10, 30
ENDS_MINUS_AT, ENDS_MINUS_STEP = 760, 36
ENDS_SPLIT = (2, 310)


def end_variants(n):
    """Where an n-mer's planted sites are substituted: the exact site, one substitution at distance 0 .. 5 from the 3' end, and
    PLACEMENT_VARIANTS' two at the 5' end."""
    five = [v for v in PLACEMENT_VARIANTS if v and max(v) <= 1]
    assert five == [(0, 1)]
    return [()] + [(n - 1 - d,) for d in range(6)] + five


def _two_fold_last(s):
    return s[:-1] + ("R" if s[-1] in "AG" else "Y")


@functools.lru_cache(None)
def ends_case(oracle):
    """Three pairs: a 20 / 22-mer, an 18 / 25-mer, and a 21-mer whose last base is a two-fold code with a 32-mer (slots 0 and 31).
    Sequence 0: every forward oligo's plus site and every reverse oligo's minus site in the eight end_variants, all plus x
    minus combinations inside ENDS_AMP.  Sequence 1: a minus site of the 22-mer whose 3' base hangs over the start and a plus site
    of the 21-mer whose 3' base hangs over the end (irregular words, the empty slot under `stop`; the partial words Sequence::pack
    emits at an end are centred, which is why a 20-mer cannot hang by one base there), an exact product between them, and a plus
    site of the 18-mer with substitutions under its second and fourth base from the 3' end.
    Sequence 2: the 20-mer's plus site with R and N in the template under its second-last and last base (PCR_SITE_NO_TM, slots
    that match by IUPAC, a TaqMAMA factor of 1) and its product; a plus site of the 32-mer whose 5' base hangs over the start (an
    empty slot that is a mismatch in a record: clamp3 31 of 32); an exact product of the second pair with an EOS split at 310
    inside it.  Sequence 3 holds an exact product and is inactive."""
    rng = random.Random(6101)
    fa, ra, fb, rb, fc, rc = (_primer(rng, n) for n in (20, 22, 18, 25, 21, 32))
    s0 = rand_seq(rng, 1660)
    k = 0
    for f in (fa, fb, fc):
        for v in end_variants(len(f)):
            s0 = plant(s0, ENDS_PLUS_AT + ENDS_PLUS_STEP * k, _sub(f, v))
            k += 1
    k = 0
    for r in (ra, rb, rc):
        for v in end_variants(len(r)):
            s0 = plant(s0, ENDS_MINUS_AT + ENDS_MINUS_STEP * k, revcomp(_sub(r, v)))
            k += 1
    s1 = rand_seq(rng, 400)
    s1 = plant(s1, 0, revcomp(ra)[1:])
    s1 = plant(s1, 100, fa)
    s1 = plant(s1, 160, _sub(fb, (len(fb) - 2, len(fb) - 4)))                # two mismatches inside a window of 5: what (5, 1) drops
    s1 = plant(s1, 230, revcomp(ra))
    s1 = plant(s1, 400 - 20, fc[:20])
    s2 = rand_seq(rng, 400)
    s2 = plant(s2, 0, rc[1:])
    s2 = plant(s2, 60, fa[:18] + ("R" if fa[18] in "AG" else "Y") + "N")
    s2 = plant(s2, 190, revcomp(ra))
    s2 = plant(s2, 250, fb)
    s2 = plant(s2, 360, revcomp(rb))
    s3 = rand_seq(rng, 400)
    s3 = plant(s3, 50, fa)
    s3 = plant(s3, 180, revcomp(ra))
    w = oracle.centered_word
    panel = [(w(fa), w(ra)), (w(fb), w(rb)), (w(_two_fold_last(fc)), w(rc))]
    return dict(seqs=[s0, s1, s2, s3], panel=panel, thr=float(np.sqrt(np.float32(0.8))), select="all",
                active=(True, True, True, False), amp=ENDS_AMP, eos=[ENDS_SPLIT])


# ---------------------------------------------------------------------------------------------------------------- taq_case
DINUCS = tuple(a + b for a in "ACGT" for b in "ACGT")
TAQ_AMP = (80, 200)
TAQ_F_AT, TAQ_R_AT = 60, 180
TAQ_BASE_THR = 0.93                              # the lowest threshold the tests use: 17 of 20 slots


@functools.lru_cache(None)
def taq_case(oracle, thr=TAQ_BASE_THR):
    """Sixteen pairs: one 18-base body followed by each of the 16 dinucleotides, all with one common 21-mer R.  Sixteen sequences
    of 300 bases: sequence j spells the body and dinucleotide j at 60 and the exact R site 120 bases downstream."""
    rng = random.Random(6102)
    while True:
        body, r = _primer(rng, 18), _primer(rng, 21)
        if all(all((body + d)[j:j + 4] != (body + d)[j] * 4 for j in range(17)) for d in DINUCS):
            break
    seqs = []
    for d in DINUCS:
        s = rand_seq(rng, 300)
        s = plant(s, TAQ_F_AT, body + d)
        s = plant(s, TAQ_R_AT, revcomp(r))
        seqs.append(s)
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(body + d), w(r)) for d in DINUCS], thr=float(thr), select="all", amp=TAQ_AMP)


def taq_thresholds():
    """The identity thresholds of the TaqMAMA tests (each also the pool threshold of its call, as find_target_match collects and
    tests at one threshold): 0.96 separates one mismatch from two without the factor; the scores of 19 and of 18 matching slots
    of 20 beside an exact R, each with the float32 below and above it; 1.0 -- the exact cells' score, exactly representable --
    and the float32 below it; and two scores only the factor makes: 18/20 and 19/20 times 0.989 and 0.978."""
    out = [np.float32(0.96)]
    up, down = np.float32(np.inf), np.float32(-np.inf)
    twentieth = np.float32(1.0 / 20)
    for s in (score_of(np.float32(19) * twentieth, 1.0), score_of(np.float32(18) * twentieth, 1.0),
              score_of(np.float32(np.float32(19) * twentieth) * np.float32(0.989), 1.0),
              score_of(np.float32(np.float32(19) * twentieth) * np.float32(0.978), 1.0)):
        out += [np.nextafter(s, down), s, np.nextafter(s, up)]
    out += [np.nextafter(np.float32(1.0), down), np.float32(1.0)]
    assert min(out) >= np.float32(TAQ_BASE_THR)
    return [float(t) for t in out]


def taq_name(oracle, thr):
    """The taq scenario whose pool threshold is thr, registered."""
    name = "end3_taq@%r" % float(thr)
    if name not in PT._CASES:
        PT.register(name, taq_case(oracle, float(thr)))
    return name


def scenario_name(oracle, which):
    """"ends" / "taq" -> the name the scenario is registered under in products_tm_cases."""
    name = "end3_" + which
    if name not in PT._CASES:
        PT.register(name, {"ends": ends_case, "taq": taq_case}[which](oracle))
    return name


def oracle_bits(oracle, case, thr, use_taq):
    """(fr, rf) bool [n_pairs, n_seq]: the oracle session's target_match(pair, orient=True) at threshold thr over the scenario's
    select_words DB at its own threshold squared -- every site of these scenarios is the best of its oligo on its sequence."""
    lo, hi = PT.amp_of(case)
    so = oracle.session(target_threshold=float(thr), amp_min=lo, amp_max=hi, use_taq_mama=int(use_taq))
    for s in case["seqs"]:
        so.add_target(s)
    so.select(case["panel"], SQ(case["thr"]))
    n = len(case["seqs"])
    fr, rf = np.zeros((len(case["panel"]), n), bool), np.zeros((len(case["panel"]), n), bool)
    for i, pair in enumerate(case["panel"]):
        bits, ori = so.target_match(pair, orient=True)
        assert ((ori != 0) == (bits != 0)).all()
        fr[i], rf[i] = (ori & 1) != 0, (ori & 2) != 0
    return fr, rf


def unpack_bits(rows, n):
    """uint64 [n_pairs, words] -> bool [n_pairs, n]."""
    rows = np.asarray(rows, np.uint64)
    return np.array([[(int(rows[i, s >> 6]) >> (s & 63)) & 1 for s in range(n)] for i in range(rows.shape[0])], bool).reshape(rows.shape[0], n)
