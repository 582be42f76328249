"""The independent expectation for pcr_site_variants, and the scenarios its tests add to site_tm_cases'.

expected_variants() restates the call's definition (include/pcramp_hip.h) on a list of word-DB entries the CPU oracle produced:
site_tm_cases' site and pick rules, the sites grouped by (oligo, the picked entry's slots inside T), the mismatch mask and the
clamps from the slots, one melt per variant through the heterodimer cache site_tm_cases keeps, the record order.  Nothing here
touches the library under test.
"""
import functools
import random

import numpy as np

import site_tm_cases as SC
from select_sites_cases import floor_of, plant, word_and_np
from site_tm_cases import distinct_oligos, occupied_in_window, planes_of, slots_of, target_of
from testdata import rand_seq, revcomp

VARIANT = np.dtype([("word", np.uint64, (2,)), ("oligo", np.uint32), ("sites", np.uint32), ("sequences", np.uint32),
                    ("matches", np.uint32), ("mismatch_mask", np.uint32), ("clamp3", np.uint32), ("clamp5", np.uint32),
                    ("n_expansions", np.uint32), ("flags", np.uint32), ("first_sequence", np.uint32),
                    ("first_loc5", np.int32), ("first_strand", np.uint32), ("tm_max", np.float32),
                    ("tm_min", np.float32), ("dH", np.float32), ("dS", np.float32)])


def word_of_slots(sl):
    w = [0, 0]
    for k, v in enumerate(sl):
        w[k >> 4] |= int(v) << ((15 - (k & 15)) * 4)
    return tuple(w)


def expected_variants(oracle, entries, panel, thr, salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, template_strand=0.0,
                      active=None, thermo=True, jobs=None, cache=None):
    """-> (oligo_id list, VARIANT array in record order, site map: for the r-th site in (oligo, sequence, loc5, strand) order
    the index of its variant, number of (variant, expansion) jobs -- 0 with thermo=False)."""
    ids, words = distinct_oligos(panel)
    cache = SC._CACHE if cache is None else cache
    thr2 = np.float32(thr) * np.float32(thr)
    w0 = np.array([e[0] for e in entries], dtype=np.uint64)
    w1 = np.array([e[1] for e in entries], dtype=np.uint64)
    groups, members = {}, []                       # (oligo, masked slots) -> [member index]; (oligo, sequence, loc5, strand, key)
    for oid, c in enumerate(words):
        start, stop = oracle.word_start(c), oracle.word_stop(c)
        hit = np.nonzero(word_and_np(c, w0, w1) >= floor_of(c, thr2))[0] if len(entries) else []
        sites = {}
        for i in hit:
            _, _, loc, index, strand = entries[i]
            if strand not in (1, 2) or (active is not None and not active[index]):
                continue
            sites.setdefault((index, loc, strand), []).append(entries[i])
        lo, hi = max(start - 1, 0), min(stop + 1, 31)
        for (index, loc, strand), group in sites.items():
            esl = [slots_of(e) for e in group]
            most = max(occupied_in_window(s, start, stop) for s in esl)
            sl = min((s for s in esl if occupied_in_window(s, start, stop) == most), key=planes_of)
            masked = tuple(v if lo <= k <= hi else 0 for k, v in enumerate(sl))
            key = (oid, masked)
            groups.setdefault(key, []).append(len(members))
            members.append((oid, index, loc + start if strand == 1 else loc - stop, strand, key))
    rows, n_jobs = {}, 0
    for (oid, masked), mem in groups.items():
        c = words[oid]
        csl = slots_of(c)
        start, stop = oracle.word_start(c), oracle.word_stop(c)
        rec = np.zeros(1, VARIANT)
        rec["word"] = word_of_slots(masked)
        rec["oligo"], rec["sites"] = oid, len(mem)
        rec["sequences"] = len(set(members[m][1] for m in mem))
        match = [bool(masked[k] & csl[k]) for k in range(start, stop + 1)]
        rec["matches"] = sum(match)
        rec["mismatch_mask"] = sum(1 << i for i, ok in enumerate(match) if not ok)
        rec["clamp5"] = next((i for i, ok in enumerate(match) if not ok), len(match))
        rec["clamp3"] = next((i for i, ok in enumerate(reversed(match)) if not ok), len(match))
        exps = [SC.spell(slots_of(x)) for x in oracle.word_expand(c)]
        rec["n_expansions"] = len(exps)
        first = min(members[m][1:4] for m in mem)
        rec["first_sequence"], rec["first_loc5"], rec["first_strand"] = first
        tgt = target_of(masked, start, stop)
        if tgt is None:
            rec["flags"] = SC.NO_TM
        if thermo:
            n_jobs += len(exps)
        if thermo and tgt is not None:
            degen = oracle.word_degeneracy(c)
            ca = np.float32(float(np.float32(primer_strand)) / degen)
            cb = np.float32(template_strand)
            res = []
            for q in exps:
                k = (q, tgt[0], float(ca), float(cb))
                res.append(SC.melt_cached(oracle, cache, k, salt))
                if jobs is not None:
                    jobs.add(k)
            tms = [r[0] for r in res]
            best = max(range(len(res)), key=lambda k: (tms[k], -k))     # the highest Tm, the lowest index on a tie
            rec["tm_max"], rec["tm_min"] = tms[best], min(tms)
            rec["dH"], rec["dS"] = res[best][1], res[best][2]
        rows[(oid, masked)] = rec
    order = sorted(rows, key=lambda k: (k[0], -int(rows[k]["sequences"][0]), -int(rows[k]["sites"][0]),
                                        -int(rows[k]["matches"][0]), planes_of(k[1])))
    index_of = {k: i for i, k in enumerate(order)}
    out = np.concatenate([rows[k] for k in order]) if order else np.zeros(0, VARIANT)
    site_map = [index_of[m[4]] for m in sorted(members, key=lambda m: m[:4])]
    return ids, out, site_map, n_jobs


def expectation(oracle, case, jobs=None, **kw):
    """expected_variants() of a scenario on the DB site_tm_cases.db_of() gives."""
    args = dict(SC.conditions_of(case), template_strand=case.get("template_strand", 0.0), active=case.get("active"))
    args.update(kw)
    return expected_variants(oracle, SC.db_of(oracle, case), case["panel"], case["thr"], jobs=jobs, **args)


def as_bits(rec):
    """Records -> tuples with every float as its bit pattern (the comparison the tests make)."""
    f = lambda x: int(np.float32(x).view(np.uint32))
    ints = ("oligo", "sites", "sequences", "matches", "mismatch_mask", "clamp3", "clamp5", "n_expansions", "flags",
            "first_sequence", "first_loc5", "first_strand")
    return [(int(r["word"][0]), int(r["word"][1])) + tuple(int(r[n]) for n in ints)
            + (f(r["tm_max"]), f(r["tm_min"]), f(r["dH"]), f(r["dS"])) for r in rec]


# ---------------------------------------------------------------------------------------------------------------- scenarios
CONSERVED_N, CONSERVED_L = 600, 64
CONSERVED_3P, CONSERVED_FLANK, CONSERVED_5P2 = 6, 5, 3        # class sizes: 3' base, other 5' flank, two 5' mismatches
CONSERVED_EXACT = CONSERVED_N - CONSERVED_3P - CONSERVED_FLANK - CONSERVED_5P2 - 3   # ... and the plain members of the large class


@functools.lru_cache(None)
def conserved_case(oracle):
    """2. 600 sequences of 64 bases and one 20-mer.  Its site sits at base 20 between fixed flanking bases: exact in the large
    class (more members than two 256-thread blocks), with the 3' base substituted in 6 sequences, exact but behind another 5'
    flank base in 5, with its first two bases substituted in 3.  Of the large class one sequence holds the site twice, one
    holds it reverse-complemented (a strand-2 site); the last sequence, inactive, holds a spelling nobody else has."""
    rng = random.Random(5201)
    p = SC._primer(rng, 20)
    f5, f3 = "A", "C"
    other5 = "G"

    def seq(site, five=f5):
        s = rand_seq(rng, CONSERVED_L)
        return plant(s, 19, five + site + f3)

    seqs = [seq(p) for _ in range(CONSERVED_EXACT)]
    seqs += [seq(SC._sub(p, (19,))) for _ in range(CONSERVED_3P)]
    seqs += [seq(p, other5) for _ in range(CONSERVED_FLANK)]
    seqs += [seq(SC._sub(p, (0, 1))) for _ in range(CONSERVED_5P2)]
    twice = rand_seq(rng, CONSERVED_L)
    twice = plant(plant(twice, 6, f5 + p + f3), 35, f5 + p + f3)
    seqs.append(twice)
    seqs.append(plant(rand_seq(rng, CONSERVED_L), 19, revcomp(f5 + p + f3)))
    seqs.append(seq(SC._sub(p, (10,))))
    assert len(seqs) == CONSERVED_N and all(len(s) == CONSERVED_L for s in seqs)
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(p), w(p))], thr=float(np.sqrt(np.float32(0.88))), select="all",      # floor 17 of 20
                active=tuple([True] * (CONSERVED_N - 1) + [False]))


@functools.lru_cache(None)
def identity_case(oracle):
    """3. q is F of two pairs: one oligo.  q and q1 (q with base 8 substituted) both match q's site at this floor: two
    variants there, one per oligo.  d4 and d256 are degenerate oligos with 4 and 256 expansions on their own sites."""
    rng = random.Random(5202)
    q, a, b = (SC._primer(rng, 22) for _ in range(3))
    seqs = []
    for i in range(3):
        s = rand_seq(rng, 400)
        s = plant(s, 40, q)
        s = plant(s, 150, a if i else SC._sub(a, (5,)))
        s = plant(s, 260, revcomp(b))
        seqs.append(s)
    d4, d256 = SC._widen(a, (3, 15), "R"), SC._widen(b, (4, 9, 12, 17), "N")
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(q), w(SC._sub(q, (8,)))), (w(q), w(d4)), (w(d256), w(q))],
                thr=float(np.sqrt(np.float32(0.9))), select="all")


TIE_PLACES = (3, 7, 12, 16)


@functools.lru_cache(None)
def ties_case(oracle):
    """4. One 21-mer; four sequences carry its site with one substitution each, at four places: four variants with one
    sequence, one site and 20 matches each, which only the slot masks order; two sequences carry it exact."""
    rng = random.Random(5203)
    p, other = SC._primer(rng, 21), SC._primer(rng, 20)
    seqs = [plant(rand_seq(rng, 120), 50, SC._sub(p, (k,))) for k in TIE_PLACES]
    seqs += [plant(rand_seq(rng, 120), 50, p) for _ in range(2)]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(p), w(other))], thr=float(np.sqrt(np.float32(0.9))), select="all")


def new_scenarios(oracle):
    """name -> scenario: what tests/test_gpu_site_variants.py melts beyond site_tm_cases.gpu_scenarios."""
    return {"conserved": conserved_case(oracle), "identity": identity_case(oracle), "ties": ties_case(oracle)}


NEW_SCENARIO_NAMES = ("conserved", "identity", "ties")
