"""The independent expectation for pcr_site_repair, and the scenarios its tests add.

expected_repair() restates the call's definition (include/pcramp_hip.h) on what site_variant_cases.expected_variants gives
for the same word DB -- the variants in record order and the site map -- with each site's sequence from site_tm_cases' site
rule (the members), Python integers for the slots, and oracle.is_valid for the verdicts.  Nothing here touches the library
under test.
"""
import functools
import random

import numpy as np

import site_tm_cases as SC
import site_variant_cases as VC
from select_sites_cases import floor_of, plant, word_and_np
from site_tm_cases import distinct_oligos, slots_of
from testdata import rand_seq, revcomp

STEP = np.dtype({"names": ["word", "oligo", "step", "variant", "added_mask", "n_expansions", "candidates", "sequences_held",
                           "sites_held", "variants_held", "sequences_total", "gain", "flags", "valid", "reserved"],
                 "formats": [(np.uint64, (2,))] + [np.uint32] * 14,
                 "offsets": [0] + [16 + 4 * i for i in range(14)], "itemsize": 72})
COMPLETE, NO_GAIN, DEGENERACY, STEPS = 1, 2, 4, 8
NO_VARIANT = 0xFFFFFFFF
FIELDS = STEP.names[1:-1]
THERMO = dict(salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, tm_min=50.0, tm_max=75.0, max_hairpin=40.0, max_dimer=40.0)


def site_sequences(oracle, entries, panel, thr, active=None):
    """The sequence of every site, in pcr_site_tm's record order (oligo, sequence, loc5, strand): what the site map indexes."""
    _, words = distinct_oligos(panel)
    thr2 = np.float32(thr) * np.float32(thr)
    w0 = np.array([e[0] for e in entries], dtype=np.uint64)
    w1 = np.array([e[1] for e in entries], dtype=np.uint64)
    sites = set()
    for oid, c in enumerate(words):
        start, stop = oracle.word_start(c), oracle.word_stop(c)
        hit = np.nonzero(word_and_np(c, w0, w1) >= floor_of(c, thr2))[0] if len(entries) else []
        for i in hit:
            _, _, loc, index, strand = entries[i]
            if strand in (1, 2) and (active is None or active[index]):
                sites.add((oid, index, loc + start if strand == 1 else loc - stop, strand))
    return [s[1] for s in sorted(sites)]


def degeneracy(sl):
    d = 1
    for v in sl:
        if v:
            d *= bin(v).count("1")
    return d


def holds(w, v, start, stop, max_mismatch, clamp3):
    """Word slots w hold variant slots v: at most max_mismatch empty intersections in start..stop, none in the last clamp3."""
    miss = [k for k in range(start, stop + 1) if not (w[k] & v[k])]
    return len(miss) <= max_mismatch and clamp3 <= stop - start + 1 and all(k <= stop - clamp3 for k in miss)


def greedy(variants, sequences, oligo_slots, start, stop, max_degeneracy, max_mismatch, clamp3, max_candidates, max_steps):
    """One oligo.  variants: [(global record index, slots, sites)] in record order; sequences: {sequence: set of local variant
    numbers}.  -> list of step dicts."""
    def held_by(w):
        hv = set(i for i, (_, v, _) in enumerate(variants) if holds(w, v, start, stop, max_mismatch, clamp3))
        return hv, set(s for s, vs in sequences.items() if vs & hv)

    foot = lambda v: [v[k] if start <= k <= stop else 0 for k in range(32)]
    w = list(oligo_slots)
    hv, hs = held_by(w)
    steps = [dict(word=VC.word_of_slots(w), step=0, variant=NO_VARIANT, added_mask=0, n_expansions=degeneracy(w), candidates=0,
                  sequences_held=len(hs), sites_held=sum(variants[i][2] for i in hv), variants_held=len(hv),
                  sequences_total=len(sequences), gain=0, flags=0)]
    while True:
        if len(hs) == len(sequences):
            steps[-1]["flags"] = COMPLETE
            break
        if len(steps) - 1 == max_steps:
            steps[-1]["flags"] = STEPS
            break
        single = [i for i, (_, v, _) in enumerate(variants)
                  if i not in hv and all(bin(v[k]).count("1") == 1 for k in range(start, stop + 1))]
        cand = [i for i in single if degeneracy([a | b for a, b in zip(w, foot(variants[i][1]))]) <= max_degeneracy][:max_candidates]
        best = None
        for i in cand:
            w2 = [a | b for a, b in zip(w, foot(variants[i][1]))]
            hv2, hs2 = held_by(w2)
            key = (-(len(hs2) - len(hs)), -sum(variants[j][2] for j in hv2), degeneracy(w2), variants[i][0])
            if best is None or key < best[0]:
                best = (key, i, w2, hv2, hs2)
        if best is None or best[0][0] == 0:
            steps[-1]["flags"] = DEGENERACY if (not cand and single) else NO_GAIN
            break
        _, i, w2, hv2, hs2 = best
        added = sum(1 << (k - start) for k in range(start, stop + 1) if w2[k] != w[k])
        steps.append(dict(word=VC.word_of_slots(w2), step=len(steps), variant=variants[i][0], added_mask=added,
                          n_expansions=degeneracy(w2), candidates=len(cand), sequences_held=len(hs2),
                          sites_held=sum(variants[j][2] for j in hv2), variants_held=len(hv2), sequences_total=len(sequences),
                          gain=len(hs2) - len(hs), flags=0))
        w, hv, hs = w2, hv2, hs2
    return steps


def expected_repair(oracle, entries, panel, thr, max_degeneracy=16, max_mismatch=0, clamp3=0, max_candidates=256, max_steps=12,
                    active=None, thermo=THERMO, check_homo_dimer=True):
    """-> (oligo_id list, STEP array sorted by (oligo, step)).  thermo: oracle.is_valid's keyword arguments, or None."""
    ids, var, site_map, _ = VC.expected_variants(oracle, entries, panel, thr, active=active, thermo=False)
    seq_of_site = site_sequences(oracle, entries, panel, thr, active)
    assert len(seq_of_site) == len(site_map)
    _, words = distinct_oligos(panel)
    rows = []
    for oid, c in enumerate(words):
        start, stop = oracle.word_start(c), oracle.word_stop(c)
        mine = [f for f in range(len(var)) if int(var[f]["oligo"]) == oid]
        local = {f: i for i, f in enumerate(mine)}
        variants = [(f, slots_of((int(var[f]["word"][0]), int(var[f]["word"][1]))), int(var[f]["sites"])) for f in mine]
        sequences = {}
        for s, f in zip(seq_of_site, site_map):
            if f in local:
                sequences.setdefault(s, set()).add(local[f])
        for st in greedy(variants, sequences, slots_of(c), start, stop, max_degeneracy, max_mismatch, clamp3, max_candidates, max_steps):
            r = np.zeros(1, STEP)
            r["word"] = st["word"]
            r["oligo"] = oid
            for f in FIELDS:
                if f not in ("oligo", "valid"):
                    r[f] = st[f]
            if thermo is not None:
                r["valid"] = 1 if oracle.is_valid(st["word"], check_homo_dimer=check_homo_dimer, **thermo) else 0
            rows.append(r)
    return ids, (np.concatenate(rows) if rows else np.zeros(0, STEP))


def expectation(oracle, case, **kw):
    """expected_repair() of a scenario on the DB site_tm_cases.db_of() gives, with the scenario's own repair arguments."""
    args = dict(case.get("repair", {}))
    args.update(kw)
    return expected_repair(oracle, SC.db_of(oracle, case), case["panel"], case["thr"], active=case.get("active"), **args)


def as_tuples(rec):
    return [(int(r["word"][0]), int(r["word"][1])) + tuple(int(r[f]) for f in FIELDS) for r in rec]


# ---------------------------------------------------------------------------------------------------------------- scenarios
# As site_tm_cases' (seqs, panel, thr, select, optionally active), plus "repair": the call's own arguments.
SUB3 = {"A": "CGT", "C": "AGT", "G": "ACT", "T": "ACG"}
FLOOR_18_OF_20 = float(np.sqrt(np.float32(0.88)))                              # threshold^2 * 20 rounds up to 18


def _case(oracle, seqs, oligos, thr=FLOOR_18_OF_20, active=None, **repair):
    w = oracle.centered_word
    panel = [(w(f), w(r)) for f, r in oligos]
    return dict(seqs=seqs, panel=panel, thr=thr, select="all", active=active, repair=repair)


def _host(rng, site, n=90, at=30):
    """A random sequence with the site at base `at` between fixed flanking bases (the flanks are part of a variant's key)."""
    return plant(rand_seq(rng, n), at - 1, "A" + site + "C")


def _other(rng):
    return SC._primer(rng, 20)


@functools.lru_cache(None)
def free_coverage_case(oracle):
    """One 20-mer; variant A (base 3 substituted) in 5 sequences, B (base 10) in 4, C (both) in 1; the exact site in 2.
    Two candidates are weighed a step (C's own union would hold A, B and C at once and win step 1 outright): step 1 unions A
    (gain 5), step 2 unions B with gain 5: its 4 and C's sequence, which nobody unioned."""
    rng = random.Random(6101)
    p = SC._primer(rng, 20)
    a, b, c = SC._sub(p, (3,)), SC._sub(p, (10,)), SC._sub(p, (3, 10))
    seqs = [_host(rng, a) for _ in range(5)] + [_host(rng, b) for _ in range(4)] + [_host(rng, c)] + [_host(rng, p) for _ in range(2)]
    return _case(oracle, seqs, [(p, _other(rng))], max_candidates=2)


@functools.lru_cache(None)
def distinct_case(oracle, n):
    """n sequences carry the exact site, n more the site with base 6 substituted (variant M), and of those the first also
    carries the exact site a second time: its two sites belong to two variants and it is one sequence.  The last sequence,
    inactive, has a spelling of its own (base 12).  n = 65, 129: the run counts sit one past a 64-bit word of the bitset."""
    rng = random.Random(6102 + n)
    p = SC._primer(rng, 20)
    m = SC._sub(p, (6,))
    seqs = [_host(rng, p) for _ in range(n)]
    seqs += [plant(_host(rng, m), 59, "A" + p + "C")] + [_host(rng, m) for _ in range(n - 1)]
    seqs.append(_host(rng, SC._sub(p, (12,))))
    return _case(oracle, seqs, [(p, _other(rng))], active=tuple([True] * (2 * n) + [False]))


@functools.lru_cache(None)
def wide_case(oracle, max_candidates):
    """A 25-mer and 300 single- and double-substitution variants of it in one sequence each (variant i in i % 3 + 1 sequences
    so that the record order is not the planting order), more than one workgroup's 256 threads and than max_candidates."""
    rng = random.Random(6103)
    p = SC._primer(rng, 25)
    spellings = []
    for k in range(25):
        for ch in SUB3[p[k]]:
            spellings.append(p[:k] + ch + p[k + 1:])
    for k in range(23):                                                       # 75 singles + the first 225 doubles = 300
        for j in (k + 1, k + 2):
            for ch in SUB3[p[k]]:
                for ch2 in SUB3[p[j]]:
                    if len(spellings) < 300:
                        spellings.append(p[:k] + ch + p[k + 1:j] + ch2 + p[j + 1:])
    assert len(spellings) == 300 and len(set(spellings)) == 300
    seqs = []
    for i, s in enumerate(spellings):
        seqs += [_host(rng, s) for _ in range(i % 3 + 1)]
    return _case(oracle, seqs, [(p, SC._primer(rng, 25))], thr=float(np.sqrt(np.float32(0.9))), max_candidates=max_candidates,
                 max_degeneracy=4, max_steps=3)


@functools.lru_cache(None)
def degeneracy_case(oracle, start_codes=(), max_degeneracy=4, max_steps=12, copies=(3, 2, 1, 1)):
    """A 20-mer, optionally degenerate to begin with (start_codes: ((place, code), ...)), whose sites carry substitutions at
    places 2, 5, 9 and 14 -- in `copies` sequences each -- and the exact spelling in two."""
    rng = random.Random(6104)
    p = SC._primer(rng, 20)
    seqs = []
    for place, n in zip((2, 5, 9, 14), copies):
        seqs += [_host(rng, SC._sub(p, (place,))) for _ in range(n)]
    seqs += [_host(rng, p) for _ in range(2)]
    q = p
    for place, code in start_codes:
        q = SC._widen(q, (place,), code)
    return _case(oracle, seqs, [(q, _other(rng))], max_degeneracy=max_degeneracy, max_steps=max_steps)


@functools.lru_cache(None)
def deep_case(oracle):
    """Four places of a 20-mer, each with all three substitutions, in 12 .. 1 sequences: 12 steps to 4*4*4*4 = 256 expansions."""
    rng = random.Random(6105)
    p = SC._primer(rng, 20)
    seqs, n = [], 12
    for place in (1, 6, 11, 16):
        for ch in SUB3[p[place]]:
            seqs += [_host(rng, p[:place] + ch + p[place + 1:]) for _ in range(n)]
            n -= 1
    seqs += [_host(rng, p)]
    return _case(oracle, seqs, [(p, _other(rng))], max_degeneracy=256, max_steps=12)


@functools.lru_cache(None)
def ambiguity_case(oracle):
    """A 20-mer; three sequences spell its site with N at base 7 (held: N intersects), two with N at base 7 and base 4
    substituted (not held, and never a candidate: no single base at 7), two with base 4 substituted (the candidate, whose
    union holds the former two as well).  (A site hanging over a sequence end, empty slots in the footprint, is in
    site_tm_cases.ends_case, which the GPU test runs too.)"""
    rng = random.Random(6106)
    p = SC._primer(rng, 20)
    n7 = p[:7] + "N" + p[8:]
    s4 = SC._sub(p, (4,))
    seqs = [_host(rng, n7) for _ in range(3)] + [_host(rng, s4[:7] + "N" + s4[8:]) for _ in range(2)]
    seqs += [_host(rng, s4) for _ in range(2)] + [_host(rng, p)]
    return _case(oracle, seqs, [(p, _other(rng))])


@functools.lru_cache(None)
def mismatch_case(oracle, max_mismatch, clamp3):
    """SC.placement_case's five spellings (exact; base 10; the 3' base; bases 0 and 1; bases 3, 9 and 15) on both strands."""
    case = dict(SC.placement_case(oracle))
    case["repair"] = dict(max_mismatch=max_mismatch, clamp3=clamp3)
    return case


@functools.lru_cache(None)
def shapes_case(oracle):
    """Oligo q is F of three pairs; r2 has only strand-2 sites (planted reverse-complemented), with one substitution in two
    of four sequences; z has no site anywhere."""
    rng = random.Random(6107)
    q, r2, z, x = (SC._primer(rng, 20) for _ in range(4))
    seqs = []
    for i in range(4):
        s = rand_seq(rng, 160)
        s = plant(s, 19, "A" + (q if i else SC._sub(q, (8,))) + "C")
        s = plant(s, 89, revcomp("A" + (r2 if i < 2 else SC._sub(r2, (5,))) + "C"))
        seqs.append(s)
    return _case(oracle, seqs, [(q, r2), (q, z), (q, x)])


def ties_case(oracle):
    """VC.ties_case: four one-sequence variants that tie in gain, sites and expansions; the record index decides."""
    case = dict(VC.ties_case(oracle))
    case["repair"] = dict(max_degeneracy=16)
    return case


@functools.lru_cache(None)
def expansions_tie_case(oracle):
    """The oligo is R (A or G) at base 4.  Variant X has base 4 = C (a third base there: 2 -> 3 expansions), variant Y has
    base 12 substituted (1 -> 2 there: 2 -> 4 expansions); both in two sequences with one site each: gain and sites tie, the
    fewer expansions win although Y is planted to come first in record order when the planes say so."""
    rng = random.Random(6108)
    p = SC._primer(rng, 20)
    p = p[:4] + "A" + p[5:]
    x = p[:4] + "C" + p[5:]
    y = SC._sub(p, (12,))
    seqs = [_host(rng, y) for _ in range(2)] + [_host(rng, x) for _ in range(2)] + [_host(rng, p)]
    q = p[:4] + "R" + p[5:]
    return _case(oracle, seqs, [(q, _other(rng))], max_degeneracy=6)
