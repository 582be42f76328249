"""Scenarios that take per-site melting off its one salt, one primer concentration and two- and four-fold codes; shared by
tests/test_melt_conditions_host.py (the oracle alone, and the oracle against the reference) and
tests/test_gpu_melt_conditions.py (the kernels against the oracle).

  * codes_case: one sequence, five oligos with three-fold codes (24, 9, 27, 24 and 243 expansions), every expansion of the first
    four and 16 of the fifth planted once as an exact site.
  * conditions: thermo_cases.SALTS x thermo_cases.STRANDS x four template concentrations around the oligos' own
    primer_strand / degeneracy: both branches of NucCruc's two-strand rule and the equality.
  * pool_case: products_tm_cases' "random" scenario with a three-fold code in two of its primers, registered with
    products_tm_cases and (two pairs and their probes) probe_hit_cases at three conditions and at the default one.

The scenarios carry their conditions in the keys salt, primer_strand, template_strand (and probe_strand), which
site_tm_cases.conditions_of and the expectations read.  Everything is a pure function of fixed seeds.  Nothing here touches the
library under test.
"""
import functools
import random

import numpy as np

import probe_hit_cases as H
import products_tm_cases as PC
import site_tm_cases as SC
import site_variant_cases as VC
import thermo_cases as TC
from testdata import rand_seq, revcomp

THREE_FOLD = {"B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG"}
NIBBLE = {"B": 2 | 4 | 8, "H": 1 | 2 | 8}
GAP, LEAD = 9, 40

# (length, ((position from the 5' end, fold), ...)): every degenerate position at least 2 bases from either end.  A centred
# n-mer begins at slot (33 - n) / 2, a 32-mer at slot 0.  24 = 2 x 3 x 4 leaves the fourth oligo three degenerate slots: 15 and
# 16 (the fastest and the slowest digit of the odometer, either side of the seam between the word's halves) and one below them;
# the fifth has degenerate slots at 15 and 16 and on both sides of them.
OLIGOS = ((22, ((3, 3), (11, 2), (18, 4))),
          (20, ((4, 3), (14, 3))),
          (25, ((3, 3), (12, 3), (21, 3))),
          (32, ((10, 2), (15, 3), (16, 4))),
          (32, ((6, 3), (15, 3), (16, 3), (21, 3), (27, 3))))
DEGENERACIES = (24, 9, 27, 24, 243)
BIG = 4                                         # the oligo of which only BIG_PLANTED expansions are planted
BIG_PLANTED = 16
EQUAL_DEGENERACY = 24                           # the template concentration of the third kind equals primer_strand / 24
# A seed at which tests/test_melt_conditions_host.py's conditions hold: no clamped site, and every planted expansion the
# unique best at its own site.  (Of the seeds 7101 .. 7124 two do: a mismatch beside another degenerate slot melts above the
# exact base often enough, and an AT-rich oligo's weakest expansion falls below 0 C at 10 mM.)
CODES_SEED = 7105


def _code(rng, base, fold):
    """An IUPAC code of `fold` bases that holds `base`."""
    if fold == 2:
        return "R" if base in "AG" else "Y"
    if fold == 4:
        return "N"
    return rng.choice(sorted(c for c, held in THREE_FOLD.items() if base in held))


def _degenerate(rng, n, places):
    while True:
        s = SC._primer(rng, n)
        # the 22-mer spells B, Y and N; it is GC-rich, so that its expansions with three mismatches melt above 0 C at 10 mM
        if n != 22 or (s[3] != "A" and s[11] in "CT" and sum(b in "GC" for b in s) >= 13):
            break
    out = list(s)
    for p, fold in places:
        assert 2 <= p < n - 2
        out[p] = "B" if (n == 22 and fold == 3) else _code(rng, s[p], fold)
    return "".join(out)


def expansions_of(oracle, word):
    """The oligo's expansions as texts, in oracle.word_expand's order (the order of the expansion index)."""
    return [SC.spell(SC.slots_of(x)) for x in oracle.word_expand(word)]


@functools.lru_cache(None)
def codes_case(oracle):
    """-> the scenario (site_tm_cases' format) with two more keys: planted[oligo] = the expansion indices planted, in
    sequence order, and texts = the oligos as IUPAC texts."""
    rng = random.Random(CODES_SEED)
    texts = [_degenerate(rng, n, places) for n, places in OLIGOS]
    w = oracle.centered_word
    words = [w(t) for t in texts]
    planted, parts, k = [], [rand_seq(rng, LEAD)], 0
    for o, c in enumerate(words):
        exps = expansions_of(oracle, c)
        assert len(exps) == DEGENERACIES[o] == len(set(exps))
        which = list(range(len(exps)))
        if o == BIG:
            which = sorted([0, len(exps) - 1] + rng.sample(range(1, len(exps) - 1), BIG_PLANTED - 2))
        planted.append(tuple(which))
        for e in which:
            parts += [exps[e] if k % 2 == 0 else revcomp(exps[e]), rand_seq(rng, GAP)]
            k += 1
    parts.append(rand_seq(rng, LEAD))
    return dict(seqs=["".join(parts)], panel=[(words[0], words[1]), (words[2], words[3]), (words[4], words[4])], thr=1.0,
                select="all", planted=tuple(planted), texts=tuple(texts))


CODES_SITES = sum(DEGENERACIES[:BIG]) + BIG_PLANTED
CODES_JOBS = sum(d * d for d in DEGENERACIES[:BIG]) + BIG_PLANTED * DEGENERACIES[BIG]


def duplex_strand(primer_strand, degeneracy):
    """primer_strand / degeneracy as the call computes it: the division in double, the result a float."""
    return float(np.float32(float(np.float32(primer_strand)) / degeneracy))


def template_strands(primer_strand):
    """0; half the smallest primer_strand / degeneracy of codes_case; one equal to primer_strand / 24 (the 9-fold oligo is
    above it, the 27- and 243-fold ones below); one above every one of them."""
    ca = [duplex_strand(primer_strand, d) for d in DEGENERACIES]
    out = (0.0, float(np.float32(min(ca) * 0.5)), duplex_strand(primer_strand, EQUAL_DEGENERACY), float(np.float32(2.0 * primer_strand)))
    assert 0.0 < out[1] < min(ca) and out[2] in ca and min(ca) < out[2] < max(ca) < out[3]
    return out


def conditions():
    """The 24 (salt, primer_strand, template_strand) of the grid."""
    return tuple((salt, ps, ts) for salt in TC.SALTS for ps in TC.STRANDS for ts in template_strands(ps))


def condition_id(cond):
    return "salt%g-primer%g-template%g" % cond


def at(case, cond):
    """The scenario at a condition."""
    return dict(case, salt=cond[0], primer_strand=cond[1], template_strand=cond[2])


DEFAULT = (SC.SALT, SC.PRIMER_STRAND, 0.0)
# the conditions at which the host test asks whether every expansion counts
COUNT_CONDITIONS = (DEFAULT, (0.01, 2e-8, 0.0), (1.0, 9e-7, 5e-8))


def reference_conditions():
    """The 6 conditions at which every duplex of codes_case is held to the reference: every salt, both primer concentrations,
    all four kinds of template concentration."""
    pick = ((0.05, 9e-7, 0), (0.05, 2e-8, 1), (0.01, 9e-7, 2), (0.01, 2e-8, 3), (1.0, 9e-7, 1), (1.0, 2e-8, 2))
    out = tuple((salt, ps, template_strands(ps)[k]) for salt, ps, k in pick)
    assert set(out) <= set(conditions())
    return out


# ---------------------------------------------------------------------------------------------------------------- pool_case
POOL_CONDITIONS = ((0.01, 2e-8, 0.0), (1.0, 9e-7, 5e-8), (0.05, 2e-8, 2e-8))
POOL_NAMES = ("mc_pool_0", "mc_pool_1", "mc_pool_2")
POOL_DEFAULT = "mc_pool_default"
POOL_PROBE_STRAND = 1e-7
POOL_WIDENED = ((0, 0, "H"), (2, 0, "B"))       # (pair, 0: F / 1: R, code): F of pair 0 and F of pair 2, the probe of pair 1


def widen_word(oracle, word, code):
    """The word with one interior slot (at least 2 from either end, the one nearest the middle whose base the code holds)
    widened to a three-fold code."""
    sl = SC.slots_of(word)
    start, stop = oracle.word_start(word), oracle.word_stop(word)
    mid = (start + stop) // 2
    ok = [k for k in range(start + 2, stop - 1) if sl[k] in SC.BASE and sl[k] & NIBBLE[code]]
    k = min(ok, key=lambda k: (abs(k - mid), k))
    sl[k] = NIBBLE[code]
    out = VC.word_of_slots(sl)
    assert oracle.word_degeneracy(out) == 3 * oracle.word_degeneracy(word)
    return out


@functools.lru_cache(None)
def pool_case(oracle):
    """products_tm_cases.scenario(oracle, "random") -- 8 sequences x 2 kb, 6 pairs -- with H in F of pair 0 and B in F of pair 2."""
    base = PC.scenario(oracle, "random")
    panel = [list(p) for p in base["panel"]]
    for pair, side, code in POOL_WIDENED:
        panel[pair][side] = widen_word(oracle, panel[pair][side], code)
    return dict(base, panel=[tuple(p) for p in panel])


def probe_case(case):
    """The first two pairs with the next pair's F as their probe (as tests/test_gpu_shared_scratch.py), at POOL_PROBE_STRAND."""
    big = case["panel"]
    return dict(case, panel=big[:2], probes=[big[(i + 1) % len(big)][0] for i in range(2)], probe_strand=POOL_PROBE_STRAND)


def register_pool(oracle):
    """pool_case under POOL_NAMES (at POOL_CONDITIONS) and POOL_DEFAULT, with products_tm_cases and probe_hit_cases."""
    base = pool_case(oracle)
    for name, cond in zip(POOL_NAMES + (POOL_DEFAULT,), POOL_CONDITIONS + (DEFAULT,)):
        if name not in PC._CASES:
            PC.register(name, at(base, cond))
            H.register(name, probe_case(at(base, cond)))
    return POOL_NAMES
