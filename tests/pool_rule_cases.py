"""The independent expectation for pcr_pool_anneal_profile_end3, pcr_pool_conflicts_end3 and pcr_pool_probe_hits_end3, and the
inputs their tests share.

Nothing new is modelled here.  The products under a rule are end3_cases.expected's records (the oracle's word DB and duplex Tm,
the join, the per-site quantities and the rule, all restated in Python); they are handed to the models the three base calls
are tested against: anneal_profile_cases.expectation, pool_conflict_cases.expected(rec=, ids=) and, for the probes, the hits
of probe_hit_cases.everything whose product is among the ruled records, then probe_hit_cases.detected_of.  Nothing here
touches the library under test.

probe_ends is end3_cases.ends_case with a probe for two of its three pairs.  It departs from ends_case's four sequences in two
more places.  It has no EOS split: probe_hit_cases' model knows `splits` on a select_words DB only, and the split of ends_case cuts
the one product pair 1's probe lies in.  And sequence 1 gets a minus site of pair 1's reverse primer and a second site of
pair 1's probe: ends_case alone has no pair whose products on some sequence ALL fail a rule, so no `detected` bit could ever
go out.  With them, pair 1's only product on sequence 1 starts at the plus site with two mismatches among its last five bases.

arms is the panel the rule is for: two allele-specific assays whose forward primers differ in their last base, and a third
assay.  Every product between the two allele-specific assays has the mismatch under the primer's last base (their cell goes
away under a rule); the third assay's forward primer makes an exact and a mismatched product with the first one's reverse
primer (their cell loses a product and stays).
"""
import functools
import random

import numpy as np

import anneal_profile_cases as AP
import end3_cases as E
import pool_conflict_cases as CC
import probe_hit_cases as H
import products_tm_cases as PT
from select_sites_cases import plant
from site_tm_cases import _primer, _sub
from testdata import rand_seq, revcomp

KEY = ("plus_oligo", "minus_oligo", "sequence", "begin", "end")

# end3_cases.rule_grid()'s (min_clamp3, window, max_end_mismatch) the GPU tests run, and the two identity rules
GRID = ((3, 0, 0), (0, 5, 1), (3, 5, 1), (32, 0, 0), (1, 1, 0), (6, 32, 0))
IDENT = 0.95                                     # two mismatches of 18 fail it, one of 20 passes: sqrt(16/18) < 0.95 < sqrt(19/20)
IDENT_ARMS = 0.98                                # one mismatch of 20 beside an exact site fails it: sqrt(19/20) < 0.98


def grid_rule(g):
    have = {(r["min_clamp3"], r["window"], r["max_end_mismatch"]): r for r in E.rule_grid()}
    return have[g]


def grid_rules():
    return [grid_rule(g) for g in GRID]


def ident_rules(thr=IDENT):
    return [E.rule_of(ident_threshold=thr), E.rule_of(ident_threshold=thr, use_taq_mama=1)]


def rules(thr=IDENT):
    return grid_rules() + ident_rules(thr)


def candidates(oracle):
    """Every (call, scenario name, rule) the tests could run; test_pool_rule_host.py shows which of them can fail a wrong join."""
    ends, pe, arms = ends_name(oracle), probe_ends_name(oracle), arms_name(oracle)
    out = [("anneal", n, r) for n in (ends, pe) for r in rules()]
    out += [("conflicts", n, r) for n, thr in ((ends, IDENT), (arms, IDENT_ARMS)) for r in rules(thr)]
    out += [("probes", pe, r) for r in rules()]
    return out


# The triples the GPU tests run: those of candidates() for which the models show a dropped and a kept product where the call
# reports it (test_pool_rule_host.py::test_input_conditions holds this list to that, and shows the others lack it).
_NO_PAIR_SEQUENCE = ((3, 0, 0), (0, 5, 1), (3, 5, 1), (1, 1, 0))   # on ends: every (pair, sequence) keeps a product under these


def triples(oracle):
    ends, pe, arms = ends_name(oracle), probe_ends_name(oracle), arms_name(oracle)
    g = lambda r: (r["min_clamp3"], r["window"], r["max_end_mismatch"])
    plain = lambda r: r["ident_threshold"] == 0.0
    out = [("anneal", ends, r) for r in grid_rules() if g(r) not in _NO_PAIR_SEQUENCE]
    out += [("anneal", pe, r) for r in rules() if not (plain(r) and g(r) == (1, 1, 0))]
    out += [("conflicts", arms, r) for r in rules(IDENT_ARMS) if not (plain(r) and g(r) == (0, 5, 1))]
    out += [("probes", pe, r) for r in rules() if not (plain(r) and g(r) == (1, 1, 0))]
    return out


def triples_of(oracle, call):
    return [(n, r) for c, n, r in triples(oracle) if c == call]


def rule_id(rule):
    return "c%d_w%d_m%d_t%d_i%g" % (rule["min_clamp3"], rule["window"], rule["max_end_mismatch"], rule["use_taq_mama"], rule["ident_threshold"])


WORDS_RULE = E.rule_of(min_clamp3=32)
WORDS_SEQS = (63, 64, 65, 130)


# ---------------------------------------------------------------------------------------------------------------- scenarios
PROBE_ENDS = "rule_probe_ends"
PROBE0_AT, PROBE0_LEN = 728, 24                  # sequence 0: bases 721 .. 759 lie between the last plus and the first minus site
PROBE1_AT, PROBE1_LEN = 290, 22                  # sequence 2: inside the exact product of pair 1 (plus site 250 .. 267, minus 360 ..)
SEQ1_PROBE1_AT, SEQ1_MINUS_AT = 260, 300         # sequence 1: bases 252 .. 379 are free; pair 1's mismatched plus site is at 160 .. 177


@functools.lru_cache(None)
def probe_ends_case(oracle):
    base = E.ends_case(oracle)
    rng = random.Random(6201)
    p0, p1 = _primer(rng, PROBE0_LEN), _primer(rng, PROBE1_LEN)
    seqs = list(base["seqs"])
    seqs[0] = plant(seqs[0], PROBE0_AT, p0)
    seqs[2] = plant(seqs[2], PROBE1_AT, p1)
    rb = revcomp(seqs[2][360:360 + 25])                                      # pair 1's reverse primer, read back from its exact site
    assert oracle.centered_word(rb) == base["panel"][1][1]
    seqs[1] = plant(seqs[1], SEQ1_PROBE1_AT, p1)
    seqs[1] = plant(seqs[1], SEQ1_MINUS_AT, revcomp(rb))
    w = oracle.centered_word
    case = dict(base, seqs=seqs, probes=[w(p0), w(p1), None])
    del case["eos"]
    return case


ARMS = "rule_arms"
ARMS_F_AT, ARMS_R_AT, ARMS_F2_AT = 40, 170, 90


@functools.lru_cache(None)
def arms_case(oracle):
    """Rows (Fa, R1), (Fa', R2), (Fc, Rc); Fa' is Fa with another last base.  Sequence 0: Fa and R1 (row 0's product; Fa' x R1 is
    spurious, cell {0,1}, mismatch under the last base).  Sequence 1: Fa' and R2 (row 1's; Fa x R2 likewise).  Sequence 2: Fc, a
    copy of Fc with a substitution under its last base, and R1: two products of cell {0,2}, one exact.  Sequence 3: Fc and Rc."""
    rng = random.Random(6202)
    fa, r1, r2, fc, rc = (_primer(rng, n) for n in (20, 21, 22, 20, 21))
    fa2 = fa[:-1] + {"A": "C", "C": "A", "G": "T", "T": "G"}[fa[-1]]         # a transversion: no two-fold code joins them
    def seq(plus, minus, more=()):
        s = rand_seq(rng, 300)
        s = plant(s, ARMS_F_AT, plus)
        s = plant(s, ARMS_R_AT, revcomp(minus))
        for at, text in more:
            s = plant(s, at, text)
        return s
    seqs = [seq(fa, r1), seq(fa2, r2), seq(fc, r1, [(ARMS_F2_AT, _sub(fc, (len(fc) - 1,)))]), seq(fc, rc)]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(fa), w(r1)), (w(fa2), w(r2)), (w(fc), w(rc))], thr=float(np.sqrt(np.float32(0.8))), select="all")


def arms_name(oracle):
    if ARMS not in PT._CASES:
        PT.register(ARMS, arms_case(oracle))
    return ARMS


def ends_name(oracle):
    return E.scenario_name(oracle, "ends")


def probe_ends_name(oracle):
    """probe_ends, registered with products_tm_cases (its pool) and with probe_hit_cases (pool and probes)."""
    if PROBE_ENDS not in PT._CASES:
        PT.register(PROBE_ENDS, probe_ends_case(oracle))
        H.register(PROBE_ENDS, probe_ends_case(oracle))
    return PROBE_ENDS


def no_probe_name(oracle, name):
    """A products_tm_cases scenario as a probe_hit_cases one whose pairs have no probe: every detected row is fr | rf."""
    case = PT.scenario(oracle, name)
    key = "rule_no_probe:" + name
    if key not in H._CASES:
        H.register(key, dict(case, probes=[None] * len(case["panel"])))
    return key


def floor_of(oracle, name):
    """An in-range floor: the middle one of the distinct positive min-Tm of the scenario's products (>= keeps it); on arms, whose
    seven products leave one cell above their middle, the second lowest."""
    v = np.unique(PT.min_tm(E.products_before_rule(oracle, name)[1]))
    pos = v[v > 0]
    return float(pos[1 if name == ARMS else len(pos) // 2])


# ---------------------------------------------------------------------------------------------------------------- the models
@functools.lru_cache(None)
def _ruled(oracle, name, rule_key, tm_floor):
    ids, rec, fr, rf, before = E.expected(oracle, name, dict(rule_key), tm_floor)
    for a in (rec, fr, rf):
        a.setflags(write=False)
    return ids, rec, fr, rf, before


def ruled(oracle, name, rule, tm_floor=0.0):
    """end3_cases.expected, computed once per (scenario, rule, floor) and left unchanged."""
    return _ruled(oracle, name, tuple(sorted(rule.items())), float(tm_floor))


def anneal_temps(oracle, name, rule):
    return AP.temps_of(ruled(oracle, name, rule)[1])


def anneal(oracle, name, rule, temps):
    """-> (oligo ids, count, points, pair_sequences, melt_fr, melt_rf, melt_spurious) over the products that pass the rule."""
    ids, rec = ruled(oracle, name, rule)[:2]
    return (ids, len(rec)) + AP.expectation(ids, rec, AP.n_seq_of(oracle, name), temps)


def conflicts(oracle, name, rule, tm_floor=0.0, dimer_rule=CC.NO_DIMERS, dimer_floor=0.0):
    """-> (oligo ids, records as pool_conflict_cases' tuples) with only the ruled products attributed."""
    ids, rec = ruled(oracle, name, rule, tm_floor)[:2]
    return CC.expected(oracle, name, tm_floor, dimer_rule, dimer_floor, pool=PT.scenario(oracle, name)["panel"], rec=rec, ids=ids)


def keys_of(rec):
    return set(zip(*(rec[f].tolist() for f in KEY)))


def probes(oracle, pt_name, h_name, rule, tm_floor=0.0, probe_tm_floor=0.0):
    """-> (oligo ids, probe ids, hits, detected): the hits inside the ruled products, detected from those products and hits.
    pt_name / h_name: the scenario's names in products_tm_cases and in probe_hit_cases."""
    ids, pid, prod, _, hits = H.everything(oracle, h_name)
    r_ids, rec = ruled(oracle, pt_name, rule, tm_floor)[:2]
    assert list(r_ids) == list(ids)
    assert keys_of(rec) <= keys_of(prod)
    have = keys_of(rec)
    k = H.kept(hits, tm_floor, probe_tm_floor)
    k = k[[key in have for key in zip(*(k[f].tolist() for f in KEY))]] if len(k) else k
    return list(ids), pid, k, H.detected_of(k, rec, ids, pid, len(H.scenario(oracle, h_name)["seqs"]))
