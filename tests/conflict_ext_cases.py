"""The independent expectation for pcr_pool_conflicts_ext, and the inputs its tests share.

The base half of a record is pool_conflict_cases.expected (the oracle's products and whole-oligo dimer cells), the extension
half dimer_end3_cases.expected (the oracle's cell records, tied to the reference by tests/golden/dimer_end3_reference_calls.json.gz).
join() puts them together with a plain loop over the row pairs: the set of distinct ordered cells, the sum of their
n_placements, the best kept cell by (dG, -run, q, t).  Nothing here touches the library under test.
"""
import functools
import random

import numpy as np

import dimer_end3_cases as DE
import pool_conflict_cases as CC
import pool_dimer_cases as DC
import products_tm_cases as PC
import site_tm_cases as SC
from site_tm_cases import _primer
from testdata import rand_seq, revcomp

EXTENSION = 4
NO_DIMERS = CC.NO_DIMERS
POOL, ASSAY = DC.POOL, DC.ASSAY
ZERO_EXT = (0,) * 15

EXT_FIELDS = ("ext_cells", "ext_placements", "ext_query", "ext_target", "ext_q_expansion", "ext_t_expansion", "ext_run",
              "ext_extension", "ext_overlap", "ext_overlap_matches", "ext_flags", "ext_dG", "ext_tm", "ext_dH", "ext_dS")
# name, offset, size of every field of the 96-byte record, in order
LAYOUT = (("row_a", 0, 4), ("row_b", 4, 4), ("products", 8, 8), ("sequences", 16, 4), ("melt", 20, 4), ("melt_sequence", 24, 4),
          ("dimer_tm", 28, 4), ("dimer_query", 32, 4), ("dimer_target", 36, 4), ("flags", 40, 4), ("reserved", 44, 4),
          ("ext_cells", 48, 4), ("ext_placements", 52, 4), ("ext_query", 56, 4), ("ext_target", 60, 4), ("ext_q_expansion", 64, 4),
          ("ext_t_expansion", 68, 4), ("ext_run", 72, 1), ("ext_extension", 73, 1), ("ext_overlap", 74, 1),
          ("ext_overlap_matches", 75, 1), ("ext_flags", 76, 4), ("ext_dG", 80, 4), ("ext_tm", 84, 4), ("ext_dH", 88, 4),
          ("ext_dS", 92, 4))


# ---------------------------------------------------------------------------------------------------------------- the join
def eight_cells(ids, a, b):
    """The list of eight ordered cells of {a, b} as the definition writes them, repeats and all."""
    oa, ob = (int(ids[2 * a]), int(ids[2 * a + 1])), (int(ids[2 * b]), int(ids[2 * b + 1]))
    return [(q, t) for q in oa for t in ob] + [(q, t) for q in ob for t in oa]


def has_repeats(ids, a, b):
    e = eight_cells(ids, a, b)
    return len(set(e)) < len(e)


def better(c, best):
    """Whether cell record c beats `best` where c comes later in (q, t) order: the lower dG, then the longer run."""
    return best is None or DE.f32(c[11]) < DE.f32(best[11]) or (DE.f32(c[11]) == DE.f32(best[11]) and c[6] > best[6])


def ext_half(ids, a, b, cell_of, dg_max):
    """The fifteen ext fields of {a, b}.  cell_of: (q, t) -> dimer_end3_cases' cell record of a cell with a placement."""
    cells = CC.dimer_cells_of(ids, a, b)                                    # the distinct ones, sorted
    have = [cell_of[c] for c in cells if c in cell_of]
    placements = sum(c[3] for c in have)
    kept = [c for c in have if dg_max is None or DE.f32(c[11]) <= np.float32(dg_max)]
    best = None
    for c in kept:                                                          # in (q, t) order: the first of the best stays
        if better(c, best):
            best = c
    if best is None:
        return (0, placements) + (0,) * 13
    return (len(kept), placements, best[0], best[1]) + tuple(best[4:])


def ext_half_brute(ids, a, b, cell_of, dg_max):
    """(ext_cells, ext_placements) by walking the list of eight and counting a cell the first time it is met."""
    seen, n_cells, n_place = [], 0, 0
    for c in eight_cells(ids, a, b):
        if c in seen:
            continue
        seen.append(c)
        r = cell_of.get(c)
        if r is None:
            continue
        n_place += r[3]
        n_cells += dg_max is None or bool(DE.f32(r[11]) <= np.float32(dg_max))
    return n_cells, n_place


def base_all(oracle, name, tm_floor=0.0, rule=NO_DIMERS, dimer_floor=0.0):
    """pool_conflict_cases.expected -> (ids, {(a, b): the eleven base fields of EVERY cell}, the set of cells it keeps).  A cell
    it does not keep has no product and, with a dimer rule, a dimer_tm below the floor: its dimer fields are those of the same
    call at floor 0 (which keeps every cell) and PCR_CONFLICT_DIMER is not set."""
    scenario(oracle, name)
    ids, kept = CC.expected(oracle, name, tm_floor, rule, dimer_floor)
    n_pool = len(ids) // 2
    out = {(r[0], r[1]): r for r in kept}
    keeps = set(out)
    if rule != NO_DIMERS:
        for r in CC.expected(oracle, name, tm_floor, rule, 0.0)[1]:
            if (r[0], r[1]) not in out:
                assert r[2] == 0 and not CC.F32(r[6]) >= np.float32(dimer_floor)
                out[(r[0], r[1])] = r[:9] + (r[9] & ~CC.DIMER,) + r[10:]
    for a in range(n_pool):
        for b in range(a, n_pool):
            out.setdefault((a, b), (a, b, 0, 0, CC.NO_PRODUCT_BITS, 0, 0, 0, 0, 0, 0))
    return ids, out, keeps


@functools.lru_cache(None)
def ext_cells_of(oracle, name, ext_rule, min_run, min_extension, cells=None):
    """(q, t) -> dimer_end3_cases' cell record, over the cells with a qualifying placement (all cells, or the listed ones)."""
    case = scenario(oracle, name)
    cond = SC.conditions_of(case)
    P = DC.Pool(oracle, case["panel"])
    rec, _ = DE.expected(oracle, P, ext_rule, min_run, min_extension, cells=None if cells is None else list(cells),
                         salt=cond["salt"], primer_strand=cond["primer_strand"])
    return {(r[0], r[1]): r for r in rec}


def join(ids, base, keeps, cell_of, dg_max, pairs=None):
    """The records of pcr_pool_conflicts_ext as tuples of 26 integers, sorted by (row_a, row_b).  cell_of = None: ext = NULL."""
    n_pool = len(ids) // 2
    out = []
    for a in range(n_pool):
        for b in range(a, n_pool):
            if pairs is not None and (a, b) not in pairs:
                continue
            c = base[(a, b)]
            x = ZERO_EXT if cell_of is None else ext_half(ids, a, b, cell_of, dg_max)
            if (a, b) in keeps or x[0] > 0:
                out.append(c[:9] + (c[9] | (EXTENSION if x[0] else 0),) + c[10:] + x)
    return out


def expected(oracle, name, tm_floor=0.0, rule=NO_DIMERS, dimer_floor=0.0, ext=None):
    """ext = None or (ext_rule, min_run, min_extension, dg_max) -> (oligo ids, the records as 26-tuples)."""
    ids, base, keeps = base_all(oracle, name, tm_floor, rule, dimer_floor)
    if ext is None:
        return ids, join(ids, base, keeps, None, None)
    cell_of = ext_cells_of(oracle, name, ext[0], ext[1], ext[2])
    return ids, join(ids, base, keeps, cell_of, ext[3])


def as_bits(rec):
    """Device records -> the tuples expected() gives."""
    out = []
    for r, base in zip(rec, CC.as_bits(rec)):
        out.append(base + tuple(int(r[f]) for f in EXT_FIELDS[:11]) + tuple(CC.BITS(r[f]) for f in EXT_FIELDS[11:]))
    return out


def from_cells(cells):
    """Device records of pool_dimers_end3 -> the (q, t) -> record map join() reads."""
    return {(c[0], c[1]): c for c in DE.cells_as_bits(cells)}


# ---------------------------------------------------------------------------------------------------------------- scenarios
# pool_conflict_cases' format: a product of (plus p, minus m) is p planted at `at` and the reverse complement of m 120 bases on.


def _target_of(rng, query, r, e, n):
    """An oligo of n bases that carries the reverse complement of query's last r bases at offset e, then a base that ends the run."""
    stretch = revcomp(query[len(query) - r:])
    return rand_seq(rng, e) + stretch + DE._breaker(rng, query, r) + rand_seq(rng, n - e - r - 1)


def _own_products(rng, texts, n=500):
    """One sequence per row with the row's own product planted: the DB is not empty, and no product is spurious."""
    return [CC._seq(rng, n, [(40 + 10 * i, f, r)]) for i, (f, r) in enumerate(texts)]


PLANT_RUN, PLANT_AT = 7, 3
PLANT_EXT = (POOL, 5, 1)


@functools.lru_cache(None)
def planted_case(oracle):
    """Rows (A, B), (C, D), (E, F).  C carries the reverse complement of A's last 7 bases 3 bases in: A extends on C, cell {0, 1}.
    Every row's own product is planted and no other: no pair has a spurious product."""
    rng = random.Random(7101)
    a, b, d, e, f = (_primer(rng, n) for n in (21, 20, 22, 20, 21))
    a = a[:-PLANT_RUN] + "GCAGGCT"[:PLANT_RUN]
    c = _target_of(rng, a, PLANT_RUN, PLANT_AT, 21)
    texts = [(a, b), (c, d), (e, f)]
    w = oracle.centered_word
    return dict(seqs=_own_products(rng, texts), panel=[(w(x), w(y)) for x, y in texts], thr=0.95, select="all", texts=texts)


REPEAT_EXT = (POOL, 3, 1)


@functools.lru_cache(None)
def repeats_case(oracle):
    """Rows (A, B), (C, C), (A, D), (A, B) again, (B, A): a row with F = R, two rows that share an oligo, a repeated and an
    exchanged row; B and D carry the reverse complement of A's last 5 bases, C ends in a palindrome (it extends on itself)."""
    rng = random.Random(7102)
    a = _primer(rng, 21)
    b = _target_of(rng, a, 5, 2, 20)
    c = _primer(rng, 16) + "GAATTC"
    d = _target_of(rng, a, 5, 6, 22)
    texts = [(a, b), (c, c), (a, d), (a, b), (b, a)]
    seqs = _own_products(rng, texts[:3]) + [CC._seq(rng, 500, [(60, a, a)])]
    w = oracle.centered_word
    return dict(seqs=seqs, panel=[(w(x), w(y)) for x, y in texts], thr=0.95, select="all", texts=texts)


TIE_SITE = "GGCC"
TIE_EXT = (POOL, 4, 1)


@functools.lru_cache(None)
def tie_case(oracle):
    """Rows (Q, X), (T1, T2).  T1 and T2 carry the reverse complement of Q's last 4 bases, a base that ends the run behind it:
    under PCR_DIMER_RULE_POOL the cells (Q, T1) and (Q, T2) melt the same two strings at the same concentration.  The seed is
    the first whose pool gives {0, 1} no other placement as good (test_conflict_ext_host asserts what it yields)."""
    w = oracle.centered_word
    for seed in range(7200, 7300):
        rng = random.Random(seed)
        q = _primer(rng, 17) + TIE_SITE
        x = _primer(rng, 20)
        t1 = _target_of(rng, q, 4, 3, 20)
        t2 = _target_of(rng, q, 4, 7, 21)
        texts = [(q, x), (t1, t2)]
        case = dict(seqs=_own_products(rng, texts), panel=[(w(f), w(r)) for f, r in texts], thr=0.95, select="all", texts=texts)
        P = DC.Pool(oracle, case["panel"])
        cells = {(r[0], r[1]): r for r in DE.expected(oracle, P, *TIE_EXT)[0]}
        pair = [cells[c] for c in CC.dimer_cells_of(P.ids, 0, 1) if c in cells]
        low = min(DE.f32(c[11]) for c in pair)
        if sorted((c[0], c[1]) for c in pair if DE.f32(c[11]) == low) == [(0, 2), (0, 3)]:
            return case
    raise AssertionError("no seed gives the tie")


@functools.lru_cache(None)
def degenerate_case(oracle):
    """dimer_end3_cases.expansions_pool as three rows (degeneracies 6, 12, 24, 1, 2, 8) on two random sequences."""
    rng = random.Random(7103)
    return dict(seqs=[rand_seq(rng, 300), rand_seq(rng, 300)], panel=list(DE.expansions_pool(oracle)), thr=1.0, select="all")


DEGENERATE_EXT = {POOL: (POOL, 3, 0), ASSAY: (ASSAY, 3, 0)}

_BUILDERS = {"x_planted": planted_case, "x_repeats": repeats_case, "x_tie": tie_case, "x_degenerate": degenerate_case}
SCENARIOS = tuple(_BUILDERS)


def scenario(oracle, name):
    """name -> scenario, registered with products_tm_cases (pool_conflict_cases' scenarios pass through)."""
    if name in _BUILDERS:
        if name not in PC._CASES:
            PC.register(name, _BUILDERS[name](oracle))
        return PC.scenario(oracle, name)
    return CC.scenario(oracle, name)


def filter_dg(oracle, name, ext):
    """A dg_max for the scenario that keeps some cells and empties a pair: the mean of the two lowest distinct best dG of
    the off-diagonal pairs (rounded to float32)."""
    ids = scenario_ids(oracle, name)
    cell_of = ext_cells_of(oracle, name, *ext)
    n_pool = len(ids) // 2
    best = sorted({float(DE.f32(ext_half(ids, a, b, cell_of, None)[11])) for a in range(n_pool) for b in range(a + 1, n_pool)
                   if ext_half(ids, a, b, cell_of, None)[0]})
    assert len(best) >= 2
    return float(np.float32((best[0] + best[1]) / 2))


def scenario_ids(oracle, name):
    return SC.distinct_oligos(scenario(oracle, name)["panel"])[0]
