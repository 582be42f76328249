"""pcr_pool_conflicts_ext without a device: the record layout, the refusals that come before the handle and their order,
conflict_matrix with both record types, and whether conflict_ext_cases' scenarios show what the GPU tests use them for (read
off the oracle alone)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import conflict_ext_cases as X
import dimer_end3_cases as DE
import pool_conflict_cases as CC
import site_tm_cases as SC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1
NAME = "pcr_pool_conflicts_ext"
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


# ------------------------------------------------------------------ the ABI
def test_record_layout():
    dt = api.POOL_CONFLICT_EXT_DTYPE
    assert dt.itemsize == 96 and C.sizeof(api.DimerEnd3Args) == 16
    assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == list(X.LAYOUT)
    base = api.POOL_CONFLICT_DTYPE
    assert dt.names[:len(base.names)] == base.names                          # the first fields are pcr_pool_conflict's ...
    assert all(dt.fields[n] == base.fields[n] for n in base.names)           # ... at their offsets, with their types
    assert dt.names[len(base.names):] == X.EXT_FIELDS
    cell = api.POOL_DIMER_END3_DTYPE                                         # ext_q_expansion .. ext_dS: that record's tail, as it lies there
    tail = [n for n in cell.names if n not in ("query_oligo", "target_oligo", "n_duplexes", "n_placements")]
    assert ["ext_" + n for n in tail] == list(X.EXT_FIELDS[4:])
    assert all(dt.fields["ext_" + n][1] - dt.fields["ext_q_expansion"][1] == cell.fields[n][1] - cell.fields["q_expansion"][1] and
               dt.fields["ext_" + n][0] == cell.fields[n][0] for n in tail)
    assert api.CONFLICT_EXTENSION == 4 == X.EXTENSION
    assert [f[0] for f in api.DimerEnd3Args._fields_] == ["rule", "min_run", "min_extension", "dg_max"]


def test_symbol_and_prototype(lib):
    assert NAME in api.ABI_SYMBOLS and hasattr(lib, NAME), "libpcramp_hip.so does not export " + NAME
    fn, base = lib.pcr_pool_conflicts_ext, lib.pcr_pool_conflicts_end3
    assert fn.restype is C.c_int64
    at = list(fn.argtypes).index(C.POINTER(api.DimerEnd3Args))
    assert at == 13 and list(fn.argtypes[:at]) + list(fn.argtypes[at + 1:]) == list(base.argtypes)   # pcr_pool_conflicts_end3's, plus ext
    par = inspect.signature(api.Screener.pool_conflicts).parameters
    assert [(k, par[k].default) for k in ("ext_min_run", "ext_min_extension", "ext_dg_max", "ext_rule")] == \
        [("ext_min_run", 0), ("ext_min_extension", 1), ("ext_dg_max", None), ("ext_rule", None)]
    assert inspect.signature(api.conflict_matrix).parameters["max_extension_dg"].default is None


# ------------------------------------------------------------------ the refusals
def _refused(lib, oracle, pool=None, which=api.TARGET, null_args=False, salt=0.05, primer_strand=9e-7, template_strand=0.0, tm_floor=0.0,
             n_pool=None, out_cap=0, dimer_rule=CC.NO_DIMERS, dimer_floor=0.0, rule=None, ext=(api.DIMER_RULE_POOL, 4, 1, INF)):
    """The call on a NULL handle -> (return value, message).  rule: End3Rule fields or None; ext: the four fields or None."""
    w = oracle.centered_word
    pool = [(w("ACGTTGCAAGCTTGCATGCA"), w("TTGACCGTAGGCTAGCTAAC"))] if pool is None else pool
    a = W.pairs_array(pool)
    n = len(pool) if n_pool is None else n_pool
    ids = np.zeros(max(2 * len(pool), 1), np.uint32)
    args = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    rs = None if rule is None else api.End3Rule(*rule)
    xs = None if ext is None else api.DimerEnd3Args(*ext)
    rc = lib.pcr_pool_conflicts_ext(None, which, a.ctypes.data, n, 0.9, 80, 200, None if null_args else C.byref(args), template_strand, tm_floor,
                                    None if rs is None else C.byref(rs), dimer_rule, dimer_floor, None if xs is None else C.byref(xs),
                                    ids.ctypes.data, None, out_cap)
    return rc, api._err(lib)


BAD_RULE = (0, 33, 0, 2, 2.0)                    # window, use_taq_mama and ident_threshold, all refused
BAD_EXT = (7, 2, 40, NAN)                        # rule, min_run, min_extension and dg_max, all refused
# every case breaks one check and every later one as well
STEPS = [
    (dict(which=7, salt=2.0, tm_floor=NAN, dimer_rule=5), "unknown sequence set"),
    (dict(which=api.MULTIPLEX, salt=2.0, tm_floor=NAN, dimer_rule=5), "PCR_SET_MULTIPLEX"),
    (dict(out_cap=5, salt=2.0, tm_floor=NAN, dimer_rule=5), "bad argument"),
    (dict(n_pool=api.POOL_MAX_PAIRS + 1, salt=2.0, tm_floor=NAN, dimer_rule=5), "PCR_POOL_MAX_PAIRS"),
    (dict(primer_strand=-1.0, salt=2.0, tm_floor=NAN, dimer_rule=5), "negative strand concentration"),
    (dict(salt=2.0, tm_floor=NAN, dimer_rule=5), "salt outside"),
    (dict(primer_strand=0.0, tm_floor=NAN, dimer_rule=5), "strand concentration of an oligo's duplex is zero"),
    (dict(tm_floor=NAN, dimer_rule=5), "tm_floor is not finite"),
    (dict(dimer_rule=5, dimer_floor=NAN), "unknown dimer_rule"),
    (dict(dimer_rule=api.DIMER_RULE_POOL, dimer_floor=NAN, primer_strand=0.0, template_strand=1e-7), "dimer_floor is not finite"),
    (dict(dimer_rule=api.DIMER_RULE_POOL, primer_strand=0.0, template_strand=1e-7), "with a dimer rule primer_strand must be positive"),
    (dict(rule=BAD_RULE), "window, min_clamp3 or max_end_mismatch above 32"),
    (dict(rule=(0, 0, 0, 2, 2.0)), "use_taq_mama is neither 0 nor 1"),
    (dict(rule=(0, 0, 0, 0, 2.0)), "ident_threshold is not finite or outside [0, 1]"),
]
EXT_STEPS = [
    (dict(ext=BAD_EXT, primer_strand=0.0, template_strand=1e-7), "unknown ext->rule"),
    (dict(ext=(2, 2, 40, NAN), primer_strand=0.0, template_strand=1e-7), "unknown ext->rule"),
    (dict(ext=(api.DIMER_RULE_ASSAY, 2, 40, NAN), primer_strand=0.0, template_strand=1e-7), "ext->min_run outside 3 .. 32"),
    (dict(ext=(api.DIMER_RULE_ASSAY, 33, 40, NAN), primer_strand=0.0, template_strand=1e-7), "ext->min_run outside 3 .. 32"),
    (dict(ext=(api.DIMER_RULE_POOL, 3, 32, NAN), primer_strand=0.0, template_strand=1e-7), "ext->min_extension above 31"),
    (dict(ext=(api.DIMER_RULE_POOL, 32, 31, NAN), primer_strand=0.0, template_strand=1e-7), "ext->dg_max is not a number"),
    (dict(ext=(api.DIMER_RULE_POOL, 32, 0, -INF), primer_strand=0.0, template_strand=1e-7), "with ext primer_strand must be positive"),
    (dict(ext=(api.DIMER_RULE_POOL, 4, 1, INF)), "null handle"),
    (dict(ext=(api.DIMER_RULE_ASSAY, 3, 0, -5.0), dimer_rule=api.DIMER_RULE_POOL, rule=(32, 32, 32, 1, 1.0)), "null handle"),
    (dict(ext=None), "null handle"),
    (dict(ext=None, out_cap=0, rule=(0, 0, 0, 0, 0.0)), "null handle"),
]


def test_refusals_in_order(lib, oracle):
    """Every PCR_ERR_ARG on a NULL handle: pcr_pool_conflicts_end3's checks in its order, then ext's, then the handle."""
    late = dict(rule=BAD_RULE, ext=BAD_EXT)
    for kw, what in [(dict(late, **k), w) for k, w in STEPS[:11]] + [(dict(k, ext=BAD_EXT), w) for k, w in STEPS[11:]] + EXT_STEPS:
        rc, msg = _refused(lib, oracle, **kw)
        assert rc == PCR_ERR_ARG and what in msg and msg.startswith(NAME + ": "), (kw, msg)


def test_underflow_is_under_the_ext_rule(lib, oracle):
    """primer_strand / degeneracy underflows for a degenerate oligo under PCR_DIMER_RULE_ASSAY only; dimer_rule has no say."""
    w = oracle.centered_word
    pool = [(w("ACGTTGCAAGCTTGCATGCN"), w("TTGACCGTAGGCTAGCTAAC"))]
    tiny = float(np.float32(1.5e-45))                                        # the smallest float32: a quarter of it is zero
    kw = dict(pool=pool, primer_strand=tiny, template_strand=1e-7)
    rc, msg = _refused(lib, oracle, ext=(api.DIMER_RULE_ASSAY, 4, 1, INF), **kw)
    assert rc == PCR_ERR_ARG and "primer_strand / degeneracy underflows to zero" in msg and msg.startswith(NAME)
    rc, msg = _refused(lib, oracle, ext=(api.DIMER_RULE_POOL, 4, 1, INF), **kw)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _refused(lib, oracle, ext=None, **kw)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _refused(lib, oracle, pool=[(SC.too_degenerate_oligo(oracle), pool[0][1])], rule=BAD_RULE, ext=BAD_EXT)
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg             # the oligos come before both


# ------------------------------------------------------------------ conflict_matrix
def test_conflict_matrix_with_both_record_types():
    ext = np.zeros(5, api.POOL_CONFLICT_EXT_DTYPE)
    ext["row_a"], ext["row_b"] = [0, 0, 1, 2, 3], [1, 2, 3, 2, 3]
    ext["products"] = [1, 0, 0, 0, 0]
    ext["melt"] = [60.0, -1.0, -1.0, -1.0, -1.0]
    ext["dimer_tm"] = [10.0, 45.0, 10.0, 10.0, 10.0]
    ext["flags"] = [api.CONFLICT_PRODUCT, api.CONFLICT_DIMER, api.CONFLICT_EXTENSION, api.CONFLICT_EXTENSION, 0]
    ext["ext_cells"] = [0, 0, 1, 2, 0]
    ext["ext_dG"] = [0.0, 0.0, -5.0, -2.0, -9.0]                             # (the last has no flag: its dG is not read)
    plain = np.zeros(5, api.POOL_CONFLICT_DTYPE)
    for f in api.POOL_CONFLICT_DTYPE.names:
        plain[f] = ext[f]
    cells = lambda m: sorted((int(a), int(b)) for a, b in zip(*np.nonzero(np.triu(m))))
    for rec in (plain, ext):                                                 # what it always did, with either type
        assert cells(api.conflict_matrix(rec, 4)) == [(0, 1)]
        assert cells(api.conflict_matrix(rec, 4, max_dimer=40.0)) == [(0, 1), (0, 2)]
        assert cells(api.conflict_matrix(rec, 4, anneal=65.0, max_dimer=40.0)) == [(0, 2)]
        m = api.conflict_matrix(rec, 4, max_dimer=40.0)
        assert m.dtype == bool and (m == m.T).all()
    assert cells(api.conflict_matrix(ext, 4, max_extension_dg=-3.0)) == [(0, 1), (1, 3)]
    assert cells(api.conflict_matrix(ext, 4, max_extension_dg=-2.0)) == [(0, 1), (1, 3), (2, 2)]      # <=, in float32
    assert cells(api.conflict_matrix(ext, 4, max_extension_dg=np.nextafter(np.float32(-2.0), np.float32(-3.0)))) == [(0, 1), (1, 3)]
    assert cells(api.conflict_matrix(ext, 4, anneal=65.0, max_dimer=40.0, max_extension_dg=0.0)) == [(0, 2), (1, 3), (2, 2)]
    m = api.conflict_matrix(ext, 4, max_extension_dg=-3.0)
    assert (m == m.T).all() and m[3, 1]
    with pytest.raises(ValueError, match="max_extension_dg"):
        api.conflict_matrix(plain, 4, max_extension_dg=-3.0)
    with pytest.raises(ValueError, match="max_extension_dg"):
        api.conflict_matrix(plain[:0], 4, max_extension_dg=-3.0)
    assert not api.conflict_matrix(ext[:0], 4, max_extension_dg=-3.0).any()
    tube, _ = api.assign_tubes(api.conflict_matrix(ext, 4, max_extension_dg=-3.0))
    assert tube[0] != tube[1] and tube[1] != tube[3]


# ------------------------------------------------------------------ the join's order, on made-up records
def test_join_order_on_the_expected_side():
    """Equal dG and unequal runs do not arise from the engine (no scenario's oracle yields one): the rule is held on the model."""
    rec = lambda q, t, run, dg: (q, t, 1, 1, 0, 0, run, 1, run, run, 0, CC.BITS(dg), 0, 0, 0)
    ids = [0, 1, 2, 3]
    pick = lambda cells: X.ext_half(ids, 0, 1, {(c[0], c[1]): c for c in cells}, None)[2:4]
    assert pick([rec(0, 2, 4, -3.0), rec(0, 3, 5, -3.0)]) == (0, 3)         # the longer run at equal dG
    assert pick([rec(0, 2, 5, -3.0), rec(0, 3, 4, -3.0)]) == (0, 2)
    assert pick([rec(0, 3, 4, -3.0), rec(2, 0, 4, -3.0), rec(1, 2, 4, -3.0)]) == (0, 3)   # the lowest (q, t) on a full tie
    assert pick([rec(0, 2, 9, -3.0), rec(3, 1, 3, -3.5)]) == (3, 1)         # dG first
    assert X.ext_half(ids, 0, 1, {(0, 2): rec(0, 2, 4, -3.0), (0, 3): rec(0, 3, 4, -1.0)}, -2.0)[:4] == (1, 2, 0, 2)
    assert X.ext_half(ids, 0, 1, {(0, 2): rec(0, 2, 4, -3.0)}, -3.5) == (0, 1) + (0,) * 13


# ------------------------------------------------------------------ the scenarios
def _pairs(ids):
    n = len(ids) // 2
    return [(a, b) for a in range(n) for b in range(a, n)]


def test_scenarios_show_their_case(oracle):
    # planted: {0, 1} extends, has no product, and the whole oligos melt far below 40 C; rows 1 and 2 have nothing
    ids, rec = X.expected(oracle, "x_planted", 0.0, X.POOL, 0.0, X.PLANT_EXT + (None,))
    by = {(r[0], r[1]): r for r in rec}
    p = by[(0, 1)]
    assert p[2] == 0 and p[4] == CC.NO_PRODUCT_BITS and p[11] >= 1 and (p[13], p[14]) == (0, 2)
    assert (p[17], p[18]) == (X.PLANT_RUN, X.PLANT_AT) and DE.f32(p[22]) < -5.0
    assert all(r[2] == 0 for r in rec) and all(CC.F32(r[6]) < 40.0 for r in rec)
    assert [k for k, r in by.items() if k[0] != k[1] and r[11] and DE.f32(r[22]) <= -5.0] == [(0, 1)]
    assert by[(1, 2)][11] == 0 and by[(1, 2)][12] == 0
    only = X.expected(oracle, "x_planted", 0.0, X.NO_DIMERS, 0.0, X.PLANT_EXT + (None,))[1]
    assert (0, 1) in {(r[0], r[1]) for r in only} and all(r[9] == X.EXTENSION for r in only)   # kept through ext alone
    assert X.expected(oracle, "x_planted")[1] == []                          # ... and by nothing else
    # repeats: every kind of repeat in the list of eight, with placements to count twice if one is careless
    ids, rec = X.expected(oracle, "x_repeats", 0.0, X.NO_DIMERS, 0.0, X.REPEAT_EXT + (None,))
    assert ids == [0, 1, 2, 2, 0, 3, 0, 1, 1, 0]
    by = {(r[0], r[1]): r for r in rec}
    cell_of = X.ext_cells_of(oracle, "x_repeats", *X.REPEAT_EXT)
    for pair, distinct in (((0, 0), 4), ((1, 1), 1), ((0, 1), 4), ((0, 2), 7), ((0, 3), 4), ((0, 4), 4), ((3, 4), 4), ((2, 2), 4), ((1, 2), 4)):
        eight = X.eight_cells(ids, *pair)
        assert len(eight) == 8 and len(set(eight)) == distinct < 8 and pair in by
        naive = sum(cell_of[c][3] for c in eight if c in cell_of)
        assert by[pair][12] > 0 and naive > by[pair][12]                     # counting all eight would overcount
    assert any(r[2] > 0 and r[11] > 0 for r in rec) and any(r[2] == 0 and r[11] > 0 for r in rec)   # with and without a product
    # tie: two distinct cells with equal (dG, run), both the best of {0, 1}; the lower (q, t) is reported
    ids, rec = X.expected(oracle, "x_tie", 0.0, X.NO_DIMERS, 0.0, X.TIE_EXT + (None,))
    cell_of = X.ext_cells_of(oracle, "x_tie", *X.TIE_EXT)
    a, b = cell_of[(0, 2)], cell_of[(0, 3)]
    assert a[11:] == b[11:] and a[6] == b[6] == 4 and (a[7], b[7]) == (3, 7)
    others = [cell_of[c] for c in CC.dimer_cells_of(ids, 0, 1) if c in cell_of and c not in ((0, 2), (0, 3))]
    assert all(DE.f32(c[11]) > DE.f32(a[11]) for c in others)
    r = {(r[0], r[1]): r for r in rec}[(0, 1)]
    assert (r[13], r[14], r[18]) == (0, 2, 3) and r[11] >= 2
    # degenerate: cells of many duplexes, best placements in expansions other than the first
    for rule in (X.POOL, X.ASSAY):
        ids, rec = X.expected(oracle, "x_degenerate", 0.0, X.NO_DIMERS, 0.0, X.DEGENERATE_EXT[rule] + (None,))
        assert len(rec) == 6 and any(r[15] > 0 and r[16] > 0 for r in rec) and max(r[12] for r in rec) > 100
    tm_of = lambda rule: [r[23] for r in X.expected(oracle, "x_degenerate", 0.0, X.NO_DIMERS, 0.0, X.DEGENERATE_EXT[rule] + (None,))[1]]
    assert tm_of(X.POOL) != tm_of(X.ASSAY)                                   # the two rules melt at different concentrations


def test_filter_scenario_shows_its_case(oracle):
    ext = X.REPEAT_EXT
    dg = X.filter_dg(oracle, "x_repeats", ext)
    ids, all_rec = X.expected(oracle, "x_repeats", 0.0, X.NO_DIMERS, 0.0, ext + (None,))
    _, cut = X.expected(oracle, "x_repeats", 0.0, X.NO_DIMERS, 0.0, ext + (dg,))
    _, cut_d = X.expected(oracle, "x_repeats", 0.0, X.POOL, 0.0, ext + (dg,))
    full = {(r[0], r[1]): r for r in all_rec}
    have, have_d = {(r[0], r[1]): r for r in cut}, {(r[0], r[1]): r for r in cut_d}
    gone = [k for k in full if k not in have]
    assert gone and all(full[k][12] > 0 and full[k][2] == 0 for k in gone)   # qualifying placements, all above dg_max, no product
    assert all(have_d[k][11] == 0 and have_d[k][12] == full[k][12] and have_d[k][13:] == (0,) * 13 for k in gone)   # ... kept by the dimers
    assert any(r[11] > 0 for r in cut) and len(have_d) == len(_pairs(ids))
    assert any(0 < r[11] < full[(r[0], r[1])][11] for r in cut)              # a pair that loses some of its cells only
    # below every dG: the pairs with a product stay, with ext_cells = 0 and their placements still counted
    _, low = X.expected(oracle, "x_repeats", 0.0, X.NO_DIMERS, 0.0, ext + (-30.0,))
    assert low and all(r[2] > 0 and r[11] == 0 and r[9] == CC.PRODUCT for r in low) and any(r[12] > 0 for r in low)
    # with dg_max = +inf every pair with a qualifying placement has a record
    cell_of = X.ext_cells_of(oracle, "x_repeats", *ext)
    with_placement = [p for p in _pairs(ids) if any(c in cell_of for c in X.eight_cells(ids, *p))]
    assert sorted(full) == with_placement


def test_model_against_brute_force(oracle):
    for name, ext in (("x_repeats", X.REPEAT_EXT), ("x_planted", X.PLANT_EXT), ("x_tie", X.TIE_EXT), ("x_degenerate", X.DEGENERATE_EXT[X.ASSAY])):
        ids = X.scenario_ids(oracle, name)
        cell_of = X.ext_cells_of(oracle, name, *ext)
        for dg in (None, X.filter_dg(oracle, name, ext) if name in ("x_repeats", "x_degenerate") else -2.5):
            for a, b in _pairs(ids):
                assert X.ext_half(ids, a, b, cell_of, dg)[:2] == X.ext_half_brute(ids, a, b, cell_of, dg), (name, a, b)
