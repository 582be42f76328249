"""pcr_pool_anneal_profile_end3, pcr_pool_conflicts_end3 and pcr_pool_probe_hits_end3 on the GPU: the zero rule against the base
entry points on the same handle (bytes), the rules of pool_rule_cases against the composed models (every integer and every
float as bits), the three calls against pcr_pool_products_end3 on the same handle, the TaqMAMA factor against the oracle's
find_target_match, bits on both sides of a 64-sequence word boundary, counting, caps and poisoned buffers, and the wrappers."""
import ctypes as C

import numpy as np
import pytest

import anneal_profile_cases as AP
import end3_cases as E
import pool_conflict_cases as CC
import pool_rule_cases as R
import probe_hit_cases as H
import products_tm_cases as PT
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

POISON_BYTE = 0xA5
BASE = "base"                                    # `rule` of the raw calls: the base entry point; None: the ruled one with rule = NULL


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


@pytest.fixture(scope="module", autouse=True)
def _entry_points():
    L = api.load_library()
    for name in ("pcr_pool_anneal_profile_end3", "pcr_pool_conflicts_end3", "pcr_pool_probe_hits_end3"):
        assert hasattr(L, name), "libpcramp_hip.so does not export " + name


def _case(oracle, name):
    """-> (the scenario with a `probes` key, its name in products_tm_cases): probe_hit_cases' own, or a pool without probes."""
    if name == R.PROBE_ENDS:
        return H.scenario(oracle, R.probe_ends_name(oracle)), name
    return H.scenario(oracle, R.no_probe_name(oracle, name)), name


def _load(d, oracle, case):
    """Sequences, flags, EOS splits and the all-sites word DB of the pool plus (P, P) per probe; the DB is the oracle's."""
    d.load_texts(case["seqs"])
    if case.get("active") is not None:
        d.set_active(case["active"])
    for s, p in list(case.get("splits", ())) + list(case.get("eos", ())):
        d.split(s, p)
    assert case["select"] == "all"
    d.select_sites(H.db_case(case)["panel"], SC.SQ(case["thr"]))
    assert d.entries() == H.db_of(oracle, case)


def _poisoned(shape, dtype):
    a = np.zeros(shape, dtype)
    a.view(np.uint8)[...] = POISON_BYTE
    return a


def _clean(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == POISON_BYTE).all())


def _head(d, case, thr=None):
    cond = SC.conditions_of(case)
    lo, hi = PT.amp_of(case)
    a = W.pairs_array(case["panel"])
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    keep = (a, args)                                                        # (alive while the call runs)
    return keep, a, [float(case["thr"] if thr is None else thr), lo, hi, C.byref(args)]


def _rule_arg(rule):
    if rule is None:
        return None, None
    rs = api.End3Rule(rule["min_clamp3"], rule["window"], rule["max_end_mismatch"], rule["use_taq_mama"], rule["ident_threshold"])
    return rs, C.byref(rs)


def _anneal(d, case, rule, temps, thr=None):
    """-> (return value, [oligo ids, points, pair_sequences, melt_fr, melt_rf, melt_spurious]); every buffer poisoned first."""
    keep, a, head = _head(d, case, thr)
    n_pool, n_seq = len(case["panel"]), len(case["seqs"])
    t = np.ascontiguousarray(temps, np.float32)
    ids = np.zeros(2 * n_pool, np.uint32)
    bufs = [_poisoned(len(t), api.ANNEAL_POINT_DTYPE), _poisoned((n_pool, len(t)), np.uint32), _poisoned((n_pool, n_seq), np.float32),
            _poisoned((n_pool, n_seq), np.float32), _poisoned(n_seq, np.float32)]
    tail = [t.ctypes.data, len(t), ids.ctypes.data] + [b.ctypes.data for b in bufs]
    first = [d.h, api.TARGET, a.ctypes.data, n_pool] + head + [float(case.get("template_strand", 0.0))]
    if rule == BASE:
        n = d.L.pcr_pool_anneal_profile(*first, *tail)
    else:
        rs, ref = _rule_arg(rule)
        n = d.L.pcr_pool_anneal_profile_end3(*first, ref, *tail)
    return n, [ids] + bufs


def _conflicts(d, case, rule, tm_floor=0.0, dimer_rule=CC.NO_DIMERS, dimer_floor=0.0, cap=None):
    """-> (return value, oligo ids, the poisoned buffer of `cap` records (None: every cell and a guard record))."""
    keep, a, head = _head(d, case)
    n_pool = len(case["panel"])
    cap = n_pool * (n_pool + 1) // 2 + 1 if cap is None else cap
    ids = np.zeros(2 * n_pool, np.uint32)
    out = _poisoned(max(cap, 1), api.POOL_CONFLICT_DTYPE)
    first = [d.h, api.TARGET, a.ctypes.data, n_pool] + head + [float(case.get("template_strand", 0.0)), float(tm_floor)]
    tail = [dimer_rule, float(dimer_floor), ids.ctypes.data, out.ctypes.data if cap else None, cap]
    if rule == BASE:
        n = d.L.pcr_pool_conflicts(*first, *tail)
    else:
        rs, ref = _rule_arg(rule)
        n = d.L.pcr_pool_conflicts_end3(*first, ref, *tail)
    return n, ids, out


def _probes(d, case, rule, tm_floor=0.0, probe_tm_floor=0.0, cap=4096, thr=None, want_detected=True):
    """-> (return value, oligo ids, probe ids, the poisoned buffer of `cap` records, detected (poisoned first))."""
    keep, a, head = _head(d, case, thr)
    n_pool = len(case["panel"])
    pr = np.array([(0, 0) if p is None else (int(p[0]), int(p[1])) for p in case["probes"]], np.uint64).reshape(-1, 2)
    ids, pid = np.zeros(2 * n_pool, np.uint32), np.zeros(n_pool, np.uint32)
    out = _poisoned(max(cap, 1), api.PROBE_HIT_DTYPE)
    det = _poisoned((n_pool, (len(case["seqs"]) + 63) // 64), np.uint64)
    first = [d.h, api.TARGET, a.ctypes.data, pr.ctypes.data, n_pool] + head + [float(case.get("probe_strand", H.PROBE_STRAND)),
                                                                              float(case.get("template_strand", 0.0)), float(tm_floor), float(probe_tm_floor)]
    tail = [ids.ctypes.data, pid.ctypes.data, out.ctypes.data if cap else None, cap, det.ctypes.data if want_detected else None]
    if rule == BASE:
        n = d.L.pcr_pool_probe_hits(*first, *tail)
    else:
        rs, ref = _rule_arg(rule)
        n = d.L.pcr_pool_probe_hits_end3(*first, ref, *tail)
    return n, ids, pid, out, det


def _end3(d, case, rule, tm_floor=0.0, thr=None):
    """pool_products_end3 with records and bits on the same handle -> (ids, records, fr, rf)."""
    lo, hi = PT.amp_of(case)
    return d.pool_products_end3(case["panel"], case["thr"] if thr is None else thr, tm_floor=tm_floor, bits=True, amp_min=lo, amp_max=hi,
                                template_strand=case.get("template_strand", 0.0), **rule, **SC.conditions_of(case))[:4]


def _bytes(arrays):
    return [np.ascontiguousarray(x).tobytes() for x in arrays]


def _by_scenario(pairs):
    out = {}
    for name, rule in pairs:
        out.setdefault(name, []).append(rule)
    return out.items()


# ------------------------------------------------------------------ 1. the zero rule is the base call
@pytest.mark.parametrize("name", ["ladder", "end3_ends", R.PROBE_ENDS])
def test_zero_rule(dev, oracle, name):
    if name == "end3_ends":
        name = R.ends_name(oracle)
    case, pt_name = _case(oracle, name)
    _load(dev, oracle, case)
    everything = _end3(dev, case, E.ZERO_RULE)[1]
    temps = AP.temps_of(everything)
    mid = R.floor_of(oracle, pt_name)
    assert 0 < len(_end3(dev, case, E.ZERO_RULE, mid)[1]) < len(everything)
    n0, base = _anneal(dev, case, BASE, temps)
    assert n0 == len(everything) and not any(_clean(b) for b in base[1:])
    for rule in (None, E.ZERO_RULE):
        n, got = _anneal(dev, case, rule, temps)
        assert n == n0 and _bytes(got) == _bytes(base)
    for tm_floor in (0.0, mid):
        for dimer_rule in (CC.NO_DIMERS, api.DIMER_RULE_POOL):
            n0, ids0, out0 = _conflicts(dev, case, BASE, tm_floor, dimer_rule)
            assert n0 >= (1 if dimer_rule != CC.NO_DIMERS or len(case["panel"]) > 1 else 0)
            for rule in (None, E.ZERO_RULE):
                n, ids, out = _conflicts(dev, case, rule, tm_floor, dimer_rule)
                assert n == n0 and _bytes([ids, out]) == _bytes([ids0, out0])
        n0, ids0, pid0, out0, det0 = _probes(dev, case, BASE, tm_floor)
        assert n0 >= (1 if name == R.PROBE_ENDS else 0) and det0.any() and not _clean(det0)
        for rule in (None, E.ZERO_RULE):
            n, ids, pid, out, det = _probes(dev, case, rule, tm_floor)
            assert n == n0 and _bytes([ids, pid, out, det]) == _bytes([ids0, pid0, out0, det0])


# ------------------------------------------------------------------ 2. the rules against the composed models
def test_anneal_rules(dev, oracle):
    for name, rules in _by_scenario(R.triples_of(oracle, "anneal")):
        case, pt_name = _case(oracle, name)
        _load(dev, oracle, case)
        for rule in rules:
            temps = R.anneal_temps(oracle, pt_name, rule)
            want = R.anneal(oracle, pt_name, rule, temps)
            n, got = _anneal(dev, case, rule, temps)
            print("anneal %s %s: %d products, %d temperatures" % (name, R.rule_id(rule), n, len(temps)))
            assert n == want[1] and got[0].tolist() == want[0]
            for what, g, w in zip(("points", "pair_sequences", "melt_fr", "melt_rf", "melt_spurious"), got[1:], want[2:]):
                assert AP.as_words(g) == AP.as_words(w), (name, R.rule_id(rule), what)


def test_conflict_rules(dev, oracle):
    for name, rules in _by_scenario(R.triples_of(oracle, "conflicts")):
        case, pt_name = _case(oracle, name)
        _load(dev, oracle, case)
        for tm_floor in (0.0, R.floor_of(oracle, pt_name)):
            base = {}
            for dimer_rule in (CC.NO_DIMERS, api.DIMER_RULE_POOL):
                n0, _, out0 = _conflicts(dev, case, BASE, tm_floor, dimer_rule)
                base[dimer_rule] = {(int(r["row_a"]), int(r["row_b"])): r for r in out0[:n0]}
            for rule in rules:
                for dimer_rule in (CC.NO_DIMERS, api.DIMER_RULE_POOL):
                    want_ids, want = R.conflicts(oracle, pt_name, rule, tm_floor, dimer_rule)
                    n, ids, out = _conflicts(dev, case, rule, tm_floor, dimer_rule)
                    print("conflicts %s %s floor %.3f dimers %d: %d records" % (name, R.rule_id(rule), tm_floor, dimer_rule, n))
                    assert n == len(want) and ids.tolist() == want_ids
                    assert CC.as_bits(out[:n]) == want, (name, R.rule_id(rule), tm_floor, dimer_rule)
                    assert _clean(out[n:])
                    for r in out[:n]:                                       # the dimer half: the base call's bytes
                        b = base[dimer_rule].get((int(r["row_a"]), int(r["row_b"])))
                        if dimer_rule == CC.NO_DIMERS:
                            assert b is not None and not r["dimer_tm"].view(np.uint32) and not r["dimer_query"] and not r["dimer_target"]
                        else:
                            assert b is not None and [r[f].tobytes() for f in ("dimer_tm", "dimer_query", "dimer_target")] == \
                                [b[f].tobytes() for f in ("dimer_tm", "dimer_query", "dimer_target")]
                            assert (int(r["flags"]) & CC.DIMER) == (int(b["flags"]) & CC.DIMER)


def test_probe_rules(dev, oracle):
    for name, rules in _by_scenario(R.triples_of(oracle, "probes")):
        case, pt_name = _case(oracle, name)
        _load(dev, oracle, case)
        for rule in rules:
            for tm_floor, probe_tm_floor in ((0.0, 0.0), (R.floor_of(oracle, pt_name), 0.0), (0.0, 50.0)):
                want = R.probes(oracle, pt_name, name, rule, tm_floor, probe_tm_floor)
                n, ids, pid, out, det = _probes(dev, case, rule, tm_floor, probe_tm_floor)
                print("probes %s %s floors %.3f %.1f: %d hits" % (name, R.rule_id(rule), tm_floor, probe_tm_floor, n))
                assert n == len(want[2]) and ids.tolist() == want[0] and pid.tolist() == want[1]
                assert H.as_bits(out[:n]) == H.as_bits(want[2]), (R.rule_id(rule), tm_floor, probe_tm_floor)
                assert det.tolist() == want[3].tolist() and _clean(out[n:])


# ------------------------------------------------------------------ 3. the three calls against pcr_pool_products_end3 on the same handle
def test_device_side_consistency(dev, oracle):
    name = R.PROBE_ENDS
    case, pt_name = _case(oracle, name)
    _load(dev, oracle, case)
    n_pool = len(case["panel"])
    for rule in (R.grid_rule((3, 5, 1)), R.ident_rules()[1]):
        assert any(R.rule_id(rule) == R.rule_id(r) for c in ("anneal", "probes") for _, r in R.triples_of(oracle, c))
        ids, rec, fr, rf = _end3(dev, case, rule)
        temps = AP.temps_of(rec)
        n, (a_ids, points, pair_seq, melt_fr, melt_rf, melt_sp) = _anneal(dev, case, rule, temps)
        assert n == len(rec) and a_ids.tolist() == ids.tolist()
        for t, temp in enumerate(temps.tolist()):
            _, rec_t, fr_t, rf_t = _end3(dev, case, rule, temp)
            assert api.melt_to_bits(melt_fr, temp).tolist() == fr_t.tolist() and api.melt_to_bits(melt_rf, temp).tolist() == rf_t.tolist(), temp
            assert int(points[t]["products_intended"]) + int(points[t]["products_spurious"]) == len(rec_t), temp
            assert int(points[t]["products_intended"]) == int((rec_t["intended"] != 0).sum())
        for tm_floor in (0.0, R.floor_of(oracle, pt_name)):
            _, rec_f, fr_f, rf_f = _end3(dev, case, rule, tm_floor)
            # conflicts: the cells of pool_conflict_cases.product_cells over the device's own ruled records
            cells = CC.product_cells(ids.tolist(), rec_f, tm_floor)
            n, _, out = _conflicts(dev, case, rule, tm_floor)
            got = {(int(r["row_a"]), int(r["row_b"])): dict(products=int(r["products"]), sequences=int(r["sequences"]),
                                                            melt_bits=CC.BITS(r["melt"]), melt_sequence=int(r["melt_sequence"])) for r in out[:n]}
            assert got == cells and len(cells) >= 1
            # probes: the row of the pair without a probe is fr | rf; every hit lies in one of the ruled products
            n, _, pid, hits, det = _probes(dev, case, rule, tm_floor)
            assert pid.tolist()[2] == H.NO_PROBE and det[2].tolist() == (fr_f[2] | rf_f[2]).tolist() and det[2].any()
            assert 0 < n and R.keys_of(hits[:n]) <= R.keys_of(rec_f)
    # the ARMS panel: its conflicts are pool_products_end3's spurious products, cell by cell
    case, pt_name = _case(oracle, R.arms_name(oracle))
    _load(dev, oracle, case)
    for rule in (R.grid_rule((1, 1, 0)), R.ident_rules(R.IDENT_ARMS)[1]):
        ids, rec, _, _ = _end3(dev, case, rule)
        n, _, out = _conflicts(dev, case, rule)
        cells = CC.product_cells(ids.tolist(), rec, 0.0)
        assert {(int(r["row_a"]), int(r["row_b"])): int(r["products"]) for r in out[:n]} == {c: v["products"] for c, v in cells.items()} == {(0, 2): 1}


# ------------------------------------------------------------------ 4. the TaqMAMA factor
@pytest.mark.parametrize("use_taq", [0, 1])
def test_taq_mama(dev, oracle, use_taq):
    base, _ = _case(oracle, E.scenario_name(oracle, "taq"))
    _load(dev, oracle, base)
    n_seq = len(base["seqs"])
    seen = set()
    for thr in E.taq_thresholds():
        case, _ = _case(oracle, E.taq_name(oracle, thr))                    # the same sequences and panel, collected at thr
        rule = E.rule_of(use_taq_mama=use_taq, ident_threshold=thr)
        fr, rf = E.oracle_bits(oracle, case, thr, use_taq)
        n, got = _anneal(dev, case, rule, [0.0], thr=thr)
        assert n >= 0 and got[2][:, 0].tolist() == (fr | rf).sum(axis=1).tolist(), thr
        n, _, pid, _, det = _probes(dev, case, rule, thr=thr)
        assert n == 0 and (pid == H.NO_PROBE).all()
        assert E.unpack_bits(det, n_seq).tolist() == (fr | rf).tolist(), thr
        seen.add((fr | rf).tobytes())
    assert len(seen) >= (4 if use_taq else 3)


# ------------------------------------------------------------------ 5. bits on both sides of a word boundary
def test_word_boundary(dev, oracle):
    case, pt_name = _case(oracle, "words")
    _load(dev, oracle, case)
    rule = R.WORDS_RULE
    temps = R.anneal_temps(oracle, pt_name, rule)
    want = R.anneal(oracle, pt_name, rule, temps)
    n, got = _anneal(dev, case, rule, temps)
    assert n == want[1]
    cols = list(R.WORDS_SEQS)
    for g, w in zip(got[3:5], want[4:6]):                                   # melt_fr, melt_rf
        assert AP.as_words(g[:, cols]) == AP.as_words(w[:, cols])
        assert AP.as_words(g) == AP.as_words(w)
    assert AP.as_words(got[5][cols]) == AP.as_words(want[6][cols]) and AP.as_words(got[2]) == AP.as_words(want[3])
    _, _, fr, rf, _ = R.ruled(oracle, pt_name, rule)
    n0, zero = _anneal(dev, case, BASE, temps)
    assert n < n0 and api.melt_to_bits(got[3], 0.0).tolist() == fr.tolist() and api.melt_to_bits(got[4], 0.0).tolist() == rf.tolist()
    lost = api.melt_to_bits(zero[3], 0.0) & ~fr
    assert lost[:, 0].any() and lost[:, 1].any()                            # words 0 and 1 both lose a bit
    n, _, _, _, det = _probes(dev, case, rule)
    assert n == 0 and det.tolist() == (fr | rf).tolist()


# ------------------------------------------------------------------ 6. state, counting, caps, buffers written in full
def test_state_and_caps(dev, oracle):
    name = R.PROBE_ENDS
    case, pt_name = _case(oracle, name)
    _load(dev, oracle, case)
    rule = R.grid_rule((3, 5, 1))
    temps = R.anneal_temps(oracle, pt_name, rule)
    floor = R.floor_of(oracle, pt_name)
    # a ruled call between two base calls
    for base_call, ruled_call in ((lambda: _anneal(dev, case, BASE, temps), lambda: _anneal(dev, case, rule, temps)),
                                  (lambda: _conflicts(dev, case, BASE, floor, api.DIMER_RULE_POOL), lambda: _conflicts(dev, case, rule, floor, api.DIMER_RULE_POOL)),
                                  (lambda: _probes(dev, case, BASE, floor), lambda: _probes(dev, case, rule, floor))):
        first = base_call()
        mid = ruled_call()
        again = base_call()
        assert first[0] == again[0] and _bytes(first[1] if isinstance(first[1], list) else first[1:]) == \
            _bytes(again[1] if isinstance(again[1], list) else again[1:])
        assert mid[0] != first[0] or _bytes(mid[1] if isinstance(mid[1], list) else mid[1:]) != _bytes(first[1] if isinstance(first[1], list) else first[1:])
    # counts and caps
    want = R.conflicts(oracle, pt_name, rule)[1]
    for cap in (0, len(want) - 1, len(want)):
        n, _, out = _conflicts(dev, case, rule, cap=cap)
        assert n == len(want) >= 2, cap
        if cap == 0:
            assert _clean(out)
        elif cap >= n:
            assert CC.as_bits(out[:n]) == want
    hits = R.probes(oracle, pt_name, name, rule)
    for cap in (0, len(hits[2]) - 1, len(hits[2]), len(hits[2]) + 3):
        n, ids, pid, out, det = _probes(dev, case, rule, cap=cap)
        assert n == len(hits[2]) >= 2, cap
        assert det.tolist() == hits[3].tolist()                             # the rows in full whatever the cap
        if cap == 0:
            assert _clean(out)
        elif cap >= n:
            assert H.as_bits(out[:n]) == H.as_bits(hits[2]) and _clean(out[n:])
    n, _, _, _, det = _probes(dev, case, rule, cap=0, want_detected=False)
    assert n == len(hits[2]) and _clean(det)
    # anneal: everything asked for is written in full, also where no product passes the rule on a sequence
    n, got = _anneal(dev, case, rule, temps)
    assert n > 0 and not any((np.ascontiguousarray(b).view(np.uint8).reshape(-1, b.dtype.itemsize) == POISON_BYTE).all(axis=1).any() for b in got[1:])
    assert (got[3][:, 3] == AP.NO_PRODUCT).all()                            # the inactive sequence: written, no product


# ------------------------------------------------------------------ 7. the wrappers
def test_wrappers(dev, oracle):
    name = R.PROBE_ENDS
    case, pt_name = _case(oracle, name)
    _load(dev, oracle, case)
    lo, hi = PT.amp_of(case)
    kw = dict(amp_min=lo, amp_max=hi, template_strand=case.get("template_strand", 0.0), **SC.conditions_of(case))
    rule = R.grid_rule((3, 5, 1))
    temps = R.anneal_temps(oracle, pt_name, rule)
    floor = R.floor_of(oracle, pt_name)
    # the defaults: what they return today (the base entry point)
    n, base = _anneal(dev, case, BASE, temps)
    assert _bytes(dev.anneal_profile(case["panel"], temps, case["thr"], melt=True, **kw)) == _bytes(base)
    assert _bytes(dev.anneal_profile(case["panel"], temps, case["thr"], melt=True, **kw, **E.ZERO_RULE)) == _bytes(base)
    n, ids, out = _conflicts(dev, case, BASE, floor, api.DIMER_RULE_POOL)
    assert _bytes(dev.pool_conflicts(case["panel"], case["thr"], tm_floor=floor, **kw)) == _bytes([ids, out[:n]])
    n, ids, pid, out, det = _probes(dev, case, BASE, floor)
    assert _bytes(dev.probe_hits(case["panel"], case["probes"], case["thr"], tm_floor=floor, bits=True, probe_strand=H.PROBE_STRAND, **kw)) == \
        _bytes([ids, pid, out[:n], det])
    # with a rule: the C call's results
    r = dict(rule, use_taq_mama=bool(rule["use_taq_mama"]))
    n, ruled = _anneal(dev, case, rule, temps)
    got = dev.anneal_profile(case["panel"], temps, case["thr"], melt=True, **kw, **r)
    assert _bytes(got) == _bytes(ruled) and _bytes(got) != _bytes(base)
    n, ids, out = _conflicts(dev, case, rule, floor, api.DIMER_RULE_POOL)
    assert _bytes(dev.pool_conflicts(case["panel"], case["thr"], tm_floor=floor, **kw, **r)) == _bytes([ids, out[:n]])
    n, ids, pid, out, det = _probes(dev, case, rule, floor)
    for cap in (1 << 16, 1):                                                # (a cap that grows)
        got = dev.probe_hits(case["panel"], case["probes"], case["thr"], tm_floor=floor, bits=True, cap=cap, probe_strand=H.PROBE_STRAND, **kw, **r)
        assert _bytes(got) == _bytes([ids, pid, out[:n], det])
    with pytest.raises(api.PcrError, match="pcr_pool_conflicts_end3: window"):
        dev.pool_conflicts(case["panel"], case["thr"], window=40, **kw)
