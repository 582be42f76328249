"""pcr_pool_anneal_profile / Screener.anneal_profile on the GPU: points, pair_sequences, both melt matrices and the spurious
vector against anneal_profile_cases (the oracle's products, the definitions restated in numpy), every float as bits; and
against pcr_pool_products_tm on the same device at every temperature."""
import ctypes as C

import numpy as np
import pytest

import anneal_profile_cases as AC
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

pytestmark = pytest.mark.gpu

PCR_ERR_STATE = -3
GUARD = 8                                        # poisoned elements behind every output buffer
POISON_BYTE = 0xA5


@pytest.fixture(scope="module")
def dev():
    d = api.Screener(0)
    yield d
    d.close()


def _load(d, oracle, case, which=api.TARGET):
    """The scenario's sequences, flags, splits and word DB on the device; the DB must be the one the oracle expects."""
    d.load_texts(case["seqs"], which=which)
    if case.get("active") is not None:
        d.set_active(case["active"], which=which)
    for s, p in case.get("splits", ()):
        d.split(s, p, which=which)
    thr2 = SC.SQ(case["thr"])
    if case["select"] == "all":
        d.select_sites(case["panel"], thr2, which=which)
    else:
        d.select_words(case["panel"], thr2, which=which)
    assert d.entries(which=which) == SC.db_of(oracle, case)


def _run(d, case, temps, which=api.TARGET, **kw):
    lo, hi = PC.amp_of(case)
    return d.anneal_profile(case["panel"], temps, case["thr"], template_strand=case.get("template_strand", 0.0), amp_min=lo,
                            amp_max=hi, which=which, **SC.conditions_of(case), **kw)


def _poisoned(n, dtype):
    a = np.zeros(n + GUARD, dtype)
    a.view(np.uint8)[:] = POISON_BYTE
    return a


def _raw(d, case, temps, want=("pair_seq", "fr", "rf", "spur"), which=api.TARGET):
    """The C call with poisoned, guarded buffers; the outputs not in `want` are passed as NULL.
    -> (return value, dict of the written parts, dict of the guards)"""
    n_pool, n_seq, n_t = len(case["panel"]), len(case["seqs"]), len(temps)
    a = W.pairs_array(case["panel"])
    t = np.ascontiguousarray(temps, np.float32)
    cond = SC.conditions_of(case)
    args = api.ThermoArgs(cond["salt"], cond["primer_strand"], 0.0, 0.0, 0.0, 0.0)
    lo, hi = PC.amp_of(case)
    size = dict(ids=(2 * n_pool, np.uint32), points=(n_t, api.ANNEAL_POINT_DTYPE), pair_seq=(n_pool * n_t, np.uint32),
                fr=(n_pool * n_seq, np.float32), rf=(n_pool * n_seq, np.float32), spur=(n_seq, np.float32))
    buf = {k: _poisoned(n, dt) for k, (n, dt) in size.items()}
    ptr = lambda k: buf[k].ctypes.data if k in want or k in ("ids", "points") else None
    n = d.L.pcr_pool_anneal_profile(d.h, which, a.ctypes.data, n_pool, float(case["thr"]), lo, hi, C.byref(args),
                                    float(case.get("template_strand", 0.0)), t.ctypes.data, n_t, ptr("ids"), ptr("points"),
                                    ptr("pair_seq"), ptr("fr"), ptr("rf"), ptr("spur"))
    out = {k: buf[k][:size[k][0]] for k in buf}
    guards = {k: buf[k][size[k][0]:] for k in buf}
    return n, out, guards


def _same(got, want, what):
    g, w = AC.as_words(got), AC.as_words(want)
    assert len(g) == len(w), what
    for k, (a, b) in enumerate(zip(g, w)):
        assert a == b, (what, k, a, b)


def _check(oracle, name, temps, ids, points, pair_seq, fr, rf, spur):
    """Everything a call returned against the expectation, floats as bits."""
    want_ids = PC.all_products(oracle, name)[0]
    w_points, w_pair_seq, w_fr, w_rf, w_spur = AC.expected(oracle, name, temps)
    assert np.asarray(ids).tolist() == want_ids
    for field in api.ANNEAL_POINT_DTYPE.names:
        _same(points[field], w_points[field], "points." + field)
    assert not points["reserved"].any()
    _same(pair_seq, w_pair_seq, "pair_sequences")
    _same(fr, w_fr, "melt_fr")
    _same(rf, w_rf, "melt_rf")
    _same(spur, w_spur, "melt_spurious")


# ------------------------------------------------------------------ 1. every scenario against the expectation
@pytest.mark.parametrize("name", PC.SCENARIO_NAMES)
def test_scenario(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    rec = PC.all_products(oracle, name)[1]
    temps = AC.temps_of(rec)
    n, out, guards = _raw(dev, case, temps)
    assert n == len(rec)
    _check(oracle, name, temps, out["ids"], out["points"], out["pair_seq"], out["fr"], out["rf"], out["spur"])
    assert all((g.view(np.uint8) == POISON_BYTE).all() for g in guards.values())
    ids, points, pair_seq, fr, rf, spur = _run(dev, case, temps, melt=True)        # the wrapper: the same, shaped
    assert fr.shape == rf.shape == (len(case["panel"]), len(case["seqs"])) and spur.shape == (len(case["seqs"]),)
    assert pair_seq.shape == (len(case["panel"]), len(temps)) and points.dtype == api.ANNEAL_POINT_DTYPE
    _check(oracle, name, temps, ids, points, pair_seq, fr, rf, spur)
    assert len(_run(dev, case, temps)) == 3


# ------------------------------------------------------------------ 2. against pcr_pool_products_tm on the device
def _products_tm_bits(d, case, tm_floor):
    n_pool, words = len(case["panel"]), int(d.bitset_words())
    a = W.pairs_array(case["panel"])
    ids = np.zeros(2 * n_pool, np.uint32)
    args = api.ThermoArgs(SC.SALT, SC.PRIMER_STRAND, 0.0, 0.0, 0.0, 0.0)
    lo, hi = PC.amp_of(case)
    fr, rf = np.zeros((n_pool, words), np.uint64), np.zeros((n_pool, words), np.uint64)
    n = d.L.pcr_pool_products_tm(d.h, api.TARGET, a.ctypes.data, n_pool, float(case["thr"]), lo, hi, C.byref(args),
                                 float(case.get("template_strand", 0.0)), float(tm_floor), ids.ctypes.data, None, 0,
                                 fr.ctypes.data, rf.ctypes.data)
    return n, fr, rf


@pytest.mark.parametrize("name", ["ladder", "words", "pairs", "random"])
def test_every_temperature_is_pool_products_tm_at_that_floor(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    temps = AC.temps_of(PC.all_products(oracle, name)[1])
    ids, points, pair_seq, fr, rf, spur = _run(dev, case, temps, melt=True)
    for t, temp in enumerate(temps):
        n, want_fr, want_rf = _products_tm_bits(dev, case, float(temp))
        assert n == int(points[t]["products_intended"]) + int(points[t]["products_spurious"]), float(temp)
        assert api.melt_to_bits(fr, temp).tolist() == want_fr.tolist(), float(temp)
        assert api.melt_to_bits(rf, temp).tolist() == want_rf.tolist(), float(temp)
        both = want_fr | want_rf
        pop = [sum(bin(int(w)).count("1") for w in row) for row in both]
        assert pop == pair_seq[:, t].tolist() and sum(pop) == int(points[t]["cells"]), float(temp)


# ------------------------------------------------------------------ 3. whatever is NULL
@pytest.mark.parametrize("name", ["pairs", "random"])
def test_whatever_is_null(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    rec = PC.all_products(oracle, name)[1]
    temps = AC.temps_of(rec)
    everything = ("pair_seq", "fr", "rf", "spur")
    n_all, full, _ = _raw(dev, case, temps)
    _check(oracle, name, temps, full["ids"], full["points"], full["pair_seq"], full["fr"], full["rf"], full["spur"])
    for absent in [(k,) for k in everything] + [("fr", "rf"), everything]:
        want = tuple(k for k in everything if k not in absent)
        n, out, guards = _raw(dev, case, temps, want=want)
        assert n == n_all == len(rec), absent
        for k in ("ids", "points") + want:
            assert out[k].tobytes() == full[k].tobytes(), (absent, k)
        for k in absent:                                                        # a NULL output's stand-in was never written
            assert (out[k].view(np.uint8) == POISON_BYTE).all(), (absent, k)
        assert all((g.view(np.uint8) == POISON_BYTE).all() for g in guards.values()), absent


# ------------------------------------------------------------------ 4. one temperature, and PCR_ANNEAL_MAX_TEMPS of them
@pytest.mark.parametrize("name", ["ladder", "random"])
def test_one_and_256_temperatures(dev, oracle, name):
    case = PC.scenario(oracle, name)
    _load(dev, oracle, case)
    rec = PC.all_products(oracle, name)[1]
    big = AC.ladder_temps(rec)
    assert len(big) == api.ANNEAL_MAX_TEMPS
    v = np.unique(AC.melt_values(rec))
    for temps in (big, big[:1], big[-1:], np.array([v[len(v) // 2]], np.float32)):
        n, out, guards = _raw(dev, case, temps)
        assert n == len(rec)
        _check(oracle, name, temps, out["ids"], out["points"], out["pair_seq"], out["fr"], out["rf"], out["spur"])
        assert all((g.view(np.uint8) == POISON_BYTE).all() for g in guards.values())
    points = AC.expected(oracle, name, big)[0]
    total = points["products_intended"] + points["products_spurious"]
    assert total[0] == len(rec) and total[-1] == 0 and len(set(total.tolist())) >= min(len(v), 100)   # both ends of the search and many bins


# ------------------------------------------------------------------ 5. inactive sequences, many threads one cell
def test_inactive_sequences_and_many_threads_one_cell(dev, oracle):
    case = PC.scenario(oracle, "words")
    _load(dev, oracle, case)
    rec = PC.all_products(oracle, "words")[1]
    temps = AC.temps_of(rec)
    ids, points, pair_seq, fr, rf, spur = _run(dev, case, temps, melt=True)
    _check(oracle, "words", temps, ids, points, pair_seq, fr, rf, spur)
    sentinel = int(np.float32(-1.0).view(np.uint32))
    for s in PC.WORDS_INACTIVE + PC.WORDS_NO_SITE:
        assert fr[:, s].view(np.uint32).tolist() == [sentinel] * 3 and rf[:, s].view(np.uint32).tolist() == [sentinel] * 3
        assert int(spur[s:s + 1].view(np.uint32)[0]) == sentinel
    block = rec[rec["sequence"] == PC.WORDS_BLOCK]
    assert len(block) >= 64
    cells = [(i, o) for i in range(3) for o, m in enumerate((fr, rf)) if m[i, PC.WORDS_BLOCK] >= 0]
    assert cells == [(0, 0)]                                                    # one cell, fed by all of them
    assert fr[0:1, PC.WORDS_BLOCK].view(np.uint32)[0] == AC.melt_values(block).max().view(np.uint32)


# ------------------------------------------------------------------ 6. the background set
@pytest.mark.parametrize("name", ["ids", "pairs"])
def test_background(oracle, name):
    case = PC.scenario(oracle, name)
    d = api.Screener(0)
    try:
        _load(d, oracle, case, which=api.BACKGROUND)
        temps = AC.temps_of(PC.all_products(oracle, name)[1])
        n, out, _ = _raw(d, case, temps, which=api.BACKGROUND)
        assert n == len(PC.all_products(oracle, name)[1])
        _check(oracle, name, temps, out["ids"], out["points"], out["pair_seq"], out["fr"], out["rf"], out["spur"])
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case, temps)                                                # the target set has none
    finally:
        d.close()


# ------------------------------------------------------------------ 7. state, resources, determinism
def test_state_errors_other_calls_and_resources(oracle):
    case = PC.scenario(oracle, "ids")
    rec = PC.all_products(oracle, "ids")[1]
    temps = AC.temps_of(rec)
    panel = case["panel"]
    held = api.live_resources()
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        if case.get("active") is not None:
            d.set_active(case["active"])
        with pytest.raises(api.PcrError, match="no word DB"):
            _run(d, case, temps)
        assert _raw(d, case, temps)[0] == PCR_ERR_STATE
        _load(d, oracle, case)

        def state():
            bits = d.find_target_match(panel, case["thr"])
            sid, sites = d.site_tm(panel, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND)
            n0, fr0, rf0 = _products_tm_bits(d, case, 0.0)
            n1, fr1, rf1 = _products_tm_bits(d, case, 58.0)
            return (bits.tolist(), sid.tolist(), sites.tobytes(), n0, fr0.tobytes(), rf0.tobytes(), n1, fr1.tobytes(), rf1.tobytes(),
                    d.entries())

        before = state()
        a = _run(d, case, temps, melt=True)
        _check(oracle, "ids", temps, *a)
        assert state() == before
        empty = d.anneal_profile([], temps, case["thr"], melt=True)             # n_pool = 0: the temperatures and zero counts
        assert len(empty[0]) == 0 and empty[1]["temperature"].tolist() == temps.tolist()
        assert not any(empty[1][f].any() for f in api.ANNEAL_POINT_DTYPE.names[1:]) and empty[2].shape == (0, len(temps))
        with pytest.raises(api.PcrError, match="strictly ascending"):
            d.anneal_profile(panel, [55.0, 55.0], case["thr"])
        with pytest.raises(ValueError):
            d.anneal_profile(panel, temps, case["thr"], select="some")
        b = _run(d, case, temps, melt=True)                                     # the handle is as it was; two runs, the same bytes
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
        assert api.live_resources()[0] > held[0]
    finally:
        d.close()
    assert api.live_resources() == held


def test_determinism(dev, oracle):
    case = PC.scenario(oracle, "random")
    _load(dev, oracle, case)
    temps = AC.ladder_temps(PC.all_products(oracle, "random")[1])
    a = _run(dev, case, temps, melt=True)
    b = _run(dev, case, temps, melt=True)
    assert int(a[1][0]["products_spurious"]) > 1000 and (a[5] >= 0).any()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------ 8. end to end
def test_select_all_end_to_end(oracle):
    case = PC.scenario(oracle, "ladder")
    rec = PC.all_products(oracle, "ladder")[1]
    temps = AC.temps_of(rec)
    d = api.Screener(0)
    try:
        d.load_texts(case["seqs"])
        lo, hi = PC.amp_of(case)
        out = d.anneal_profile(case["panel"], temps, case["thr"], salt=SC.SALT, primer_strand=SC.PRIMER_STRAND, amp_min=lo, amp_max=hi,
                               select="all", melt=True)
        assert d.entries() == SC.db_of(oracle, case)
        _check(oracle, "ladder", temps, *out)
        w_points, w_pair_seq = AC.expected(oracle, "ladder", temps)[:2]
        top = api.anneal_ceiling(out[1], out[2], keep=1.0)
        assert top == api.anneal_ceiling(w_points, w_pair_seq, keep=1.0) and 0 < top < len(temps) - 1
        assert out[2][0, top] == 3 and out[2][0, top + 1] < 3                   # one step hotter drops a sequence
        assert api.bits_to_bool(api.melt_to_bits(out[3], temps[top])[0], 3).tolist() == [True, True, True]
    finally:
        d.close()
