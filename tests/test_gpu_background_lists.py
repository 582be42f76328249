"""pcr_background_match's candidate lists on the rack sets of tests/background_lists.py: every form of the pairing kernel
(k_bg_emit<64>, <128>, <0> by bucket size and by batch width), the wave list's flush and direct append, the overflow of the
sub-lists and the repeated pass (at the library's own capacity and under PCRAMP_DEBUG_AMP_CAP), k_bg_compact's histogram
on either side of 8192 pairs, the pair limit, and candidate_amplicons' own retry under pcr_make_degenerate.

Every case compares the result bits with the oracle bit for bit -- the reference's index mode and evaluate_all, with and
without TaqMAMA, the row of a repeated pair with the row of its original -- and reads the "[pcramp] background_match:"
lines: the form that ran, the bucket slots, the capacities each attempt had, and the records the last attempt emitted, which
must EQUAL the oracle's candidate count summed over the batch (the bits are an OR over the records: a dropped or doubled
record rarely shows in them)."""
import re

import numpy as np
import pytest

import background_lists as BL
from pcramp_amd import api

pytestmark = pytest.mark.gpu

CAND = re.compile(r"\[pcramp\] candidate_amplicons: attempt (\d+), (\d+) pairs, list of (\d+) records, (\d+) records emitted: (\w+)")
_lines = BL.debug_lines


@pytest.fixture(scope="module")
def cases(oracle):
    return BL.cases(oracle)


SEEN = []


@pytest.fixture(autouse=True)
def _show_lines():
    """The debug lines of the test's calls, printed when it ends (pytest -rA shows them)."""
    del SEEN[:]
    yield
    print("\n".join(SEEN))


def _open(c, monkeypatch):
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    if c.hook is None:
        monkeypatch.delenv("PCRAMP_DEBUG_AMP_CAP", raising=False)
    else:
        monkeypatch.setenv("PCRAMP_DEBUG_AMP_CAP", str(c.hook))
    return api.Screener(0)


def _load(d, c, a):
    """The set as BACKGROUND with its inactive flags and its split, the DB selected and equal to the oracle's."""
    d.load_texts(c.seqs, which=api.BACKGROUND)
    act = np.ones(len(c.seqs), np.uint8)
    act[list(c.inactive)] = 0
    d.set_active(act, which=api.BACKGROUND)
    for i, pos in c.splits:
        d.split(i, pos, which=api.BACKGROUND)
    n = d.select_words(c.select, BL.collect_threshold(), BL.MIN_LEN, which=api.BACKGROUND)
    assert n == len(a.entries) and d.entries(which=api.BACKGROUND) == a.entries


def _calls(d, c, a, capfd, cap0):
    """The four calls of a case on a loaded handle whose list holds cap0 records -> (bits by (evaluate_all, taq), lines of
    the first call, the list capacity the handle ends with)."""
    got, first, cap = {}, None, cap0
    for ev in (False, True):
        for taq in (0, 1):
            capfd.readouterr()
            bits = d.find_background_match(c.batch, BL.BT, BL.MULT, BL.AMP[0], BL.AMP[1], bool(taq), evaluate_all=ev)
            err = capfd.readouterr().err
            want = a.bits[(ev, taq)]
            for i, o in enumerate(c.origin):
                assert np.array_equal(bits[i], want[o]), (c.name, ev, taq, i, o)
            got[(ev, taq)] = bits
            ls = _lines(err)
            SEEN.append("%s, evaluate_all=%d, taq=%d:" % (c.name, ev, taq))
            SEEN.extend("  " + l for l in err.splitlines() if "background_match:" in l or "candidate_amplicons:" in l)
            caps = BL.attempts(cap, a.records)
            assert [l["attempt"] for l in ls] == list(range(len(caps))), (c.name, ls)
            assert [l["cap"] for l in ls] == caps and [l["sub_cap"] for l in ls] == [x // BL.SUB_LISTS for x in caps], (c.name, ls)
            assert len(ls) < 6
            for l in ls:
                assert (l["form"], l["slots"], l["pairs"]) == (c.form, c.slots, len(c.batch)), (c.name, l)
                assert l["emitted"] == a.records, (c.name, l)                  # every attempt pairs the whole set again
            for l in ls[:-1]:
                assert l["overflow"] == 1 and l["end"] == "repeated" and l["kept"] < l["emitted"], (c.name, l)
            last = ls[-1]
            assert last["overflow"] == 0 and last["kept"] == last["emitted"] == a.records, (c.name, last)
            # the reference's index rule can only drop a candidate of a pair that has more of them than there are sequences
            ordered = not ev and max(a.counts) > len(c.seqs)
            assert last["end"] == ("ordered path" if ordered else "default path"), (c.name, last)
            cl = [(int(m.group(4)), m.group(5)) for m in CAND.finditer(err)]
            assert cl == ([(a.records, "done")] if ordered else []), (c.name, cl)
            cap = caps[-1]
            if first is None:
                first = ls
    return got, first, cap


def _run(oracle, c, capfd, monkeypatch):
    a = BL.oracle_answers(oracle, c)
    d = _open(c, monkeypatch)
    try:
        _load(d, c, a)
        return _calls(d, c, a, capfd, BL.DEFAULT_CAP if c.hook is None else max(16, c.hook))
    finally:
        d.close()


def test_classes(oracle, cases, capfd, monkeypatch):
    """a. emit<64>, emit<128> and emit<0> chosen by the bucket size: dense racks of each class, and the batch of the 64-slot
    rack at 128- and 256-slot buckets (a ballast sequence grows them), where it must give what it gives at 64."""
    forms = {}
    for s in (64, 128, 256):
        got, first, _ = _run(oracle, cases["class%d" % s], capfd, monkeypatch)
        forms[s] = first[0]["form"]
        if s == 64:
            base = got
    assert forms == {64: "emit<64>", 128: "emit<128>", 256: "emit<0>"}
    for s, form in ((128, "emit<128>"), (256, "emit<0>")):
        c = cases["ballast%d" % s]
        got, first, _ = _run(oracle, c, capfd, monkeypatch)
        assert first[0]["form"] == form and first[0]["slots"] == s
        for key in base:
            assert np.array_equal(got[key][:, :-1], base[key]) and not got[key][:, -1].any(), (s, key)


@pytest.mark.parametrize("p", [129, 200])
def test_wide_batch(oracle, cases, capfd, monkeypatch, p):
    """b. More than eight mask words: k_match + emit<0> at 64-slot buckets; the first 128 rows are those of the 128-pair call."""
    narrow, first, _ = _run(oracle, cases["wide128"], capfd, monkeypatch)
    assert first[0]["form"] == "emit<64>"
    wide, first, _ = _run(oracle, cases["wide%d" % p], capfd, monkeypatch)
    assert first[0]["form"] == "emit<0>" and first[0]["slots"] == 64 and first[0]["pairs"] == p
    for key in narrow:
        assert np.array_equal(wide[key][:128], narrow[key]), key


@pytest.mark.parametrize("name", ["spill_%d_%d" % (nr, p) for nr in BL.SPILL_NR for p in range(1, 6)] + ["spill_24_128"])
def test_spill_sweep(oracle, cases, capfd, monkeypatch, name):
    """c. The wave list: P * nR records from one F site and one chunk of partners, around the flush at 64 and the capacity of
    128, and thousands per chunk (the direct append and the clamp behind it)."""
    _, first, _ = _run(oracle, cases[name], capfd, monkeypatch)
    assert first[0]["form"] == "emit<128>"


def test_natural_overflow(oracle, cases, capfd, monkeypatch):
    """d. More than 65 536 records in one sub-list of the library's own list: the pass is repeated with twice the list; the
    handle keeps the grown list and serves a sparse batch afterwards."""
    c = cases["natural"]
    a = BL.oracle_answers(oracle, c)
    d = _open(c, monkeypatch)
    try:
        _load(d, c, a)
        _, first, cap = _calls(d, c, a, capfd, BL.DEFAULT_CAP)
        assert len(first) == 2 and first[0]["sub_cap"] == 65536 and first[0]["overflow"] == 1 and first[0]["end"] == "repeated"
        assert first[1]["cap"] == 2 * BL.DEFAULT_CAP and first[1]["end"] == "ordered path"
        sparse = c._replace(name="natural, sparse", batch=c.batch[:3], origin=c.origin[:3], form="emit<64>")
        sa = BL.oracle_answers(oracle, sparse)
        _, first, _ = _calls(d, sparse, sa, capfd, cap)
        assert len(first) == 1 and first[0]["cap"] == 2 * BL.DEFAULT_CAP and first[0]["form"] == "emit<64>"
    finally:
        d.close()


@pytest.mark.parametrize("tag", ["16", "256", "_n-1", "_n", "_16n-1", "_16n"])
def test_hooked_overflow(oracle, cases, capfd, monkeypatch, tag):
    """e. PCRAMP_DEBUG_AMP_CAP: a sub-list overflowing while the sum fits, the sum overflowing, several doublings in one
    call, the exact-fit edges; the bits of a handle without the hook."""
    c = cases["hook" + tag]
    n = BL.oracle_answers(oracle, c).records
    got, first, cap = _run(oracle, c, capfd, monkeypatch)
    assert first[0]["cap"] == c.hook
    assert (len(first) > 1) == (c.hook < 16 * n) and len(first) < 6
    assert first[-1]["kept"] == first[-1]["emitted"] == n and cap // BL.SUB_LISTS >= n
    plain, pfirst, _ = _run(oracle, cases["class64"], capfd, monkeypatch)
    assert len(pfirst) == 1 and pfirst[0]["cap"] == BL.DEFAULT_CAP
    for key in plain:
        assert np.array_equal(got[key], plain[key]), key


@pytest.mark.parametrize("p", [8192, 8193])
def test_histogram_boundary(oracle, cases, capfd, monkeypatch, p):
    """f. k_bg_compact counts the records per pair in LDS up to 8192 pairs and with global atomics beyond: the reference mode
    reads those counts (a pair with more candidates than sequences sends the call down the ordered path)."""
    _, first, _ = _run(oracle, cases["hist%d" % p], capfd, monkeypatch)
    assert first[0]["pairs"] == p and first[0]["form"] == "emit<0>"


def test_pair_limit(oracle, cases, capfd, monkeypatch):
    """g. More pairs than the LDS of a workgroup holds geometry for: PCR_ERR_CAPACITY naming the largest batch, nothing
    launched; then that many pairs (16 384 if it is more) against the oracle, and a sparse batch on the same handle."""
    c = cases["limit"]
    a = BL.oracle_answers(oracle, c)
    d = _open(c, monkeypatch)
    try:
        _load(d, c, a)
        too_many = [c.batch[i % len(c.batch)] for i in range(BL.LDS_PER_WORKGROUP // 8 + 1)]     # 8 bytes each: past any workgroup's LDS
        capfd.readouterr()
        with pytest.raises(api.PcrError) as e:
            d.find_background_match(too_many, BL.BT, BL.MULT, *BL.AMP)
        assert e.value.rc == -4                                            # PCR_ERR_CAPACITY
        m = re.fullmatch(r"pcr_background_match: too many pairs in one call: at most (\d+) pairs \(.*\)", str(e.value))
        assert m, str(e.value)
        assert "background_match:" not in capfd.readouterr().err           # refused before any attempt
        limit = int(m.group(1))
        assert BL.LIMIT_PAIRS <= limit < BL.LDS_PER_WORKGROUP // 8        # 160 KiB less the kernel's own arrays, 8 bytes per pair
        assert len(c.batch) == min(limit, BL.LIMIT_PAIRS)
        _, first, cap = _calls(d, c, a, capfd, BL.DEFAULT_CAP)
        assert first[0]["pairs"] == BL.LIMIT_PAIRS and first[0]["form"] == "emit<0>"
        sparse = c._replace(name="limit, sparse", batch=c.batch[:3], origin=c.origin[:3], form="emit<64>")
        _, first, _ = _calls(d, sparse, BL.oracle_answers(oracle, sparse), capfd, cap)
        assert first[0]["form"] == "emit<64>"
    finally:
        d.close()


def test_candidate_amplicons_retry_golden(oracle, capfd, monkeypatch):
    """h. candidate_amplicons (the ordered path's and pcr_make_degenerate's list) with a list of 16 records: every case of
    test_make_degenerate_golden gives the golden result, and the lines show the repeated pass."""
    from test_gpu_golden import test_make_degenerate_golden
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    monkeypatch.setenv("PCRAMP_DEBUG_AMP_CAP", "16")
    repeated = 0
    for ci in range(5):
        capfd.readouterr()
        test_make_degenerate_golden(ci, oracle)
        ls = [(int(m.group(1)), int(m.group(3)), int(m.group(4)), m.group(5)) for m in CAND.finditer(capfd.readouterr().err)]
        assert ls
        SEEN.extend("golden case %d: attempt %d, list of %d records, %d emitted: %s" % ((ci,) + l) for l in ls if l[3] == "repeated")
        for attempt, cap, emitted, end in ls:
            assert end == ("done" if emitted <= cap else "repeated"), (ci, ls)
            repeated += end == "repeated"
        for (a0, c0, e0, end0), (a1, c1, e1, _) in zip(ls, ls[1:]):
            if end0 == "repeated":
                assert (a1, c1, e1) == (a0 + 1, e0 + e0 // 8, e0), (ci, ls)   # the next attempt: room for what was counted, and an eighth
    assert repeated >= 5


def test_candidate_amplicons_retry_rack(oracle, cases, capfd, monkeypatch):
    """h. pcr_make_degenerate on the rack as a target set with a list of 16 records, against the oracle's make_degenerate; then
    find_background_match on the same handle, whose list now holds n + n / 8 records -- no multiple of 16."""
    import json
    import os
    from pcramp_amd import moves
    from oracle_lib import make_degenerate as oracle_make_degenerate
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "degenerate.json")) as f:
        g = json.load(f)["cases"][0]
    o, mo = dict(g["options"], amp_min=BL.AMP[0], amp_max=BL.AMP[1]), g["move_options"]
    c = cases["class64"]._replace(name="class64 after make_degenerate", hook=16)
    a = BL.oracle_answers(oracle, c)
    ts = oracle.session(**o)
    for q in c.seqs:
        ts.add_target(q)
    for i in c.inactive:
        ts.set_active(i, False)
    for i, pos in c.splits:
        ts.split(i, pos)
    ts.select(c.select)
    d = _open(c, monkeypatch)
    try:
        d.load_texts(c.seqs, which=api.TARGET)
        act = np.ones(len(c.seqs), np.uint8)
        act[list(c.inactive)] = 0
        d.set_active(act, which=api.TARGET)
        for i, pos in c.splits:
            d.split(i, pos, which=api.TARGET)
        thr = float(np.float32(o["target_threshold"]) * np.float32(o["search_multiplier"]))
        d.select_words(c.select, thr, o["min_primer"], o["optimize_5"], o["optimize_3"], which=api.TARGET)
        assert d.entries(which=api.TARGET) == ts.db_entries()
        kw = dict(target_threshold=o["target_threshold"], search_multiplier=o["search_multiplier"], amp_min=o["amp_min"],
                  amp_max=o["amp_max"], use_taq_mama=bool(o["use_taq_mama"]), **mo)
        capfd.readouterr()
        got, ok = moves.make_degenerate(d, c.select, max_dimer=g["max_dimer"], **kw)
        err = capfd.readouterr().err
        for k, pair in enumerate(c.select):
            assert (got[k], ok[k]) == oracle_make_degenerate(oracle, ts, pair, max_dimer=g["max_dimer"], **mo), k
        ls = [(int(m.group(1)), int(m.group(3)), int(m.group(4)), m.group(5)) for m in CAND.finditer(err)]
        SEEN.extend(l for l in err.splitlines() if "candidate_amplicons:" in l)
        n = ls[0][2]
        assert n == sum(ts.background_candidates(p, thr, o["amp_min"], o["amp_max"]) for p in c.select)
        assert n > 16 and ls[:2] == [(0, 16, n, "repeated"), (1, n + n // 8, n, "done")], ls
        cap = n + n // 8
        assert cap % 16 != 0
        _load(d, c, a)
        _calls(d, c, a, capfd, cap)
    finally:
        d.close()
