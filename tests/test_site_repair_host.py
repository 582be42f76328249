"""pcr_site_repair without a device: the symbol and the record, the refusals that come before the handle, repaired_panel on
hand-made records, and the restatement of site_repair_cases on scenarios whose answers are written out here by hand."""
import ctypes as C

import numpy as np
import pytest

import site_repair_cases as RC
import site_tm_cases as SC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module", autouse=True)
def lib():
    """The library under test; every test of this file is about a call it must export."""
    L = api.load_library()
    assert hasattr(L, "pcr_site_repair"), "libpcramp_hip.so does not export pcr_site_repair"
    return L


def _call(lib, which, panel, max_degeneracy=16, max_mismatch=0, clamp3=0, max_candidates=256, max_steps=12, primer_strand=9e-7,
          salt=0.05, ids=True, out=None, cap=0, args=True):
    a = W.pairs_array(panel) if panel else None
    oid = np.zeros(max(2 * len(panel), 1), np.uint32)
    targs = api.ThermoArgs(salt, primer_strand, 50.0, 75.0, 40.0, 40.0)
    rc = lib.pcr_site_repair(None, which, a.ctypes.data if a is not None else None, len(panel), 0.9, max_degeneracy, max_mismatch,
                             clamp3, max_candidates, max_steps, C.byref(targs) if args else None, 1,
                             oid.ctypes.data if ids else None, out, cap)
    return rc, api._err(lib)


def test_symbol_and_record():
    assert "pcr_site_repair" in api.ABI_SYMBOLS
    assert hasattr(api.load_library(), "pcr_site_repair")
    assert api.REPAIR_STEP_DTYPE.itemsize == 72 and RC.STEP == api.REPAIR_STEP_DTYPE
    assert api.REPAIR_STEP_DTYPE.fields["word"][0].shape == (2,)
    assert api.REPAIR_STEP_DTYPE.fields["oligo"][1] == 16 and api.REPAIR_STEP_DTYPE.fields["valid"][1] == 64
    assert (api.REPAIR_COMPLETE, api.REPAIR_NO_GAIN, api.REPAIR_DEGENERACY, api.REPAIR_STEPS) == \
        (RC.COMPLETE, RC.NO_GAIN, RC.DEGENERACY, RC.STEPS) == (1, 2, 4, 8)
    assert api.REPAIR_MAX_STEPS == 12 and api.REPAIR_MAX_CANDIDATES == 4096 and api.REPAIR_NO_VARIANT == RC.NO_VARIANT


def test_refusals_before_the_handle(lib, oracle):
    """pcr_site_variants' refusals in its order; then max_degeneracy, clamp3, max_candidates, max_steps; then the handle."""
    pair = (oracle.centered_word("ACGTTGCAAGCTTGCATGCA"), oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))
    bad_oligo = (pair[0], SC.too_degenerate_oligo(oracle))
    buf = np.zeros(4, api.REPAIR_STEP_DTYPE)
    rc, msg = _call(lib, api.TARGET, [pair])
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every argument is fine: only the handle is missing
    rc, msg = _call(lib, api.TARGET, [pair], args=False)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [pair], max_steps=0, max_candidates=api.REPAIR_MAX_CANDIDATES, clamp3=32,
                    max_degeneracy=api.SITE_MAX_EXPANSIONS, cap=4, out=buf.ctypes.data)
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every limit itself is legal, max_steps = 0 too
    rc, msg = _call(lib, 7, [pair], ids=False, salt=2.0, max_degeneracy=0)  # the set comes first
    assert rc == PCR_ERR_ARG and "unknown sequence set" in msg
    rc, msg = _call(lib, api.MULTIPLEX, [pair], ids=False, salt=2.0, max_degeneracy=0)
    assert rc == PCR_ERR_ARG and "PCR_SET_MULTIPLEX" in msg
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), ids=False, salt=2.0)   # null pointers before the size
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair], cap=4, salt=2.0)               # cap without a buffer
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), primer_strand=-1e-9)   # the size before the numbers
    assert rc == PCR_ERR_ARG and "PCR_POOL_MAX_PAIRS" in msg
    rc, msg = _call(lib, api.TARGET, [pair], primer_strand=-9e-7, salt=2.0)   # concentrations before salt
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair, bad_oligo], salt=2.0)           # salt before the oligos
    assert rc == PCR_ERR_ARG and "salt" in msg
    rc, msg = _call(lib, api.TARGET, [pair, bad_oligo], max_degeneracy=0)   # the oligos before the call's own numbers
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS expansions" in msg
    rc, msg = _call(lib, api.TARGET, [(pair[0], (0, 0))], args=False, max_degeneracy=0)
    assert rc == PCR_ERR_ARG and "empty" in msg
    rc, msg = _call(lib, api.TARGET, [pair], primer_strand=0.0, max_degeneracy=0)   # log(0) is no concentration
    assert rc == PCR_ERR_ARG and "zero" in msg
    # the call's own, in order
    rc, msg = _call(lib, api.TARGET, [pair], max_degeneracy=0, clamp3=33, max_candidates=0, max_steps=13)
    assert rc == PCR_ERR_ARG and "max_degeneracy" in msg
    rc, msg = _call(lib, api.TARGET, [pair], max_degeneracy=api.SITE_MAX_EXPANSIONS + 1, clamp3=33)
    assert rc == PCR_ERR_ARG and "max_degeneracy" in msg
    rc, msg = _call(lib, api.TARGET, [pair], clamp3=33, max_candidates=0, max_steps=13)
    assert rc == PCR_ERR_ARG and "clamp3" in msg
    rc, msg = _call(lib, api.TARGET, [pair], max_candidates=0, max_steps=13)
    assert rc == PCR_ERR_ARG and "max_candidates" in msg
    rc, msg = _call(lib, api.TARGET, [pair], max_candidates=api.REPAIR_MAX_CANDIDATES + 1, max_steps=13)
    assert rc == PCR_ERR_ARG and "max_candidates" in msg
    rc, msg = _call(lib, api.TARGET, [pair], max_steps=api.REPAIR_MAX_STEPS + 1)
    assert rc == PCR_ERR_ARG and "max_steps" in msg
    rc, msg = _call(lib, api.TARGET, [], args=False, max_steps=13)          # ... also for an empty panel, which needs no pointers
    assert rc == PCR_ERR_ARG and "max_steps" in msg
    rc, msg = _call(lib, api.TARGET, [], args=False)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    # without thermodynamics salt and the concentration are not read
    rc, msg = _call(lib, api.TARGET, [pair], args=False, salt=2.0, primer_strand=-1.0)
    assert rc == PCR_ERR_ARG and "null handle" in msg


# ------------------------------------------------------------------ repaired_panel, on hand-made records
def _step(oligo, step, word, gain, valid, flags=0):
    r = np.zeros(1, api.REPAIR_STEP_DTYPE)
    r["word"], r["oligo"], r["step"], r["gain"], r["valid"], r["flags"] = word, oligo, step, gain, valid, flags
    return r


def test_repaired_panel():
    w = lambda text: W.centered_word(W.codes_from_text(text))
    a, b, c, d = w("ACGTACGTACGTACGTAC"), w("TTGACCGTTTGACCGTAA"), w("GGATCCGGATCCGGATCC"), w("CATGCATGGTACGTACAA")
    a1, a2, a3 = w("ACGTRCGTACGTACGTAC"), w("ACGTRCGTACGYACGTAC"), w("ACGTRCGTACGYACGTAM")
    b1, c1, c2 = w("TTGACCGTTTGWCCGTAA"), w("GGATCCGGRTCCGGATCC"), w("GGATCCGGRTCCGGMTCC")
    panel = [(a, b), (c, a), (a, d)]                                        # a is shared by all three pairs
    ids = np.array([0, 1, 2, 0, 0, 3], np.uint32)
    steps = np.concatenate([
        _step(0, 0, a, 0, 1), _step(0, 1, a1, 5, 1), _step(0, 2, a2, 2, 1), _step(0, 3, a3, 1, 0, api.REPAIR_STEPS),   # the last is invalid
        _step(1, 0, b, 0, 1), _step(1, 1, b1, 3, 0, api.REPAIR_COMPLETE),                                              # its only step is invalid
        _step(2, 0, c, 0, 0), _step(2, 1, c1, 4, 1), _step(2, 2, c2, 1, 1, api.REPAIR_NO_GAIN),
        _step(3, 0, d, 0, 1, api.REPAIR_COMPLETE)])
    got = api.repaired_panel(panel, ids, steps)
    assert got == [(a2, b), (c2, a2), (a2, d)]                              # a falls back to step 2; b has no acceptable step
    assert api.repaired_panel(panel, ids, steps, min_gain=2) == [(a2, b), (c1, a2), (a2, d)]
    assert api.repaired_panel(panel, ids, steps, min_gain=3) == [(a1, b), (c1, a1), (a1, d)]
    assert api.repaired_panel(panel, ids, steps, min_gain=6) == [(a, b), (c, a), (a, d)]
    assert api.repaired_panel(panel, ids, steps, require_valid=False) == [(a3, b1), (c2, a3), (a3, d)]
    assert api.repaired_panel(panel, ids, steps[:0]) == [(a, b), (c, a), (a, d)]
    assert api.repaired_panel([], ids[:0], steps[:0]) == []
    assert all(isinstance(x, int) for pair in got for word in pair for x in word)


# ------------------------------------------------------------------ the restatement itself, answers written out by hand
def _slots(text, start=6):
    sl = [0] * 32
    for i, ch in enumerate(text):
        sl[start + i] = W._CODE[ch]
    return sl


def test_greedy_by_hand():
    """An 8-mer at slots 6 .. 13, max_degeneracy 4.  Record order: E exact (3 sequences); A, base 2 C -> T (sequences 3, 4);
    B, base 5 G -> A (sequence 5; sequence 4 carries it too, beside A); C, both (sequence 6); N, base 2 = N (sequence 7: held
    as it is); D, base 7 T -> G (sequence 8)."""
    oligo = _slots("ACCTAGGT")
    variants = [(10, _slots("ACCTAGGT"), 3), (11, _slots("ACTTAGGT"), 2), (12, _slots("ACCTAAGT"), 2), (13, _slots("ACTTAAGT"), 1),
                (14, _slots("ACNTAGGT"), 1), (15, _slots("ACCTAGGG"), 1)]
    sequences = {0: {0}, 1: {0}, 2: {0}, 3: {1}, 4: {1, 2}, 5: {2}, 6: {3}, 7: {4}, 8: {5}}
    steps = RC.greedy(variants, sequences, oligo, 6, 13, 4, 0, 0, 2, 12)    # two candidates a step: C is not weighed at step 1
    pick = lambda name: [s[name] for s in steps]
    assert pick("step") == [0, 1, 2]
    assert pick("variant") == [RC.NO_VARIANT, 11, 12]                       # A and B tie at gain 2, sites 6, 2 expansions: the index decides
    assert pick("added_mask") == [0, 1 << 2, 1 << 5]
    assert pick("n_expansions") == [1, 2, 4]
    assert pick("candidates") == [0, 2, 2]                                  # A, B (N is held); then B, C -- the same union, B by index
    assert pick("sequences_held") == [4, 6, 8] and pick("gain") == [0, 2, 2]   # B's union holds C's sequence too: 5 and 6
    assert pick("sites_held") == [4, 6, 9] and pick("variants_held") == [2, 3, 5]
    assert pick("sequences_total") == [9, 9, 9]
    assert pick("flags") == [0, 0, RC.DEGENERACY]                           # D is left and its union would have 8 expansions
    assert steps[2]["word"] == W.word_from_slots(_slots("ACYTARGT"))
    # every candidate weighed: C's union holds A, B and C at once and wins step 1
    wide = RC.greedy(variants, sequences, oligo, 6, 13, 4, 0, 0, 256, 12)
    assert [s["variant"] for s in wide] == [RC.NO_VARIANT, 13] and wide[1]["gain"] == 4 and wide[1]["candidates"] == 4
    assert wide[1]["added_mask"] == (1 << 2) | (1 << 5) and wide[1]["n_expansions"] == 4 and wide[1]["flags"] == RC.DEGENERACY
    assert (wide[1]["sequences_held"], wide[1]["sites_held"], wide[1]["variants_held"]) == (8, 9, 5)
    # one step only; none; room for D; one mismatch allowed; a clamp that B, C and D break
    assert [s["flags"] for s in RC.greedy(variants, sequences, oligo, 6, 13, 4, 0, 0, 256, 1)] == [0, RC.STEPS]
    assert [s["flags"] for s in RC.greedy(variants, sequences, oligo, 6, 13, 4, 0, 0, 256, 0)] == [RC.STEPS]
    full = RC.greedy(variants, sequences, oligo, 6, 13, 8, 0, 0, 256, 12)
    assert [s["flags"] for s in full] == [0, 0, RC.COMPLETE] and full[2]["variant"] == 15 and full[2]["n_expansions"] == 8
    one = RC.greedy(variants, sequences, oligo, 6, 13, 4, 1, 0, 256, 12)    # E, A, B, N, D held as they are; C needs one union
    assert [s["sequences_held"] for s in one] == [8, 9] and one[1]["flags"] == RC.COMPLETE and one[1]["variant"] == 13
    clamp = RC.greedy(variants, sequences, oligo, 6, 13, 4, 1, 3, 256, 0)
    assert clamp[0]["variants_held"] == 3 and clamp[0]["sequences_held"] == 6
    assert RC.greedy(variants, sequences, oligo, 6, 13, 4, 8, 9, 256, 0)[0]["variants_held"] == 0   # a clamp longer than the oligo
    # max_candidates cuts by record order: with 1 only A is ever weighed, then B, then C (gain 0 once A and B are in)
    cut = RC.greedy(variants, sequences, oligo, 6, 13, 4, 0, 0, 1, 12)
    assert [s["variant"] for s in cut] == [RC.NO_VARIANT, 11, 12] and [s["candidates"] for s in cut] == [0, 1, 1]
    assert cut[2]["flags"] == RC.DEGENERACY
    # no site at all
    none = RC.greedy([], {}, oligo, 6, 13, 4, 0, 0, 256, 12)
    assert len(none) == 1 and none[0]["flags"] == RC.COMPLETE and none[0]["sequences_total"] == 0


def test_free_coverage_by_hand(oracle):
    """The free-coverage scenario through the whole restatement: A, then B with C's sequence for free."""
    case = RC.free_coverage_case(oracle)
    ids, steps = RC.expectation(oracle, case)
    mine = steps[steps["oligo"] == 0]
    assert mine["step"].tolist() == [0, 1, 2]
    assert mine["sequences_held"].tolist() == [2, 7, 12] and mine["gain"].tolist() == [0, 5, 5]
    assert mine["variants_held"].tolist() == [1, 2, 4] and mine["sites_held"].tolist() == [2, 7, 12]
    assert mine["added_mask"].tolist() == [0, 1 << 3, 1 << 10] and mine["n_expansions"].tolist() == [1, 2, 4]
    assert mine["flags"].tolist() == [0, 0, RC.COMPLETE] and mine["sequences_total"].tolist() == [12] * 3
    assert mine["candidates"].tolist() == [0, 2, 2]                         # A, B; then B, C (one union: B by index)
    other = steps[steps["oligo"] == 1]                                      # the partner has no site: its step 0 alone
    assert len(other) == 1 and other[0]["flags"] == RC.COMPLETE and other[0]["sequences_total"] == 0
    assert set(steps["valid"].tolist()) <= {0, 1}
    cold = RC.expectation(oracle, case, thermo=None)[1]
    assert not cold["valid"].any()
    assert [t[:-1] for t in RC.as_tuples(cold)] == [t[:-1] for t in RC.as_tuples(steps)]
