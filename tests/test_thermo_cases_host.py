"""The oracle held to the reference on the inputs of tests/thermo_cases.py -- oligos of 1..11 and 31..32 nt, dimers with a side
of 1..32 nt, degenerate words at either end of the word -- so that tests/test_gpu_thermo_edges.py, which compares the kernel
with the oracle there, proves something.  Also: that those inputs still reach the edges they are meant for, and the refusals
of pcr_valid_words that come before the handle."""
import ctypes as C

import numpy as np
import pytest

import thermo_cases as TC
from pcramp_amd import api

PCR_ERR_ARG = -1
NARROW = dict(tm_min=45.0, tm_max=70.0, max_hairpin=35.0)


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def conditions(k):
    """Salt and strand concentration of case k: the two lists rotate against each other."""
    return TC.SALTS[k % len(TC.SALTS)], TC.STRANDS[(k // len(TC.SALTS)) % len(TC.STRANDS)]


def test_generators_are_what_they_say():
    so = TC.short_oligos()
    assert len(set(so)) == len(so)
    by_len = {}
    for s in so:
        by_len[len(s)] = by_len.get(len(s), 0) + 1
    assert [by_len[n] for n in (1, 2, 3, 4)] == [4, 16, 64, 256]
    assert all(by_len[n] == TC.PER_LENGTH for n in tuple(range(5, 12)) + TC.FULL_LENGTHS) and len(by_len) == 13
    dp = TC.dimer_pairs()
    assert len(dp) == TC.PER_DIMER * len(TC.DIMER_LENGTHS)
    assert {(len(a), len(b)) for a, b in dp} == set(TC.DIMER_LENGTHS)
    assert sum(1 for a, b in dp if len(a) == 32 and b == TC.revcomp(a)) >= 3
    assert sum(1 for a, b in dp if len(a) == 32 and a == TC.revcomp(a)) >= 3
    texts = TC.degenerate_texts()
    assert {len(s) for s in texts} == set(TC.DEGENERATE_LENGTHS) | {24}
    assert max(TC.degeneracy(s) for s in texts) == TC.BIG_TEXT_DEGENERACY
    words = TC.degenerate_words()
    assert len(set(words)) == len(words)
    firsts = {(len(s), f) for s in texts for f in TC.positions(len(s))}
    assert (5, 0) in firsts and (5, 27) in firsts and (5, 14) in firsts and (31, 0) in firsts and (31, 1) in firsts and (32, 0) in firsts
    assert TC.expand("ARCB") == ["AACC", "AACG", "AACT", "AGCC", "AGCG", "AGCT"]


def test_word_positions_agree_with_the_oracle(oracle):
    for s in TC.degenerate_texts():
        for first in TC.positions(len(s)):
            w = TC.word_at(s, first)
            assert oracle.word_start(w) == first and oracle.word_size(w) == len(s) and oracle.word_degeneracy(w) == TC.degeneracy(s)
        assert TC.word_at(s, (33 - len(s)) // 2) == oracle.centered_word(s)
        if TC.degeneracy(s) <= 64:
            spelt = sorted(api.W.word_text(x) for x in oracle.word_expand(oracle.centered_word(s)))
            assert spelt == TC.expand(s)


def test_short_and_full_oligos_oracle_equals_reference(oracle, reference):
    """All ten thermo_full values as float bits; and the edges the oligos are there for, counted on the oracle's values."""
    n = {"tm0": 0, "tm0_le4": 0, "tm": 0, "hairpin": 0, "homodimer": 0}
    for k, s in enumerate(TC.short_oligos()):
        salt, strand = conditions(k)
        got, want = oracle.thermo_full(s, salt, strand), reference.thermo_full(s, salt, strand)
        assert bits(got) == bits(want), (s, salt, strand, got, want)
        if len(s) <= max(TC.SHORT_LENGTHS):
            n["tm0"] += int(got[0] == 0)
            n["tm0_le4"] += int(got[0] == 0 and len(s) <= 4)
            n["tm"] += int(got[0] > 0)
            n["hairpin"] += int(got[4] > 0)
            n["homodimer"] += int(got[7] > 0)
    assert n["tm0_le4"] >= 1 and n["tm0"] >= 100, n                  # dH >= 0, or a Tm below 0 C: the early return and the clamp
    assert n["tm"] >= 100 and n["hairpin"] >= 20 and n["homodimer"] >= 50, n


def test_default_conditions_oracle_equals_reference(oracle, reference):
    """The same oligos at the conditions the GPU test runs them at (a third of the rotation above already is)."""
    for s in TC.short_oligos():
        assert bits(oracle.thermo_full(s, 0.05, 9e-7)) == bits(reference.thermo_full(s, 0.05, 9e-7)), s


def test_dimer_pairs_oracle_equals_reference(oracle, reference):
    nz = nz_full = 0
    pairs = TC.dimer_pairs()
    for k, (a, b) in enumerate(pairs):
        salt, strand = conditions(k)
        sb = strand if k % 4 else strand * 0.5                        # unequal concentrations now and then
        got, want = oracle.heterodimer_full(a, b, salt, strand, sb), reference.heterodimer_full(a, b, salt, strand, sb)
        assert bits(got) == bits(want), (a, b, salt, strand, sb, got, want)
        got, want = oracle.heterodimer_full(b, a, 0.05, 9e-7, 9e-7), reference.heterodimer_full(b, a, 0.05, 9e-7, 9e-7)
        assert bits(got) == bits(want), (b, a, got, want)
        nz += int(got[0] > 0)
        nz_full += int(got[0] > 0 and len(a) == 32 and len(b) == 32)
    assert 4 * nz >= len(pairs) and nz_full >= 5, (nz, nz_full, len(pairs))


def test_degenerate_words_filters_oracle_equals_reference(oracle, reference):
    words = TC.degenerate_words()
    verdicts = {0: 0, 1: 0}
    for w in words:
        for kw in (dict(), NARROW):
            for chk in (False, True):
                got = oracle.is_valid(w, check_homo_dimer=chk, **kw)
                assert got == reference.is_valid(w, check_homo_dimer=chk, **kw), (api.W.word_text(w), kw, chk)
                assert got in (0, 1)
        verdicts[oracle.is_valid(w, check_homo_dimer=False, **NARROW)] += 1
    assert min(verdicts.values()) >= 5, verdicts
    small = [w for w in words if oracle.word_degeneracy(w) <= 64]
    assert len(small) >= 60
    for k, f in enumerate(small):
        r = small[(5 * k + 3) % len(small)]
        if oracle.word_degeneracy(f) * oracle.word_degeneracy(r) > 256:
            continue
        assert bits(oracle.max_dimer_tm((f, r))) == bits(reference.max_dimer_tm((f, r))), (f, r)
        md = (10.0, 25.0, 40.0)[k % 3]
        assert oracle.multiplex_compatible((f, r), (r, f), max_dimer=md) == reference.multiplex_compatible((f, r), (r, f), max_dimer=md), (f, r, md)


def test_unequal_degeneracy_oracle_equals_reference(oracle, reference):
    """1 x 4, 4 x 1, 2 x 3, 3 x 2: both branches of the two-concentration strand term."""
    pairs = TC.unequal_pairs()
    seen, nz = set(), 0
    for k, p in enumerate(pairs):
        seen.add((int(oracle.word_degeneracy(p[0])), int(oracle.word_degeneracy(p[1]))))
        got = oracle.max_dimer_tm(p)
        assert bits(got) == bits(reference.max_dimer_tm(p)), p
        nz += int(got > 0)
        q = pairs[(k + 1) % len(pairs)]
        for md in (10.0, 25.0, 40.0):
            assert oracle.multiplex_compatible(p, q, max_dimer=md) == reference.multiplex_compatible(p, q, max_dimer=md), (p, q, md)
    assert seen == {(1, 4), (4, 1), (2, 3), (3, 2)} and 2 * nz >= len(pairs), (seen, nz)


# ---------------------------------------------------------------------------------- pcr_valid_words, before the handle
def test_valid_words_symbol_and_refusals():
    lib = api.load_library()
    assert "pcr_valid_words" in api.ABI_SYMBOLS and hasattr(lib, "pcr_valid_words")
    w = np.array([TC.word_at("ACGTTGCAAGCTTGCATGCA", 6)], np.uint64)
    out = np.zeros(1, np.uint8)
    args = api.ThermoArgs(0.05, 9e-7, 50.0, 75.0, 40.0, 40.0)
    assert lib.pcr_valid_words(None, w.ctypes.data, 1, C.byref(args), out.ctypes.data) == PCR_ERR_ARG
    assert "bad argument" in api._err(lib)
