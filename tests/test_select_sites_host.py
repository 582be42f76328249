"""pcr_select_sites without a GPU: the symbol and its argument checks (which come before any device work), and the tests'
own expectation (select_sites_cases.expected_entries) against the oracle.

Order of the argument checks, as include/pcramp_hip.h documents it: the set, then min_oligo_length, then the handle -- so the
min_oligo_length refusal can be reached without a device."""
import ctypes as C
import random

import numpy as np

from pcramp_amd import api
from select_sites_cases import (argmax_filter, border_case, expected_entries, floor_of, single_site_case,
                                sites_per_oligo_and_sequence, word_and_np, word_size_np)

PCR_ERR_ARG = -1


def _call(L, handle, which, min_len, n_pairs=0):
    return L.pcr_select_sites(handle, which, None, n_pairs, C.c_float(0.9), min_len, None)


def test_symbol_exists():
    L = api.load_library()
    assert hasattr(L, "pcr_select_sites")
    assert "pcr_select_sites" in api.ABI_SYMBOLS


def test_null_handle_is_refused():
    L = api.load_library()
    assert _call(L, None, api.TARGET, 18) == PCR_ERR_ARG
    assert b"pcr_select_sites" in L.pcr_last_error()


def test_min_oligo_length_checked_before_the_handle():
    L = api.load_library()
    for bad in (0, 33):
        assert _call(L, None, api.TARGET, bad) == PCR_ERR_ARG
        err = L.pcr_last_error()
        assert b"pcr_select_sites" in err and b"min_oligo_length" in err
    for ok in (1, 32):                                   # in range: the refusal is the handle's
        assert _call(L, None, api.TARGET, ok) == PCR_ERR_ARG
        assert b"min_oligo_length" not in L.pcr_last_error()


def test_multiplex_and_unknown_sets_are_refused():
    L = api.load_library()
    for which in (2, 3, 17):
        assert _call(L, None, which, 18) == PCR_ERR_ARG
        assert b"pcr_select_sites" in L.pcr_last_error()


def test_numpy_word_and_against_the_oracle(oracle):
    rng = random.Random(5)
    words = []
    for _ in range(300):
        slots = [0] * 32
        a = rng.randint(0, 14)
        b = rng.randint(a + 1, 32)
        for k in range(a, b):
            slots[k] = rng.choice((1, 2, 4, 8)) if rng.random() < 0.8 else rng.randint(0, 15)
        w = [0, 0]
        for k in range(32):
            w[k >> 4] |= slots[k] << ((15 - (k & 15)) * 4)
        words.append((w[0], w[1]))
    w0 = np.array([w[0] for w in words], dtype=np.uint64)
    w1 = np.array([w[1] for w in words], dtype=np.uint64)
    for i in range(0, 300, 7):
        got = word_and_np(words[i], w0, w1)
        assert [int(x) for x in got] == [oracle.word_and(words[i], w) for w in words]
        assert word_size_np(words[i]) == oracle.word_size(words[i])


def test_floor_is_the_float_product():
    c = (0x0000001111111111, 0x1111111111000000)        # a centred 20-mer
    assert word_size_np(c) == 20
    assert [floor_of(c, t) for t in (1.0, 0.9, 0.85, 0.81, 0.8, 0.7, 0.5)] == [20, 18, 17, 16, 16, 14, 10]
    assert floor_of(c, float(np.float32(0.9) * np.float32(0.9))) == 16


def test_expected_entries_equals_select_where_sites_are_single(oracle):
    """One site at most per (oligo, sequence): the arg-max of select_words keeps exactly the sites, so the oracle's own
    select must give the same DB as the all-sites expectation."""
    rng = random.Random(11)
    seqs, pairs = single_site_case(rng, oracle)
    for thr in (1.0, 0.9, 0.81):
        assert sites_per_oligo_and_sequence(oracle, seqs, pairs, thr) == 1
        so = oracle.session(target_threshold=1.0)
        for s in seqs:
            so.add_target(s, 1.0)
        n = so.select(pairs, threshold=thr)
        exp = expected_entries(oracle, seqs, pairs, thr)
        assert len(exp) == n > 0
        assert exp == so.db_entries()


def test_argmax_of_expected_entries_equals_select(oracle):
    """Several sites per (oligo, sequence) (mutated copies, both strands, sequence ends): select_words' filter applied to the
    all-sites expectation is the oracle's select."""
    rng = random.Random(991)
    seqs, pairs = border_case(rng, oracle)
    seqs = seqs[6:]                                      # the longer sequences and the mutants
    for thr in (0.9, 0.7):
        so = oracle.session(target_threshold=1.0)
        for s in seqs:
            so.add_target(s, 1.0)
        so.select(pairs, threshold=thr)
        exp = expected_entries(oracle, seqs, pairs, thr)
        assert sites_per_oligo_and_sequence(oracle, seqs, pairs, thr) > 1
        assert argmax_filter(exp, pairs, thr) == so.db_entries()
        assert len(exp) > len(so.db_entries())
