"""The independent expectation for pcr_pool_anneal_profile, and the temperature lists its tests share.

Everything is restated in numpy and plain Python from products_tm_cases.all_products' records (the oracle's word DB and duplex
Tm, the join by the rule of include/pcramp_hip.h), by the definitions of the header: a product's melt value v =
min(tm_plus, tm_minus), kept at T iff not (T > 0) or v >= T in float32; per (pool row, sequence) the highest v.  Nothing here
touches the library under test.
"""
import functools

import numpy as np

import products_tm_cases as PC

ANNEAL_POINT = np.dtype([("temperature", np.float32), ("reserved", np.uint32), ("products_intended", np.uint64),
                         ("products_spurious", np.uint64), ("cells", np.uint64), ("spurious_sequences", np.uint64)])
NO_PRODUCT = np.float32(-1.0)
MAX_TEMPS = 256


def n_seq_of(oracle, name):
    return len(PC.scenario(oracle, name)["seqs"])


def melt_values(rec):
    """v of every record: min(tm_plus, tm_minus) with a -0 turned into +0."""
    return (PC.min_tm(rec) + np.float32(0.0)).astype(np.float32)


def keeps(v, temp):
    """The keeping rule on an array of melt values (float32)."""
    t = np.float32(temp)
    v = np.asarray(v, np.float32)
    if not (t > 0):
        return np.ones(v.shape, bool)
    return v >= t


def _strictly_ascending(values):
    t = np.unique(np.asarray(values, np.float32))                              # sorted, distinct as float32
    assert np.isfinite(t).all() and (np.diff(t) > 0).all()
    return t


def temps_of(rec):
    """The temperatures the tests use for a scenario: PC.floors_of(rec) and 0.0, sorted and distinct as float32 -- a negative
    one, 0, values equal to a melt value, the nextafter above each of them, one below all and one above all.  A scenario
    without a positive melt value (no product, or only a NO_TM one) has no such floors: a negative one, 0, a small and an
    ordinary temperature stand in."""
    v = np.unique(PC.min_tm(rec))
    if not (v > 0).any():
        return _strictly_ascending([-10.0, 0.0, 1e-3, 55.0])
    return _strictly_ascending(list(PC.floors_of(rec)) + [0.0])


def ladder_temps(rec, n=MAX_TEMPS):
    """n ascending temperatures around the scenario's melt values: every distinct positive value and the nextafter above it
    (as many as fit), a negative one, 0, one above all, the rest spread evenly from below the lowest to above the highest."""
    v = np.unique(melt_values(rec))
    pos = v[v > 0]
    lo, hi = (float(pos[0]), float(pos[-1])) if len(pos) else (40.0, 70.0)
    must = [np.float32(-10.0), np.float32(0.0), np.float32(hi) + np.float32(5.0)]
    exact = []
    room = max(min(len(pos), (n - len(must)) // 2 - 1), 0)
    for x in (pos[np.unique(np.linspace(0, len(pos) - 1, room).astype(np.int64))] if room else pos[:0]):
        exact += [np.float32(x), np.nextafter(np.float32(x), np.float32(np.inf))]
    have = _strictly_ascending(must + exact)
    fill = np.setdiff1d(np.linspace(lo * 0.5, hi + 4.0, 4 * n).astype(np.float32), have)
    need = n - len(have)
    pick = fill[np.linspace(0, len(fill) - 1, need).astype(np.int64)] if need else fill[:0]
    have = _strictly_ascending(np.concatenate([have, pick]))
    assert len(have) == n
    return have


def expectation(ids, rec, n_seq, temps):
    """-> (points, pair_sequences, melt_fr, melt_rf, melt_spurious) of a scenario's records by the header's definitions."""
    temps = np.asarray(temps, np.float32)
    n_pool = len(ids) // 2
    v = melt_values(rec)
    plus, minus, seq = rec["plus_oligo"].astype(np.int64), rec["minus_oligo"].astype(np.int64), rec["sequence"].astype(np.int64)
    pool = {frozenset((ids[2 * i], ids[2 * i + 1])) for i in range(n_pool)}
    intended = np.array([frozenset((int(a), int(b))) in pool for a, b in zip(plus, minus)], bool)
    assert intended.tolist() == (rec["intended"] != 0).tolist()
    fr = np.full((n_pool, n_seq), NO_PRODUCT, np.float32)
    rf = np.full((n_pool, n_seq), NO_PRODUCT, np.float32)
    spur = np.full(n_seq, NO_PRODUCT, np.float32)
    for k in range(len(rec)):
        s = int(seq[k])
        for i in range(n_pool):
            f, r = ids[2 * i], ids[2 * i + 1]
            if (plus[k], minus[k]) == (f, r):
                fr[i, s] = max(fr[i, s], v[k])
            if (plus[k], minus[k]) == (r, f):
                rf[i, s] = max(rf[i, s], v[k])
        if not intended[k]:
            spur[s] = max(spur[s], v[k])
    points = np.zeros(len(temps), ANNEAL_POINT)
    pair_seq = np.zeros((n_pool, len(temps)), np.uint32)
    both = np.maximum(fr, rf)
    for t, temp in enumerate(temps):
        k = keeps(v, temp)
        points[t]["temperature"] = temp
        points[t]["products_intended"] = int((k & intended).sum())
        points[t]["products_spurious"] = int((k & ~intended).sum())
        pair_seq[:, t] = ((both >= 0) & keeps(both, temp)).sum(axis=1)
        points[t]["cells"] = int(pair_seq[:, t].sum())
        points[t]["spurious_sequences"] = int(((spur >= 0) & keeps(spur, temp)).sum())
    return points, pair_seq, fr, rf, spur


@functools.lru_cache(None)
def _expected(oracle, name, temps_key):
    ids, rec, _, _ = PC.all_products(oracle, name)
    temps = np.frombuffer(temps_key, np.float32)
    out = expectation(ids, rec, n_seq_of(oracle, name), temps)
    for x in out:
        x.setflags(write=False)
    return out


def expected(oracle, name, temps):
    """expectation() of a named scenario, computed once per temperature list and left unchanged."""
    return _expected(oracle, name, np.ascontiguousarray(temps, np.float32).tobytes())


def as_words(x):
    """Any array -> its bytes as a list of integers (floats as their bit patterns): the comparison the tests make."""
    a = np.ascontiguousarray(x)
    return a.view(np.uint32).reshape(-1).tolist() if a.dtype.itemsize % 4 == 0 else a.view(np.uint8).reshape(-1).tolist()
