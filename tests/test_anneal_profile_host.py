"""pcr_pool_anneal_profile without a device: the symbol and the record layout, the refusals that come before the handle in
their order, api.melt_to_bits against the bit rows of products_tm_cases at every test temperature (the defining property of
the melt matrices, on the CPU), api.anneal_ceiling on hand-made arrays, and the properties of the scenarios that
tests/test_gpu_anneal_profile.py relies on, computed with the CPU oracle."""
import ctypes as C

import numpy as np
import pytest

import anneal_profile_cases as AC
import products_tm_cases as PC
import site_tm_cases as SC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


def test_symbol_is_exported(lib):
    assert "pcr_pool_anneal_profile" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_pool_anneal_profile"), "libpcramp_hip.so does not export pcr_pool_anneal_profile"
    assert api.ANNEAL_POINT_DTYPE.itemsize == 40 and api.ANNEAL_POINT_DTYPE == AC.ANNEAL_POINT
    assert api.ANNEAL_MAX_TEMPS == AC.MAX_TEMPS == 256
    assert np.float32(api.ANNEAL_NO_PRODUCT).view(np.uint32) == np.float32(-1.0).view(np.uint32) == AC.NO_PRODUCT.view(np.uint32)
    assert hasattr(api.Screener, "anneal_profile")


def _call(lib, which, pool, temps=(50.0, 55.0, 60.0), n_temps=None, template_strand=0.0, primer_strand=9e-7, salt=0.05,
          ids=True, args=True, have_temps=True, points=True):
    a = W.pairs_array(pool) if pool else None
    oid = np.zeros(max(2 * len(pool), 1), np.uint32)
    th = api.ThermoArgs(salt, primer_strand, 0.0, 0.0, 0.0, 0.0)
    t = np.zeros(api.ANNEAL_MAX_TEMPS + 8, np.float32)
    t[:len(temps)] = temps
    pts = np.zeros(api.ANNEAL_MAX_TEMPS + 8, api.ANNEAL_POINT_DTYPE)
    rc = lib.pcr_pool_anneal_profile(None, which, a.ctypes.data if a is not None else None, len(pool), 0.9, 80, 200,
                                     C.byref(th) if args else None, float(template_strand), t.ctypes.data if have_temps else None,
                                     len(temps) if n_temps is None else n_temps, oid.ctypes.data if ids else None,
                                     pts.ctypes.data if points else None, None, None, None, None)
    return rc, api._err(lib)


def test_refusals_before_the_handle(lib, oracle):
    """pcr_pool_products_tm's checks in its order, then the number of temperatures, then their values, then the handle: each
    call below is wrong in one thing and in the handle, and the message names the one thing; two things wrong name the
    earlier."""
    pair = (oracle.centered_word("ACGTTGCAAGCTTGCATGCA"), oracle.centered_word("TTGACCGTAGGCTAGCTAAC"))
    too = SC.too_degenerate_oligo(oracle)
    rc, msg = _call(lib, api.TARGET, [pair])
    assert rc == PCR_ERR_ARG and "null handle" in msg                       # every argument is fine: only the handle is missing
    rc, msg = _call(lib, 7, [pair], ids=False)
    assert rc == PCR_ERR_ARG and "unknown sequence set" in msg              # the set comes before the pointers
    rc, msg = _call(lib, api.MULTIPLEX, [pair], ids=False)
    assert rc == PCR_ERR_ARG and "PCR_SET_MULTIPLEX" in msg
    for missing in ("ids", "args", "have_temps", "points"):
        rc, msg = _call(lib, api.TARGET, [pair], **{missing: False})
        assert rc == PCR_ERR_ARG and "bad argument" in msg, missing
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), points=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg                       # ... come before the pool's size
    rc, msg = _call(lib, api.TARGET, [pair] * (api.POOL_MAX_PAIRS + 1), template_strand=-1e-9)
    assert rc == PCR_ERR_ARG and "PCR_POOL_MAX_PAIRS" in msg                 # ... which comes before the concentrations
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=-1e-9, salt=2.0)
    assert rc == PCR_ERR_ARG and "negative" in msg                           # ... which come before the salt
    rc, msg = _call(lib, api.TARGET, [pair], primer_strand=-9e-7)
    assert rc == PCR_ERR_ARG and "negative" in msg
    rc, msg = _call(lib, api.TARGET, [pair, (pair[0], too)], salt=2.0)
    assert rc == PCR_ERR_ARG and "salt" in msg                               # ... which comes before the oligos
    rc, msg = _call(lib, api.TARGET, [pair], salt=1e-7)
    assert rc == PCR_ERR_ARG and "salt" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=0.0, primer_strand=0.0)   # log(0) is no concentration
    assert rc == PCR_ERR_ARG and "zero" in msg
    rc, msg = _call(lib, api.TARGET, [pair], template_strand=1e-7, primer_strand=0.0)  # the template alone is one
    assert rc == PCR_ERR_ARG and "null handle" in msg
    assert oracle.word_degeneracy(too) == 512
    rc, msg = _call(lib, api.TARGET, [pair, (pair[0], too)], n_temps=0)
    assert rc == PCR_ERR_ARG and "PCR_SITE_MAX_EXPANSIONS" in msg            # the oligos come before the temperatures
    rc, msg = _call(lib, api.TARGET, [(pair[0], (0, 0))], temps=(float("nan"),))
    assert rc == PCR_ERR_ARG and "empty" in msg
    holed = W.word_from_slots([1 if k in (5, 6, 7, 9, 10, 11) else 0 for k in range(32)])
    rc, msg = _call(lib, api.TARGET, [(pair[0], holed)])
    assert rc == PCR_ERR_ARG and "hole" in msg
    rc, msg = _call(lib, api.TARGET, [pair], n_temps=0)
    assert rc == PCR_ERR_ARG and "n_temps" in msg
    rc, msg = _call(lib, api.TARGET, [pair], temps=(float("nan"), 50.0), n_temps=api.ANNEAL_MAX_TEMPS + 1)
    assert rc == PCR_ERR_ARG and "n_temps" in msg                            # the number comes before the values
    rc, msg = _call(lib, api.TARGET, [pair], temps=np.arange(api.ANNEAL_MAX_TEMPS, dtype=np.float32))
    assert rc == PCR_ERR_ARG and "null handle" in msg                        # PCR_ANNEAL_MAX_TEMPS itself passes
    for bad in (float("nan"), float("inf"), float("-inf")):
        for temps in ((bad,), (40.0, bad), (bad, 70.0)):
            rc, msg = _call(lib, api.TARGET, [pair], temps=temps)
            assert rc == PCR_ERR_ARG and "not finite" in msg, temps
    for temps in ((50.0, 50.0), (50.0, 55.0, 55.0), (55.0, 50.0), (-0.0, 0.0), (50.0, 60.0, 59.0)):
        rc, msg = _call(lib, api.TARGET, [pair], temps=temps)
        assert rc == PCR_ERR_ARG and "strictly ascending" in msg, temps
    rc, msg = _call(lib, api.TARGET, [pair], temps=(-5.0, 0.0, float(np.nextafter(np.float32(0), np.float32(1))), 55.0))
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [pair], temps=(55.0,))                  # one temperature is a profile
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, api.TARGET, [])                                     # n_pool = 0 still needs a handle
    assert rc == PCR_ERR_ARG and "null handle" in msg


# ------------------------------------------------------------------ melt_to_bits: the defining property, on the CPU
@pytest.mark.parametrize("name", PC.SCENARIO_NAMES)
def test_melt_to_bits_is_the_floored_bit_rows(oracle, name):
    """For every test temperature f: melt_to_bits(expected melt rows, f) == the bit rows of the products kept at f."""
    ids, rec, _, _ = PC.all_products(oracle, name)
    n_seq = AC.n_seq_of(oracle, name)
    temps = AC.temps_of(rec)
    assert (temps < 0).any() and (temps == 0).any() and (temps > 0).any()
    _, _, fr, rf, _ = AC.expected(oracle, name, temps)
    for f in temps:
        want_fr, want_rf = PC.bits_of(PC.kept(rec, float(f)), ids, n_seq)
        got_fr, got_rf = api.melt_to_bits(fr, float(f)), api.melt_to_bits(rf, float(f))
        assert got_fr.dtype == np.uint64 and got_fr.shape == want_fr.shape == (len(ids) // 2, (n_seq + 63) // 64)
        assert got_fr.tolist() == want_fr.tolist() and got_rf.tolist() == want_rf.tolist(), (name, float(f))


def test_melt_to_bits_layout():
    m = np.full((2, 131), -1.0, np.float32)
    m[0, [0, 63, 64, 130]] = [0.0, 55.0, 60.0, 54.999996]
    m[1, 5] = -0.0                                                           # (never written by the call; counts as 0)
    b = api.melt_to_bits(m, 0.0)
    assert b.shape == (2, 3) and b[0].tolist() == [1 | 1 << 63, 1, 1 << 2] and b[1].tolist() == [1 << 5, 0, 0]
    assert api.melt_to_bits(m, -3.0).tolist() == b.tolist()
    assert api.melt_to_bits(m, 55.0).tolist() == [[1 << 63, 1, 0], [0, 0, 0]]
    assert api.melt_to_bits(m, float(np.nextafter(np.float32(55.0), np.float32(99)))).tolist() == [[0, 1, 0], [0, 0, 0]]
    assert api.bits_to_bool(b[0], 131).nonzero()[0].tolist() == [0, 63, 64, 130]
    assert api.melt_to_bits(np.zeros((0, 70), np.float32), 1.0).shape == (0, 2)
    with pytest.raises(ValueError):
        api.melt_to_bits(np.zeros(5, np.float32), 1.0)


def test_anneal_ceiling():
    pts = np.zeros(4, api.ANNEAL_POINT_DTYPE)
    ps = np.array([[10, 10, 9, 0], [4, 4, 4, 3], [0, 0, 0, 0]], np.uint32)   # a row that never amplifies anything holds nobody back
    assert api.anneal_ceiling(pts, ps) == 1
    assert api.anneal_ceiling(pts, ps, keep=0.9) == 2                        # ceil(9.0) = 9 and ceil(3.6) = 4
    assert api.anneal_ceiling(pts, ps, keep=0.75) == 2                       # ceil(7.5) = 8, ceil(3.0) = 3: row 0 fails at index 3
    assert api.anneal_ceiling(pts, ps, keep=0.0) == 3
    assert api.anneal_ceiling(pts, ps, keep=1.5) == -1                       # more than there is: not even index 0
    assert api.anneal_ceiling(pts, np.zeros((0, 4), np.uint32)) == 3         # no row, no constraint
    assert api.anneal_ceiling(pts[:1], ps[:, :1]) == 0
    with pytest.raises(ValueError):
        api.anneal_ceiling(pts, ps[:, :3])


# ------------------------------------------------------------------ what the GPU tests rely on, computed with the oracle
def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_temperature_lists(oracle):
    for name in PC.SCENARIO_NAMES:
        rec = PC.all_products(oracle, name)[1]
        t = AC.temps_of(rec)
        assert t.dtype == np.float32 and (np.diff(t) > 0).all() and 1 <= len(t) <= AC.MAX_TEMPS
        v = np.unique(AC.melt_values(rec))
        if (v > 0).any():                                                    # a value itself and the nextafter above it; one below, one above all
            assert np.isin(v[v > 0][0], t) and np.isin(np.nextafter(v[v > 0][0], np.float32(np.inf)), t)
            assert 0 < t[t > 0][0] < v[v > 0][0] and t[-1] > v[-1]
        big = AC.ladder_temps(rec)
        assert len(big) == AC.MAX_TEMPS and (np.diff(big) > 0).all() and big[0] < 0 and (big == 0).any() and big[-1] > v.max(initial=0)
        assert np.isin(v[v > 0], big).sum() >= min(len(v[v > 0]), 100)      # the search lands on equal values, not only between them


def test_scenarios_are_what_the_gpu_tests_need(oracle):
    # ladder: one cell fed by 25 products, three distinct melt values over the three sequences
    ids, rec, _, _ = PC.all_products(oracle, "ladder")
    temps = AC.temps_of(rec)
    points, pair_seq, fr, rf, spur = AC.expected(oracle, "ladder", temps)
    cell = rec[(rec["plus_oligo"] == 0) & (rec["minus_oligo"] == 1) & (rec["sequence"] == 0)]
    assert len(cell) >= 25 and len(np.unique(AC.melt_values(cell))) >= 3      # the maximum is taken over many unequal values
    assert fr.shape == (1, 3) and (fr[0] >= 0).all() and fr[0, 0] == AC.melt_values(cell).max() > AC.melt_values(cell).min()
    # (the row itself has two distinct values, not three: sequence 2 holds sequence 0's strongest combination, sequence 1 the weakest)
    assert _bits(fr[0, 0]) == _bits(fr[0, 2]) and fr[0, 1] < fr[0, 0] and fr[0, 1] == AC.melt_values(cell).min()
    assert (_bits(rf) == _bits(AC.NO_PRODUCT)).all() and (_bits(spur) == _bits(AC.NO_PRODUCT)).all()
    assert pair_seq[0].tolist()[0] == 3 and pair_seq[0].tolist()[-1] == 0 and set(pair_seq[0].tolist()) == {3, 2, 0}
    assert [int(p["products_intended"]) for p in points][:3] == [27, 27, 27] and not points["products_spurious"].any()
    assert api.anneal_ceiling(points, pair_seq) == int(np.nonzero(pair_seq[0] == 3)[0][-1]) >= 2
    # words: a cell fed by 64 products, rows over three u64 words, inactive sequences
    ids, rec, _, _ = PC.all_products(oracle, "words")
    _, pair_seq, fr, rf, spur = AC.expected(oracle, "words", AC.temps_of(rec))
    assert fr.shape == (3, PC.WORDS_N) and api.melt_to_bits(fr, 0.0).shape == (3, 3)
    block = rec[(rec["sequence"] == PC.WORDS_BLOCK) & (rec["plus_oligo"] == 0) & (rec["minus_oligo"] == 1)]
    assert len(block) >= 64 and fr[0, PC.WORDS_BLOCK] == AC.melt_values(block).max()
    for s in PC.WORDS_INACTIVE + PC.WORDS_NO_SITE:
        assert (_bits(fr[:, s]) == _bits(AC.NO_PRODUCT)).all() and (_bits(rf[:, s]) == _bits(AC.NO_PRODUCT)).all()
    assert all((api.melt_to_bits(fr, 0.0)[:, w] != 0).any() for w in range(3))
    # pairs: duplicate, exchanged and F = R rows (every product of this scenario is intended: the spurious side is random's and placement's)
    ids, rec, _, _ = PC.all_products(oracle, "pairs")
    _, pair_seq, fr, rf, spur = AC.expected(oracle, "pairs", AC.temps_of(rec))
    assert ids == [0, 1, 2, 2, 0, 3, 0, 1, 1, 0]
    assert _bits(fr[0]).tolist() == _bits(fr[3]).tolist() and _bits(rf[0]).tolist() == _bits(rf[3]).tolist()
    assert _bits(fr[1]).tolist() == _bits(rf[1]).tolist() and (fr[1] >= 0).any()
    assert _bits(fr[4]).tolist() == _bits(rf[0]).tolist() and _bits(rf[4]).tolist() == _bits(fr[0]).tolist()
    assert (fr[0] >= 0).any() and (rf[0] >= 0).any() and _bits(fr[0]).tolist() != _bits(rf[0]).tolist()
    assert pair_seq[0].tolist() == pair_seq[3].tolist() == pair_seq[4].tolist()
    # the spurious side: random has thousands of spurious products, placement nothing else
    ids, rec, _, _ = PC.all_products(oracle, "random")
    points, _, _, _, spur = AC.expected(oracle, "random", AC.temps_of(rec))
    assert int(points[0]["products_spurious"]) == int((rec["intended"] == 0).sum()) > 1000 and (spur >= 0).sum() >= 4
    assert len(set(points["products_spurious"].tolist())) >= 3
    points = AC.expected(oracle, "random", AC.ladder_temps(rec))[0]         # (the 256-step ladder walks through the spurious maxima)
    assert len(set(points["spurious_sequences"].tolist())) >= 5 and len(set(points["products_spurious"].tolist())) >= 20
    ids, rec, _, _ = PC.all_products(oracle, "placement")
    points, pair_seq, fr, rf, spur = AC.expected(oracle, "placement", AC.temps_of(rec))
    assert not points["products_intended"].any() and points[0]["products_spurious"] == 16 and (spur >= 0).any()
    assert (fr < 0).all() and (rf < 0).all() and not pair_seq.any()
    # ambiguity: a cell whose melt is exactly +0.0 -- a product, not the sentinel
    ids, rec, _, _ = PC.all_products(oracle, "ambiguity")
    temps = AC.temps_of(rec)
    points, pair_seq, fr, rf, spur = AC.expected(oracle, "ambiguity", temps)
    assert len(rec) == 1 and _bits(fr).reshape(-1).tolist().count(0) == 1 and (np.sort(fr.reshape(-1))[:-1] == -1).all()
    assert (rf == -1).all() and (spur == -1).all()
    assert pair_seq[0].tolist() == [1 if not t > 0 else 0 for t in temps] and 1 in pair_seq[0].tolist() and 0 in pair_seq[0].tolist()
    # split has no product at all
    rec = PC.all_products(oracle, "split")[1]
    assert len(rec) == 0 and not AC.expected(oracle, "split", AC.temps_of(rec))[1].any()
