"""The host side of pcr_pool_conflicts: the expectation's grouping against a brute-force restatement, and api.conflict_matrix
and api.assign_tubes (no GPU)."""
import itertools

import numpy as np
import pytest

import pool_conflict_cases as CC
import products_tm_cases as PC
from pcramp_amd import api


# ------------------------------------------------------------------ the model against the definition read literally
@pytest.mark.parametrize("name", CC.ALL_SCENARIOS)
def test_model_is_the_brute_force_restatement(oracle, name):
    CC.scenario(oracle, name)
    ids, rec, _, _ = PC.all_products(oracle, name)
    floors = CC.floors_of(rec)
    for f in ([0.0, floors[2]] if name == "c_pool40" else [0.0] + floors[:4]):
        assert CC.product_cells(ids, rec, f) == CC.product_cells_brute(ids, rec, f), f


def test_existing_scenarios_barely_group(oracle):
    """Why the new scenarios exist: of the earlier ones only `random` fills more than one cell."""
    filled = {}
    for name in PC.SCENARIO_NAMES:
        ids, rec, _, _ = PC.all_products(oracle, name)
        filled[name] = CC.product_cells(ids, rec, 0.0)
    assert len(filled["random"]) == 21 and sum(c["products"] for c in filled["random"].values()) == 6155
    assert list(filled["placement"]) == [(0, 0)] and filled["placement"][(0, 0)]["products"] == 16
    assert all(len(c) <= 1 for n, c in filled.items() if n != "random")


# ------------------------------------------------------------------ conflict_matrix
def _records(rows):
    rec = np.zeros(len(rows), api.POOL_CONFLICT_DTYPE)
    for k, r in enumerate(rows):
        for f, v in r.items():
            rec[k][f] = v
    return rec


MELT, DIMER_TM = np.float32(57.25), np.float32(41.5)
UP = lambda x: np.nextafter(np.float32(x), np.float32(np.inf))


def test_conflict_matrix_thresholds_and_symmetry():
    rec = _records([
        dict(row_a=0, row_b=1, products=3, sequences=2, melt=MELT, flags=api.CONFLICT_PRODUCT),
        dict(row_a=1, row_b=2, melt=api.ANNEAL_NO_PRODUCT, dimer_tm=DIMER_TM, flags=api.CONFLICT_DIMER),
        dict(row_a=2, row_b=2, products=1, sequences=1, melt=np.float32(30.0), dimer_tm=np.float32(10.0), flags=3),
        dict(row_a=0, row_b=3, melt=api.ANNEAL_NO_PRODUCT, dimer_tm=np.float32(80.0), flags=0),      # below the call's dimer_floor: no flag
    ])
    cells = lambda m: sorted(zip(*np.nonzero(np.triu(m))))
    m = api.conflict_matrix(rec, 4)
    assert m.dtype == bool and m.shape == (4, 4) and (m == m.T).all() and cells(m) == [(0, 1), (2, 2)]
    assert cells(api.conflict_matrix(rec, 4, anneal=MELT)) == [(0, 1)]                   # exactly at melt: still a conflict
    assert cells(api.conflict_matrix(rec, 4, anneal=UP(MELT))) == []
    assert cells(api.conflict_matrix(rec, 4, anneal=30.0)) == [(0, 1), (2, 2)]
    assert cells(api.conflict_matrix(rec, 4, max_dimer=DIMER_TM)) == [(0, 1), (1, 2), (2, 2)]
    assert cells(api.conflict_matrix(rec, 4, max_dimer=UP(DIMER_TM))) == [(0, 1), (2, 2)]
    assert cells(api.conflict_matrix(rec, 4, anneal=UP(MELT), max_dimer=DIMER_TM)) == [(1, 2)]
    assert cells(api.conflict_matrix(rec, 4, anneal=UP(MELT), max_dimer=5.0)) == [(1, 2), (2, 2)]
    for kw in (dict(), dict(anneal=40.0), dict(max_dimer=20.0), dict(anneal=58.0, max_dimer=41.5)):
        m = api.conflict_matrix(rec, 4, **kw)
        assert (m == m.T).all()
    assert not api.conflict_matrix(rec[:0], 3).any() and api.conflict_matrix(rec[:0], 0).shape == (0, 0)


# ------------------------------------------------------------------ assign_tubes
def _graph(n, edges, loops=()):
    m = np.zeros((n, n), bool)
    for a, b in edges:
        m[a, b] = m[b, a] = True
    for a in loops:
        m[a, a] = True
    return m


def _valid(m, tube):
    n = len(tube)
    return all(not (m[a, b] or m[b, a]) or tube[a] != tube[b] for a in range(n) for b in range(a + 1, n))


def _minimum(m):
    n = len(m)
    for k in range(1, n + 1):
        for colours in itertools.product(range(k), repeat=n):
            if _valid(m, colours):
                return k
    return 0


def _greedy(m):
    """The order rule restated: (off-diagonal degree descending, index ascending), lowest free tube."""
    n = len(m)
    off = (m | m.T) & ~np.eye(n, dtype=bool)
    tube = [-1] * n
    for i in sorted(range(n), key=lambda i: (-int(off[i].sum()), i)):
        used = {tube[j] for j in range(n) if off[i, j]}
        tube[i] = min(t for t in range(n + 1) if t not in used)
    return tube


GRAPHS = {
    "path7": _graph(7, [(i, i + 1) for i in range(6)]),
    "path2": _graph(2, [(0, 1)]),
    "clique5": _graph(5, list(itertools.combinations(range(5), 2))),
    "clique7": _graph(7, list(itertools.combinations(range(7), 2))),
    "star7": _graph(7, [(3, i) for i in range(7) if i != 3]),
    "star_first": _graph(6, [(0, i) for i in range(1, 6)]),
    "none": _graph(5, []),
    "one": _graph(1, []),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_assign_tubes_is_minimal_on_paths_cliques_and_stars(name):
    m = GRAPHS[name]
    tube, self_conflict = api.assign_tubes(m)
    assert tube.dtype == np.int32 and self_conflict.dtype == bool and not self_conflict.any()
    assert _valid(m, tube) and tube.tolist() == _greedy(m)
    assert int(tube.max()) + 1 == _minimum(m)


def test_assign_tubes_on_random_graphs():
    rng = np.random.default_rng(6301)
    for n in (3, 6, 12, 40):
        for p in (0.1, 0.4, 0.8):
            upper = np.triu(rng.random((n, n)) < p)
            m = upper | upper.T
            tube, self_conflict = api.assign_tubes(m)
            off = m & ~np.eye(n, dtype=bool)
            assert _valid(m, tube) and tube.tolist() == _greedy(m) and tube.min() == 0
            assert int(tube.max()) + 1 <= int(off.sum(axis=1).max()) + 1
            assert self_conflict.tolist() == m.diagonal().tolist()
            assert api.assign_tubes(np.triu(m))[0].tolist() == tube.tolist()       # either triangle says it
            loops = m.copy()
            loops[np.arange(n), np.arange(n)] = True
            t2, s2 = api.assign_tubes(loops)
            assert t2.tolist() == tube.tolist() and s2.all()                       # the diagonal changes nothing


def test_assign_tubes_max_tubes_self_conflict_and_empty():
    m = GRAPHS["clique5"]
    assert api.assign_tubes(m, max_tubes=5)[0].tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="row 3 "):
        api.assign_tubes(m, max_tubes=3)
    star = GRAPHS["star7"]
    assert api.assign_tubes(star, max_tubes=2)[0].tolist() == [1, 1, 1, 0, 1, 1, 1]
    with pytest.raises(ValueError, match="row 0 "):
        api.assign_tubes(star, max_tubes=1)
    tube, self_conflict = api.assign_tubes(_graph(3, [(0, 2)], loops=(1,)))
    assert tube.tolist() == [0, 0, 1] and self_conflict.tolist() == [False, True, False]
    tube, self_conflict = api.assign_tubes(np.zeros((0, 0), bool))
    assert tube.shape == (0,) and tube.dtype == np.int32 and self_conflict.shape == (0,)
    with pytest.raises(ValueError):
        api.assign_tubes(np.zeros((2, 3), bool))
