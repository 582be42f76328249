"""Two queued pcr_screen_device passes of different handles launched as ONE pair (k_seed3_pair + k_post_pair,
PCRAMP_PAIR=force) against the same passes launched alone (PCRAMP_PAIR=0) and against the oracle: every pass records
what it records alone.  The library's `[pcramp] paired launch:` debug lines say which passes did share their launches.
Run on the GPU box with `-m gpu`."""
import random
import re

import numpy as np
import pytest

from pcramp_amd import api
from testdata import rand_seq, revcomp, sample_pair

pytestmark = pytest.mark.gpu

THR_T = 1.0
THR = float(np.float32(THR_T) * np.float32(0.9))


# ---------------------------------------------------------------------------------------------- inputs
def _plant(rng, seqs, amp, n):
    """Overwrite a stretch of n of the sequences with the amplicon, every second time with its reverse complement."""
    for k, i in enumerate(rng.sample(range(len(seqs)), n)):
        t = amp if k % 2 == 0 else revcomp(amp)
        s = seqs[i]
        if len(s) < len(t) + 2:
            continue
        at = rng.randrange(0, len(s) - len(t))
        seqs[i] = s[:at] + t + s[at + len(t):]


def _make(oracle, seed, shapes, n_pairs):
    """Sets of random sequences (shapes: per set (count, shortest, longest, length step)) and n_pairs primer pairs whose
    amplicons are planted, in both orientations, in sequences of EVERY set."""
    rng = random.Random(seed)
    sets = [[rand_seq(rng, step * rng.randint((lo + step - 1) // step, hi // step)) for _ in range(n)] for n, lo, hi, step in shapes]
    pairs = []
    while len(pairs) < n_pairs:
        src = rand_seq(rng, 260)
        p = sample_pair(rng, src)
        if not p:
            continue
        f, r = p
        i, j = src.find(f), src.find(revcomp(r))
        amp = src[i:j + len(r)]
        for s in sets:
            _plant(rng, s, amp, max(4, len(s) // 10))
        pairs.append((oracle.centered_word(f), oracle.centered_word(r)))
    return sets, pairs


_SESSIONS = {}


def _session(oracle, key, seqs, **opts):
    if key not in _SESSIONS:
        so = oracle.session(**dict(dict(target_threshold=THR_T), **opts))
        for s in seqs:
            so.add_target(s, 1.0)
        _SESSIONS[key] = so
    return _SESSIONS[key]


def _oracle_bits(so, pairs):
    so.select(pairs)
    return np.stack([so.target_match(p).astype(bool) for p in pairs])


# ---------------------------------------------------------------------------------------------- running passes
class Run:
    """Handles on ONE stream, a set each, created under PCRAMP_PAIR=mode; the first pass over a set (it builds the set's
    index, inline) is made and synchronised here, so that every later pass goes through the launcher thread."""

    def __init__(self, torch, monkeypatch, capfd, mode, sets, warm):
        monkeypatch.setenv("PCRAMP_DEBUG", "1")
        monkeypatch.setenv("PCRAMP_PAIR", mode)
        self.torch, self.capfd = torch, capfd
        self.st = torch.cuda.Stream()
        self.hs = [api.Screener(0, stream=self.st.cuda_stream) for _ in sets]
        self.n = [len(s) for s in sets]
        for h, s in zip(self.hs, sets):
            h.load_texts(s, [1.0] * len(s))
        for k in range(len(sets)):
            self.queue(k, warm)
        self.sync()
        capfd.readouterr()

    def buffer(self, k, n_pairs):
        with self.torch.cuda.stream(self.st):
            o = self.torch.full((2, n_pairs, int(self.hs[k].bitset_words())), -1, dtype=self.torch.int64, device="cuda:0")
        self.st.synchronize()
        return o

    def queue(self, k, pairs, out=None, thr=THR, thr_t=THR_T, **kw):
        out = self.buffer(k, len(pairs)) if out is None else out
        self.hs[k].screen_device(pairs, thr, out[0].data_ptr(), out[1].data_ptr(), thr_t, thr_t, 80, 200, False, **kw)
        return out

    def sync(self):
        for h in self.hs:
            h.synchronize()
        self.st.synchronize()
        self.torch.cuda.synchronize()

    def log(self):
        err = self.capfd.readouterr().err
        return err, [(int(a), int(b)) for a, b in re.findall(r"paired launch: passes (\d+) \+ (\d+)", err)]

    def bits(self, k, out):
        a = out.cpu().numpy().view(np.uint64)
        return np.stack([api.bits_to_bool(a[0, p] | a[1, p], self.n[k]) for p in range(a.shape[1])])

    def close(self):
        for h in self.hs:
            h.close()


def _both_modes(torch, monkeypatch, capfd, sets, warm, passes):
    """passes: [(handle, pairs[, keyword arguments of screen_device])], queued in this order, one synchronize at the end -> per mode the bits of every pass, and
    the paired launches of the forced run."""
    res = {}
    for mode in ("force", "0"):
        r = Run(torch, monkeypatch, capfd, mode, sets, warm)
        try:
            outs = [r.queue(q[0], q[1], **(q[2] if len(q) > 2 else {})) for q in passes]
            r.sync()
            err, paired = r.log()
            res[mode] = ([r.bits(q[0], o) for q, o in zip(passes, outs)], paired, err)
        finally:
            r.close()
    assert not res["0"][1], "PCRAMP_PAIR=0 paired"
    return res["force"][0], res["0"][0], res["force"][1], res["force"][2]


@pytest.fixture(scope="module")
def small(oracle):
    """70 sequences of 300-2 000 bases and 130 of 300-1 200 (ragged ends: irregular words; two and three bitset words, so
    the halves of the paired tail's grid differ), and a third set whose lengths are all multiples of 32."""
    sets, pairs = _make(oracle, 20261021, [(70, 300, 2000, 1), (130, 300, 1200, 1), (90, 64, 1504, 32)], 8)
    return sets, pairs


# ---------------------------------------------------------------------------------------------- 1, 2, 6
def _check_pair(torch, monkeypatch, capfd, oracle, key, sets, pa, pb, warm, min_len_b=18):
    got, alone, paired, err = _both_modes(torch, monkeypatch, capfd, sets, warm, [(0, pa), (1, pb, dict(min_oligo_length=min_len_b))])
    print("\n".join(l for l in err.splitlines() if "paired launch" in l or "scan plan" in l))
    assert len(paired) == 1, err
    for k, p in ((0, pa), (1, pb)):
        want = _oracle_bits(_session(oracle, (key, k), sets[k], min_primer=(18, min_len_b)[k]), p)
        assert np.array_equal(got[k], want), "paired pass of handle %d differs from the oracle" % k
        assert np.array_equal(alone[k], want), "single pass of handle %d differs from the oracle" % k
        assert want.any()
    return err


def test_paired_equals_unpaired_equals_oracle(small, oracle, monkeypatch, capfd):
    """A then B under force: one paired launch; 3 and 6 pairs (n_or differs), different n_seq, irregular words on both sides.
    With 5 pairs on the 130 sequences a bitset is 5 x 3 words = 120 bytes, no multiple of 16: such a pass has no fused tail
    (prepare_tables), runs inline as it always has and so cannot pair -- that case is checked too, for its bits and for
    launching alone, in call order."""
    import torch
    sets, pairs = small
    _check_pair(torch, monkeypatch, capfd, oracle, "small", sets[:2], pairs[:3], pairs[2:8], pairs[:2])
    pa, pb = pairs[:3], pairs[3:8]
    got, alone, paired, err = _both_modes(torch, monkeypatch, capfd, sets[:2], pairs[:2], [(0, pa), (1, pb)])
    assert not paired and "inline pass" in err, err
    for k, p in ((0, pa), (1, pb)):
        want = _oracle_bits(_session(oracle, ("small", k), sets[k]), p)
        assert np.array_equal(got[k], want) and np.array_equal(alone[k], want) and want.any(), k


def test_no_irregular_workgroups_on_one_side(small, oracle, monkeypatch, capfd):
    """One side without live irregular words, so that n_irr_wg = 0 on that side only: every length of its set is a multiple
    of 32 and at least 64, and its pass asks for a minimum oligo length of 32 -- the partial words at the sequence ends, which
    every set has, are live from the minimum oligo length on, so at the default 18 this set too has them."""
    import torch
    sets, pairs = small
    err = _check_pair(torch, monkeypatch, capfd, oracle, "noirr32", [sets[0], sets[2]], pairs[:3], pairs[3:8], pairs[:2], min_len_b=32)
    irr = re.findall(r"irregular workgroups (\d+) \+ (\d+)", err)
    assert irr and int(irr[0][0]) > 0 and int(irr[0][1]) == 0, irr


def test_derived_slices_c2_like_plan(oracle, monkeypatch, capfd):
    """2 000 x 1 000 bases, 50 pairs (thousands of seeds: every workgroup's derived slice differs) beside a tiny plan on the
    other handle (fewer seeds than workgroups): the half-grid slices give the hits of the full grid."""
    import torch
    sets, pairs = _make(oracle, 77, [(2000, 1000, 1000, 1), (70, 300, 2000, 1)], 50)
    err = _check_pair(torch, monkeypatch, capfd, oracle, "c2like", sets, pairs, pairs[:1], pairs[:2])
    seeds = [int(x) for x in re.findall(r"scan plan: .*\((\d+) seeds\)", err)]
    print("seeds per plan:", seeds)
    assert max(seeds) > 3000 and min(seeds) < 256, seeds


# ---------------------------------------------------------------------------------------------- 3
def test_order_and_leftovers(small, oracle, monkeypatch, capfd):
    """Three handles, passes A B C A B C A: (A, B), (C, A), (B, C) pair, the seventh pass is launched by the flush of
    synchronize(); then a single pass followed by synchronize() returns."""
    import torch
    sets, pairs = small
    batches = [pairs[:3], pairs[2:8], pairs[2:6], pairs[1:4], pairs[:4], pairs[4:8], pairs[5:8]]   # (130 sequences: an even number of pairs)
    passes = [(i % 3, b) for i, b in enumerate(batches)]
    got, alone, paired, err = _both_modes(torch, monkeypatch, capfd, sets, pairs[:2], passes)
    assert len(paired) == 3, err
    for i, (k, p) in enumerate(passes):
        want = _oracle_bits(_session(oracle, ("small", k) if k < 2 else ("noirr", 1), sets[k]), p)
        assert np.array_equal(got[i], want) and np.array_equal(alone[i], want), i
    r = Run(torch, monkeypatch, capfd, "force", sets[:2], pairs[:2])
    try:
        o = r.queue(0, pairs[:3])
        r.sync()
        _, paired = r.log()
        assert not paired
        assert np.array_equal(r.bits(0, o), _oracle_bits(_session(oracle, ("small", 0), sets[0]), pairs[:3]))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 4
def test_jobs_that_must_not_pair(small, oracle, monkeypatch, capfd):
    """Each of these is launched alone, in call order, bits right: two passes of one handle, two handles writing one buffer,
    a pass with optimize_5, a pass of the first form (select threshold 0.81), a pass whose scan pcr_profile brackets."""
    import torch
    sets, pairs = small
    sets = sets[:2]
    so = [_session(oracle, ("small", k), sets[k]) for k in range(2)]
    pa, pb = pairs[:4], pairs[4:8]
    r = Run(torch, monkeypatch, capfd, "force", sets, pairs[:2])
    try:
        # the control: these two passes do pair while nothing stands against it (the passes below grow the buckets of handle 1)
        o1, o2 = r.queue(0, pa), r.queue(1, pb)
        r.sync()
        err, paired = r.log()
        assert len(paired) == 1, err
        assert np.array_equal(r.bits(0, o1), _oracle_bits(so[0], pa)) and np.array_equal(r.bits(1, o2), _oracle_bits(so[1], pb))
        # two consecutive passes of the same handle
        o1, o2 = r.queue(0, pa), r.queue(0, pb)
        r.sync()
        err, paired = r.log()
        assert not paired, err
        assert np.array_equal(r.bits(0, o1), _oracle_bits(so[0], pa)) and np.array_equal(r.bits(0, o2), _oracle_bits(so[0], pb))
        # two handles given the same output buffer: in call order, B's bits are what is left
        shared = r.buffer(1, 4)
        r.queue(0, pa, out=shared)
        r.queue(1, pb, out=shared)
        r.sync()
        err, paired = r.log()
        assert not paired, err
        assert np.array_equal(r.bits(1, shared), _oracle_bits(so[1], pb))
        # a pass with optimize_5 set (inline: it flushes the held pass)
        o1, o2 = r.queue(0, pa), r.queue(1, pb, optimize_5=True)
        r.sync()
        err, paired = r.log()
        assert not paired, err
        s5 = _session(oracle, ("small5", 1), sets[1], optimize_5=1)
        assert np.array_equal(r.bits(0, o1), _oracle_bits(so[0], pa)) and np.array_equal(r.bits(1, o2), _oracle_bits(s5, pb))
        # a pass at select threshold 0.81 (first form)
        thr81 = float(np.float32(0.9) * np.float32(0.9))
        o1, o2 = r.queue(0, pa), r.queue(1, pb, thr=thr81, thr_t=0.9)
        r.sync()
        err, paired = r.log()
        assert not paired, err
        s81 = _session(oracle, ("small81", 1), sets[1], target_threshold=0.9)
        assert np.array_equal(r.bits(0, o1), _oracle_bits(so[0], pa)) and np.array_equal(r.bits(1, o2), _oracle_bits(s81, pb))
        # a pass whose scan pcr_profile brackets
        r.hs[1].profile(True)
        o1, o2 = r.queue(0, pa), r.queue(1, pb)
        r.sync()
        err, paired = r.log()
        assert not paired, err
        ms, n = r.hs[1].profile_read()
        assert n == 1 and ms > 0.0
        r.hs[1].profile(False)
        assert np.array_equal(r.bits(0, o1), _oracle_bits(so[0], pa)) and np.array_equal(r.bits(1, o2), _oracle_bits(so[1], pb))
    finally:
        r.close()


# ---------------------------------------------------------------------------------------------- 5
def test_replay_of_one_half(small, oracle, monkeypatch, capfd):
    """Handle A holds the dense scenario of tests/dense_buckets.py at its smallest class: its half of the pair overflows the
    64-slot buckets and synchronize() replays it, as it replays a single pass.  B's bits are untouched by that; both equal
    the oracle."""
    import torch
    import dense_buckets as DB
    import test_gpu_dense_buckets as TD
    dn, so_a = TD._case(oracle, ("4k", False))
    sc = dn.sc
    o = sc.opts
    assert o["target_threshold"] == THR_T and o["amp_min"] == 80 and o["amp_max"] == 200, o
    sets, pairs = small
    sparse = [sc.pairs[dn.k["sparse"]]]
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    monkeypatch.setenv("PCRAMP_PAIR", "force")
    st = torch.cuda.Stream()
    a, b = api.Screener(0, stream=st.cuda_stream), api.Screener(0, stream=st.cuda_stream)
    try:
        a.load_texts(sc.seqs, sc.weights)
        act = np.ones(len(sc.seqs), np.uint8)
        act[list(sc.inactive)] = 0
        a.set_active(act)
        for i, pos in sc.splits:
            a.split(i, pos)
        b.load_texts(sets[1], [1.0] * len(sets[1]))

        def queue(d, p, min_len):
            with torch.cuda.stream(st):
                out = torch.full((2, len(p), int(d.bitset_words())), -1, dtype=torch.int64, device="cuda:0")
            st.synchronize()
            d.screen_device(p, TD._thr(o), out[0].data_ptr(), out[1].data_ptr(), THR_T, THR_T, 80, 200, False, min_len)
            return out

        def sync():
            a.synchronize()
            b.synchronize()
            st.synchronize()
            torch.cuda.synchronize()

        queue(a, sparse, o["min_primer"])                   # builds the index, inline; no overflow
        queue(b, pairs[:2], o["min_primer"])
        sync()
        capfd.readouterr()
        oa, ob = queue(a, sc.pairs, o["min_primer"]), queue(b, pairs[2:8], o["min_primer"])
        sync()
        err = capfd.readouterr().err
        assert len(re.findall(r"paired launch:", err)) == 1, err
        done = [int(x) for x in re.findall(r"pass done: (\d+)-slot buckets", err)]
        assert done and done[-1] == DB.CLASSES["4k"].cap, (done, "the dense half was not replayed at its bucket size")
        ha = oa.cpu().numpy().view(np.uint64)
        fr = [api.bits_to_bool(ha[0, p], len(sc.seqs)) for p in range(len(sc.pairs))]
        rf = [api.bits_to_bool(ha[1, p], len(sc.seqs)) for p in range(len(sc.pairs))]
        TD._check_bits(sc, so_a, fr, rf)
        assert a.entries() == so_a.db_entries()
        hb = ob.cpu().numpy().view(np.uint64)
        got_b = np.stack([api.bits_to_bool(hb[0, p] | hb[1, p], len(sets[1])) for p in range(6)])
        sb = _session(oracle, ("small", 1), sets[1]) if o["min_primer"] == 18 else _session(oracle, ("smallmp", 1), sets[1], min_primer=o["min_primer"])
        assert np.array_equal(got_b, _oracle_bits(sb, pairs[2:8]))
    finally:
        a.close()
        b.close()
