"""The pipelined pcr_screen_device pass -- planned on the caller's thread, staged and launched by the stream's launcher
thread -- against the same passes run inline (PCRAMP_LAUNCH_THREAD=0) and against the oracle: bit for bit the same
buffers, whatever is called next.  Run on the GPU box with `-m gpu`."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from pcramp_amd import api
from testdata import rand_seq, revcomp
from launch_thread_cases import make_seqs, make_batches, screener

pytestmark = pytest.mark.gpu

THR_T = 1.0
THR = float(np.float32(THR_T) * np.float32(0.9))


def _queue(dev, p, o):
    dev.screen_device(p, THR, o[0].data_ptr(), o[1].data_ptr(), THR_T, THR_T, 80, 200, False)


def _buffers(torch, batches, words):
    return [torch.full((2, len(p), words), -1, dtype=torch.int64, device="cuda:0") for p in batches]


def _host(o):
    return o.cpu().numpy().view(np.uint64)


def _sync(torch, *devs):
    for d in devs:
        d.synchronize()
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def cases(oracle):
    out = {}
    for n in (43, 130):
        roots, seqs = make_seqs(n)
        out[n] = (roots, seqs, make_batches(oracle, roots, 48, 1000 + n))
    return out


@pytest.mark.parametrize("n_seqs", [43, 130])
def test_pipelined_passes_equal_inline_passes(cases, oracle, n_seqs):
    """48 passes, a different batch each (2-16 pairs: plan sizes, ring bytes and cache hits all vary), each into a buffer
    of its own, one synchronize at the end: every buffer equals the inline handle's, a sample equals the oracle, and the
    passes did go through the launcher thread."""
    import torch
    roots, seqs, batches = cases[n_seqs]
    pip, inl = screener(api, True), screener(api, False)
    try:
        for d in (pip, inl):
            d.load_texts(seqs, [1.0] * len(seqs))
        words = int(pip.bitset_words())
        assert words == (n_seqs + 63) // 64
        got, want = _buffers(torch, batches, words), _buffers(torch, batches, words)
        for p, o in zip(batches, got):
            _queue(pip, p, o)
        _sync(torch, pip)
        n_pipelined, depth = pip.launcher_stats()
        for p, o in zip(batches, want):
            _queue(inl, p, o)
        _sync(torch, inl)
        print("passes pipelined %d of %d, max queue depth %d" % (n_pipelined, len(batches), depth))
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(_host(g), _host(w)), "pass %d" % k
        assert pip.entries() == inl.entries()
        so = oracle.session(target_threshold=THR_T)
        for s in seqs:
            so.add_target(s, 1.0)
        any_set = False
        for k in range(0, len(batches), 8):
            so.select(batches[k])
            h = _host(got[k])
            for i, p in enumerate(batches[k]):
                bits = api.bits_to_bool(h[0, i] | h[1, i], n_seqs)
                assert np.array_equal(bits, so.target_match(p).astype(bool)), "pass %d pair %d" % (k, i)
                any_set = any_set or bits.any()
        assert any_set
        assert inl.launcher_stats() == (0, 0)
        assert n_pipelined >= 40, "the pipelined path did not run"
        assert depth >= 2, "the launcher thread never had a pass waiting behind another"
    finally:
        pip.close()
        inl.close()


def test_three_handles_on_one_stream_alternate_two_buffers(cases):
    """Three handles on ONE stream share its launcher thread; 60 passes go to them in turn and write two output buffers
    alternately, as bench.py does.  The launches must reach the stream in call order across the handles: at the end the two
    buffers hold exactly the results of the last two calls."""
    import torch
    roots, seqs, _ = cases[43]
    rng_batches = make_batches_fixed(roots, 60)
    st = torch.cuda.Stream()
    hs = [screener(api, True, stream=st.cuda_stream) for _ in range(3)]
    inl = screener(api, False)
    try:
        for d in hs + [inl]:
            d.load_texts(seqs, [1.0] * len(seqs))
        words = int(inl.bitset_words())
        bufs = _buffers(torch, rng_batches[:2], words)
        torch.cuda.synchronize()
        for k, p in enumerate(rng_batches):
            _queue(hs[k % 3], p, bufs[k % 2])
        for d in hs:
            d.synchronize()
        st.synchronize()
        torch.cuda.synchronize()
        want = _buffers(torch, rng_batches[58:], words)
        for p, o in zip(rng_batches[58:], want):
            _queue(inl, p, o)
        _sync(torch, inl)
        assert np.array_equal(_host(bufs[0]), _host(want[0]))
        assert np.array_equal(_host(bufs[1]), _host(want[1]))
        assert _host(want[0]).any() and _host(want[1]).any()
        assert not np.array_equal(_host(want[0]), _host(want[1]))
        stats = [d.launcher_stats() for d in hs]
        print("per handle (pipelined, depth):", stats)
        assert sum(s[0] for s in stats) >= 50
    finally:
        for d in hs + [inl]:
            d.close()


def make_batches_fixed(roots, n):
    from oracle_lib import Oracle
    return make_batches(Oracle(), roots, n, 4242, sizes=(8,))


def test_other_entry_points_right_behind_queued_passes(cases, oracle):
    """No synchronize between pipelined passes and what is called next: entries(), select_words, amplify, load_texts of a
    new set.  Every one of them first waits for the launcher thread; results equal the inline handle's."""
    import torch
    roots, seqs, batches = cases[43]
    pip, inl = screener(api, True), screener(api, False)
    try:
        for d in (pip, inl):
            d.load_texts(seqs, [1.0] * len(seqs))
        words = int(pip.bitset_words())
        res = {}
        for d in (pip, inl):
            r = res[d] = []
            o = _buffers(torch, batches[:26], words)
            for k in range(0, 6):                                        # (the first one builds the index, inline; five queued)
                _queue(d, batches[k], o[k])
            r.append(d.entries())
            for k in range(6, 11):
                _queue(d, batches[k], o[k])
            r.append(d.select_words(batches[11], THR, 18))
            r.append(d.entries())
            for k in range(12, 17):
                _queue(d, batches[k], o[k])
            _, fr, rf, cov = d.amplify(batches[16], THR_T, THR_T, 80, 200, False)
            r += [np.array(fr), np.array(rf), np.array(cov)]
            for k in range(17, 22):
                _queue(d, batches[k], o[k])
            d.load_texts(seqs[5:30], [1.0] * 25)                         # a new set right behind them
            o2 = _buffers(torch, batches[22:26], int(d.bitset_words()))
            for k in range(22, 26):
                _queue(d, batches[k], o2[k - 22])
            r.append(d.entries())
            _sync(torch, d)
            r += [_host(x) for x in o[:22]] + [_host(x) for x in o2]
        a, b = res[pip], res[inl]
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, "result %d" % k
        assert any(len(e) for e in (a[0], a[2], a[6]))
        n_pipelined, _ = pip.launcher_stats()
        print("passes pipelined: %d of 26" % n_pipelined)
        assert n_pipelined >= 20
    finally:
        pip.close()
        inl.close()


def test_close_with_passes_queued_returns_and_the_process_exits():
    """close() right behind queued passes, no synchronize: it must return (the launcher thread is flushed, stopped and
    joined) and the process must exit normally.  In a fresh child process, under a time limit."""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run(["timeout", "-k", "10", "120", sys.executable, os.path.join(here, "launch_thread_cases.py"), "close"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=here)
    print(r.stdout)
    assert r.returncode == 0, r.stdout
    assert "closed with" in r.stdout and "closed with 0 " not in r.stdout, r.stdout


def test_bucket_overflow_with_passes_queued_behind_it(oracle):
    """The dense input of test_screen_device_replays_after_bucket_overflow: the pass whose buckets overflow is queued
    with three more passes behind it; synchronize() finds the overflow and replays all four.  Bits equal the
    synchronous path's."""
    import torch
    rng = random.Random(12)
    seqs = ["A" * 300 + rand_seq(rng, 300) + "AC" * 200 + rand_seq(rng, 100) + "T" * 300, rand_seq(rng, 1200)]
    s1 = seqs[1]
    txt = [("A" * 20, "A" * 20), ("AC" * 10, "GT" * 10), (s1[100:120], revcomp(s1[220:240])), (s1[400:421], revcomp(s1[520:540]))]
    pairs = [(oracle.centered_word(f), oracle.centered_word(r)) for f, r in txt]
    behind = [pairs[2:], pairs[:2], pairs[1:3]]
    a = screener(api, True)
    try:
        a.load_texts(seqs, [1.0, 1.0])
        want = []
        for p in [pairs] + behind:
            a.select_words(p, THR, 18)
            _, fr, rf, _ = a.amplify(p, THR_T, THR_T, 80, 200, False)
            want.append((np.array(fr), np.array(rf)))
        assert len(a.entries()) > 0
        a.select_words(pairs, THR, 18)
        assert len(a.entries()) > 64                     # more than the initial bucket size in one sequence
        a.load_texts(seqs, [1.0, 1.0])                   # resets the bucket size
        words = int(a.bitset_words())
        o0 = torch.full((2, 2, words), -1, dtype=torch.int64, device="cuda:0")
        _queue(a, pairs[2:], o0)                         # builds the set's index (inline); no overflow
        a.synchronize()
        outs = _buffers(torch, [pairs] + behind, words)
        for p, o in zip([pairs] + behind, outs):
            _queue(a, p, o)
        _sync(torch, a)
        n_pipelined = a.launcher_stats()[0]
        print("passes pipelined: %d of 4" % n_pipelined)
        assert n_pipelined >= 3, "the overflowing pass and those behind it did not go through the launcher thread"
        for k, (p, o) in enumerate(zip([pairs] + behind, outs)):
            h = _host(o)
            for i in range(len(p)):
                assert np.array_equal(api.bits_to_bool(h[0, i], 2), want[k][0][i]), (k, i)
                assert np.array_equal(api.bits_to_bool(h[1, i], 2), want[k][1][i]), (k, i)
        assert want[0][0].any() or want[0][1].any()
        assert len(a.entries()) > 0
    finally:
        a.close()
