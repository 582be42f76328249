"""The seed lists of a screen pass as the caller's thread makes them (pcramp_amd/csrc/pcr_seed_lists.hpp: one block per cache
entry, two sweeps, a memo by position) through the device: ONE handle runs a chain of pcr_screen_device passes whose batches
change the way the host check's do -- repeated, oligos replaced, two swapped, shorter, longer, another select threshold, a pass
of the first form in between, the background set and back -- so that every pass after the first finds what the earlier ones left
in the caches.  The bits of every pass must equal those of a FRESH handle that runs that pass alone with
PCRAMP_LAUNCH_THREAD=0, and the oracle's.  The chain runs by default, under PCRAMP_PAIR=force on two handles of one stream,
with PCRAMP_S3_NEXT=0 and with PCRAMP_SEED3=0 (the second form shares the listing).  Run on the GPU box with `-m gpu`."""
import random
import re

import numpy as np
import pytest

from pcramp_amd import api
from pcramp_amd import words as W
from testdata import rand_seq, revcomp, sample_pair

pytestmark = pytest.mark.gpu

N_TARGETS, N_BACKGROUND, N_PAIRS = 200, 60, 8


def _thr(select_t, target_t):
    return float(np.float32(target_t) * np.float32(select_t))


# ---------------------------------------------------------------------------------------------- inputs
def _plant_at(seqs, i, at, amp):
    s = seqs[i]
    at = max(0, min(at, len(s) - len(amp)))
    seqs[i] = s[:at] + amp + s[at + len(amp):]


def _near_miss(rng, amp, f):
    """The amplicon with the forward primer's site one mismatch below the floor unsigned(size * 0.9)."""
    k = len(f) - int(np.float32(len(f)) * np.float32(0.9)) + 1
    site = list(amp[:len(f)])
    for j in rng.sample(range(2, len(f) - 2), k):
        site[j] = rng.choice([b for b in "ACGT" if b != site[j]])
    return "".join(site) + amp[len(f):]


def _make(oracle):
    """200 targets of 1.5-2 kb and 60 background sequences; 8 primer pairs whose amplicons are planted on both strands, at the
    very start and the very end of sequences (the partial words there are irregular words), and once each as a near miss
    in a sequence that holds no other copy (targets 0 ... 7: nothing else is planted there)."""
    rng = random.Random(20261021)
    tg = [rand_seq(rng, rng.randint(1500, 2000)) for _ in range(N_TARGETS)]
    bg = [rand_seq(rng, rng.randint(600, 1500)) for _ in range(N_BACKGROUND)]
    pairs, near = [], []
    while len(pairs) < N_PAIRS:
        src = rand_seq(rng, 260)
        p = sample_pair(rng, src)
        if not p:
            continue
        f, r = p
        i, j = src.find(f), src.find(revcomp(r))
        amp = src[i:j + len(r)]
        k = len(pairs)
        for seqs, lo in ((tg, N_PAIRS), (bg, 0)):
            where = rng.sample(range(lo, len(seqs)), 14)
            for n, w in enumerate(where):
                t = amp if n % 2 == 0 else revcomp(amp)
                at = 0 if n in (2, 3) else len(seqs[w]) if n in (4, 5) else rng.randrange(0, len(seqs[w]) - len(t))
                _plant_at(seqs, w, at, t)
        _plant_at(tg, k, 300 + 37 * k, _near_miss(rng, amp, f))
        near.append(k)
        pairs.append((oracle.centered_word(f), oracle.centered_word(r)))
    return tg, bg, pairs, near, {T: _packed(tg), B: _packed(bg)}


def _packed(seqs):
    """The sequences as load_sequences takes them (packed once: every handle below loads the same bytes)."""
    packs = [W.pack_codes(W.codes_from_text(s)) for s in seqs]
    off = np.zeros(len(seqs), dtype=np.uint64)
    off[1:] = np.cumsum([p.size for p in packs])[:-1]
    return np.concatenate(packs), off, [len(s) for s in seqs]


# (set, pairs by index, select threshold multiplier, target threshold): the chain, in order.  Pass 0 builds the target set's
# index and pass 11 the background set's (inline passes); pass 9 is a pass of the first form.
T, B = api.TARGET, api.BACKGROUND
CHAIN = [
    (T, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 0
    (T, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 1 repeated
    (T, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 2 and again
    (T, [0, 1, 6, 7, 4, 5], 0.9, 1.0),             # 3 two pairs replaced
    (T, [5, 1, 6, 7, 4, 0], 0.9, 1.0),             # 4 two swapped
    (T, [5, 1, 6, 7], 0.9, 1.0),                   # 5 shorter
    (T, [5, 1, 6, 7, 2, 3, 0, 4], 0.9, 1.0),       # 6 longer
    (T, [0, 1, 2, 3, 4, 5], 1.0, 1.0),             # 7 another select threshold: other floors under the same oligos
    (T, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 8 and back
    (T, [0, 1, 2, 3, 4, 5], 0.9, 0.9),             # 9 select threshold 0.81: first form
    (T, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 10
    (B, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 11 the background set: another index generation
    (T, [0, 1, 2, 3, 4, 5], 0.9, 1.0),             # 12
    (B, [2, 3, 4, 5, 6, 7], 0.9, 1.0),             # 13
    (T, [2, 3, 4, 5, 6, 7], 0.9, 1.0),             # 14
    (T, [3], 0.9, 1.0),                            # 15 one pair
]


class Handle:
    def __init__(self, torch, data, stream=None):
        self.torch, self.st = torch, stream
        packed = data[4]
        self.h = api.Screener(0, stream=stream.cuda_stream) if stream is not None else api.Screener(0)
        for which in (T, B):
            self.h.load_sequences(*packed[which], which=which)
        self.n = {T: len(data[0]), B: len(data[1])}

    def queue(self, pairs, step):
        which, idx, sel, tt = step
        p = [pairs[i] for i in idx]
        if self.st is not None:
            with self.torch.cuda.stream(self.st):
                out = self.torch.full((2, len(p), int(self.h.bitset_words(which))), -1, dtype=self.torch.int64, device="cuda:0")
            self.st.synchronize()
        else:
            out = self.torch.full((2, len(p), int(self.h.bitset_words(which))), -1, dtype=self.torch.int64, device="cuda:0")
            self.torch.cuda.synchronize()
        self.h.screen_device(p, _thr(sel, tt), out[0].data_ptr(), out[1].data_ptr(), tt, tt, 80, 200, False, which=which)
        return out

    def sync(self):
        self.h.synchronize()
        if self.st is not None:
            self.st.synchronize()
        self.torch.cuda.synchronize()

    def bits(self, out, step):
        a = out.cpu().numpy().view(np.uint64)
        return np.stack([api.bits_to_bool(a[0, p] | a[1, p], self.n[step[0]]) for p in range(a.shape[1])])


@pytest.fixture(scope="module")
def data(oracle):
    return _make(oracle)


@pytest.fixture(scope="module")
def want(oracle, data):
    """Per pass of the chain the oracle's bits, and those of a fresh handle that runs the pass alone without a launcher thread
    (computed once, shared by every mode below)."""
    import os
    import torch
    tg, bg, pairs, near = data[:4]
    sessions = {}

    def session(which, tt):
        if (which, tt) not in sessions:
            so = oracle.session(target_threshold=tt)
            for s in (tg if which == T else bg):
                so.add_target(s, 1.0)
            sessions[(which, tt)] = so
        return sessions[(which, tt)]

    orc, fresh = [], []
    old = os.environ.get("PCRAMP_LAUNCH_THREAD")
    os.environ["PCRAMP_LAUNCH_THREAD"] = "0"
    try:
        for step in CHAIN:
            which, idx, sel, tt = step
            so = session(which, tt)
            p = [pairs[i] for i in idx]
            so.select(p, threshold=_thr(sel, tt))
            orc.append(np.stack([so.target_match(q).astype(bool) for q in p]))
            h = Handle(torch, data)
            try:
                out = h.queue(pairs, step)
                h.sync()
                fresh.append(h.bits(out, step))
            finally:
                h.h.close()
    finally:
        if old is None:
            del os.environ["PCRAMP_LAUNCH_THREAD"]
        else:
            os.environ["PCRAMP_LAUNCH_THREAD"] = old
    for i, (o, f) in enumerate(zip(orc, fresh)):
        assert np.array_equal(o, f), "pass %d: a fresh handle differs from the oracle" % i
        assert o.any(), i
    # the planted sites amplify; the near misses, one mismatch below the floor, do not
    first = orc[0]
    for row, k in enumerate(CHAIN[0][1]):
        assert not first[row, near[k]], "the near miss of pair %d amplifies" % k
        assert first[row].sum() >= 6, (k, int(first[row].sum()))
    return orc


def _run_chain(torch, data, want, handles, log=None):
    """The chain on every handle (handle k starts k passes into it, so that two handles never hold the same batch), the passes
    queued in turn and synchronised once at the end, but for the first pass over each set (inline: it builds the index)."""
    pairs = data[2]
    n = len(CHAIN)
    outs = []
    for i in range(n):
        for k, h in enumerate(handles):
            j = (i + k) % n
            outs.append((k, j, h, h.queue(pairs, CHAIN[j])))
        if i == 0:
            for h in handles:
                h.sync()
    for h in handles:
        h.sync()
    for k, j, h, out in outs:
        assert np.array_equal(h.bits(out, CHAIN[j]), want[j]), "handle %d, pass %d of the chain" % (k, j)


def _forms(err):
    return re.findall(r"scan plan: form=([\w-]+)", err)


def test_chain_default(data, want, monkeypatch, capfd):
    import torch
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    st = torch.cuda.Stream()
    h = Handle(torch, data, st)
    try:
        _run_chain(torch, data, want, [h])
    finally:
        h.h.close()
    forms = _forms(capfd.readouterr().err)
    assert forms.count("seed3") >= len(CHAIN) - 2 and any(f.startswith("seed1") for f in forms), forms


def test_chain_paired_handles(data, want, monkeypatch, capfd):
    import torch
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    monkeypatch.setenv("PCRAMP_PAIR", "force")
    st = torch.cuda.Stream()
    hs = [Handle(torch, data, st), Handle(torch, data, st)]
    try:
        _run_chain(torch, data, want, hs)
    finally:
        for h in hs:
            h.h.close()
    err = capfd.readouterr().err
    assert len(re.findall(r"paired launch:", err)) >= 4, err


def test_chain_plain_seed_lists(data, want, monkeypatch, capfd):
    """PCRAMP_S3_NEXT=0: the third form on the plain 9-gram lists with span A..T."""
    import torch
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    monkeypatch.setenv("PCRAMP_S3_NEXT", "0")
    h = Handle(torch, data, torch.cuda.Stream())
    try:
        _run_chain(torch, data, want, [h])
    finally:
        h.h.close()
    assert _forms(capfd.readouterr().err).count("seed3") >= len(CHAIN) - 2


def test_chain_second_form(data, want, monkeypatch, capfd):
    """PCRAMP_SEED3=0: the second form of the seed scan, listed by the same code without a set."""
    import torch
    monkeypatch.setenv("PCRAMP_DEBUG", "1")
    monkeypatch.setenv("PCRAMP_SEED3", "0")
    h = Handle(torch, data, torch.cuda.Stream())
    try:
        _run_chain(torch, data, want, [h])
    finally:
        h.h.close()
    forms = _forms(capfd.readouterr().err)
    assert "seed3" not in forms and forms.count("seed2") >= len(CHAIN) - 2, forms
