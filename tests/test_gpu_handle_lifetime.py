"""A handle gives back everything it took (pcramp_amd/csrc/pcr_owned.hpp, api.live_resources): a tour through every
subsystem that allocates -- both sets, the word DB, the pipelined and the lean staging ring, the mapped return / input
buffers, Smith-Waterman's pinned chunks, thermodynamics, amplicon / product / site records, profiling events left unread,
the record and bound buffers of a target shard on a one-rank host communicator (not the staging of host collectives
over RCCL, which such a communicator never allocates) -- then close(), and the four process-wide counters (device bytes,
mapped host bytes, events, streams the library created) are where they were before the handle existed.  8 targets and 4
backgrounds of 200-400 bases: the smallest sizes at which every subsystem still allocates."""
import random

import numpy as np
import pytest
import torch

from pcramp_amd import api, moves, words as W
from testdata import family_targets, rand_seq, sample_pair

pytestmark = pytest.mark.gpu

SQ = lambda t: float(np.float32(t) * np.float32(t))


def _inputs():
    rng = random.Random(20261019)
    targets = family_targets(rng, 2, 4, 400, div=0.03)                      # 8 targets
    targets = [t[:rng.randint(200, 400)] if i % 2 else t for i, t in enumerate(targets)]
    backgrounds = [rand_seq(rng, rng.randint(200, 400)) for _ in range(4)]
    pairs = []
    while len(pairs) < 3:
        p = sample_pair(rng, targets[4 * (len(pairs) % 2)], primer=(20, 22), amplicon=(80, 180))
        if p:
            pairs.append(tuple(W.centered_word(W.codes_from_text(o)) for o in p))
    return targets, backgrounds, pairs


TARGETS, BACKGROUNDS, PAIRS = _inputs()


def _tour(d, after_step=lambda: None):
    """Every allocating subsystem once; after_step() is called between the steps."""
    d.load_texts(TARGETS)
    d.load_texts(BACKGROUNDS, which=api.BACKGROUND)
    after_step()
    assert d.select_words(PAIRS, SQ(0.9)) > 0
    words = int(d.bitset_words())
    out = torch.zeros((2, len(PAIRS), words), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(3):                                                      # the pipelined and the lean staging ring
        d.screen_device(PAIRS, SQ(0.9), out[0].data_ptr(), out[1].data_ptr(), 0.9, 0.9, 80, 200, False)
    d.synchronize()
    after_step()
    bits = d.amplify(PAIRS, 0.9, 0.9)[0]
    assert bits.any()
    trials = api.host_move_trials(PAIRS[0][0], moves.GROW5, 1, 18, 25)
    assert trials
    d.move_coverage(PAIRS[0], 0, trials, 0.9, 0.9, 80, 200, False)
    f, r = PAIRS[0]
    d.sw_align_words([f, r], [f, f])
    d.is_valid([f, r], True)
    after_step()
    assert d.collect_amplicons(PAIRS[0], 0.9)
    assert len(d.pool_products(PAIRS, 0.9)[1])
    assert len(d.site_tm(PAIRS, 0.9, select=True)[1])
    assert d.select_sites(PAIRS, SQ(0.9)) > 0
    d.split(0, 150)
    after_step()
    d.profile(True)
    d.screen_device(PAIRS, SQ(0.9), out[0].data_ptr(), out[1].data_ptr(), 0.9, 0.9, 80, 200, False)   # its events stay unread
    after_step()
    d.select_words(PAIRS, SQ(0.9))                                          # the word DBs the local search reads
    d.select_words(PAIRS, float(np.float32(0.8) * np.float32(0.9)), which=api.BACKGROUND)
    comm = d.comm_init_host(1, 0, lambda send: send)                        # world 1: the all-gather copies through
    d.shard_targets(comm, 0, len(TARGETS))
    glob = torch.zeros((len(PAIRS), words), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    d.shard_gather_bits(out[0], len(PAIRS), words, glob, words)
    moves.optimization_move(d, PAIRS[0], moves.TRIM5, 0)                    # coverage combined over the shard's communicator
    after_step()
    d.shard_targets(None, 0, 0)
    d.comm_destroy(comm)
    return out, glob


def test_tour_then_close_gives_everything_back():
    before = api.live_resources()
    d = api.Screener(0)
    created = api.live_resources()
    assert created[3] == before[3] + 1 and created[1] > before[1]           # its own stream, the mailbox ring
    keep = _tour(d)
    held = api.live_resources()
    assert held[0] > before[0] and held[1] > created[1] and held[2] > before[2]
    d.close()
    torch.cuda.synchronize()
    assert api.live_resources() == before
    del keep


def test_tour_on_a_borrowed_stream(monkeypatch):
    """The caller's stream is neither counted nor destroyed.  PCRAMP_OPT_SERIAL keeps the optimiser's thermodynamics on the
    handle's stream: the second stream the optimiser otherwise makes for them is the library's own and would count."""
    monkeypatch.setenv("PCRAMP_OPT_SERIAL", "1")
    s = torch.cuda.Stream(device="cuda:0")
    before = api.live_resources()
    d = api.Screener(0, stream=s.cuda_stream)
    seen = [api.live_resources()[3]]
    keep = _tour(d, lambda: seen.append(api.live_resources()[3]))
    d.close()
    assert api.live_resources() == before
    assert seen == [before[3]] * len(seen) and len(seen) == 7               # the stream counter never moved
    with torch.cuda.stream(s):
        t = torch.arange(1024, device="cuda:0").sum()
    s.synchronize()
    assert int(t.item()) == 1023 * 1024 // 2
    del keep


def test_close_with_passes_in_flight():
    before = api.live_resources()
    d = api.Screener(0)
    d.load_texts(TARGETS)
    words = int(d.bitset_words())
    out = torch.zeros((2, len(PAIRS), words), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(2):
        d.screen_device(PAIRS, SQ(0.9), out[0].data_ptr(), out[1].data_ptr(), 0.9, 0.9, 80, 200, False)
    d.close()                                                               # no synchronize() before it
    assert api.live_resources() == before
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != 0).any()                                   # the passes ran to their end


def test_create_on_a_device_that_is_not_there():
    before = api.live_resources()
    with pytest.raises(api.PcrError, match="bad device index"):
        api.Screener(torch.cuda.device_count() + 7)
    assert api.live_resources() == before
