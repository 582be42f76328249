"""The position index sorted by the base behind the 9-gram, and the folded seeds that read a quarter of a run (k_seed3,
pcramp_amd/csrc/pcr_scan_seed3.inc; pcrhost::orientation_fold_seeds): the default handle against the same binary reading whole
runs (PCRAMP_S3_NEXT=0), the bit-sliced scan (PCRAMP_SCAN=2) and the oracle -- the word DB entry for entry -- where the next
base can go wrong: mismatches at and around the tenth base of every block, sub-runs longer than one and two 64-entry chunks with
an empty one between them, 9-grams at the end of a sequence, EOS splits and inactive sequences after the index was built,
several launch groups, IUPAC primers.  Run on the GPU box with `-m gpu`."""
import random
import re

import numpy as np
import pytest

from pcramp_amd import api, words as W
from testdata import rand_seq, revcomp, mutate
from test_gpu_seed_scan import _screener_env, _entries, _entries_only

pytestmark = pytest.mark.gpu

THR_T, MULT = 1.0, 0.9
THR = float(np.float32(THR_T) * np.float32(MULT))


@pytest.fixture(scope="module")
def trio():
    """default | whole runs in the new binary | bit-sliced scan (the first two report their scan plan)"""
    devs = [_screener_env(PCRAMP_DEBUG=1), _screener_env(PCRAMP_DEBUG=1, PCRAMP_S3_NEXT=0), _screener_env(PCRAMP_SCAN=2)]
    yield devs
    for d in devs:
        d.close()


def _oracle_session(oracle, seqs):
    so = oracle.session(target_threshold=THR_T, search_multiplier=MULT, amp_min=80, amp_max=200, use_taq_mama=0,
                        pack_max_degen=256, pack_min_gc=0.0, pack_max_gc=1.0, min_primer=18, optimize_5=0, optimize_3=0)
    for s in seqs:
        so.add_target(s, 1.0)
    return so


def _agree(trio, oracle, capfd, seqs, pairs, min_entries=1):
    """Load, select on all three handles and the oracle; the two index handles must have run the third form."""
    capfd.readouterr()
    got = [_entries(d, seqs, pairs, THR) for d in trio]
    forms = re.findall(r"scan plan: form=([\w-]+),", capfd.readouterr().err)
    so = _oracle_session(oracle, seqs)
    so.select(pairs)
    want = so.db_entries()
    print("%d sequences, %d pairs: %d entries; forms %s" % (len(seqs), len(pairs), len(want), forms))
    assert len(forms) >= 2 and set(forms) == {"seed3"}
    assert len(want) >= min_entries
    assert got[0] == want, "default handle"
    assert got[1] == want, "PCRAMP_S3_NEXT=0"
    assert got[2] == want, "PCRAMP_SCAN=2"
    return so, want


def _fold_blocks(word, n):
    """First oligo positions of the 10-base block windows of the oligo's folded seeds (window slot offset - first occupied slot)."""
    floor = int(np.float32(n) * np.float32(THR))
    sd = api.host_orientation_fold_seeds(word, floor)
    assert sd is not None
    first = int(np.nonzero(W.slots_from_word(word))[0][0])
    return sorted({off - first for _, off, _, _ in sd}), n - floor


def _with_mismatches(rng, site, positions):
    s = list(site)
    for p in positions:
        s[p] = rng.choice([b for b in "ACGT" if b != s[p]])
    return "".join(s)


def test_mismatches_at_and_around_the_tenth_base(trio, oracle, capfd):
    """8 sequences of 600 bases, one primer pair per length 18 ... 25.  A (sequence, oligo) keeps the windows that tie at its best
    count, so all sites of an oligo in one sequence carry the same number of mismatches: sequence q holds sites with q % 4
    mismatching bases (where the oligo tolerates that many), of the forward primers for q < 4 (forward orientation) and of the
    reverse primers for q >= 4 (reverse-complement orientation).  The mismatches sit at the tenth, the ninth and the first base
    of a block window of the folded seeds and just outside it."""
    rng = random.Random(50510)
    oligos = [(rand_seq(rng, n), rand_seq(rng, n)) for n in range(18, 26)]
    pairs = [(oracle.centered_word(f), oracle.centered_word(r)) for f, r in oligos]
    seqs, planted = [], 0
    for q in range(8):
        j, parts = q % 4, []
        for (f, r), (wf, wr) in zip(oligos, pairs):
            n = len(f)
            if q < 4:
                site, word = f, wf
            else:                                                      # the window is the reverse complement of the reverse primer
                site, word = revcomp(r), W.word_from_slots(W.revcomp_codes(W.slots_from_word(wr)))
            blocks, k = _fold_blocks(word, n)
            if j > k:
                continue
            if j == 0:
                variants = [[]]
            else:
                variants = []
                for v, prio in enumerate(([9, 8, 0, 10], [0, 9, -1, 10], [8, 10, 9, -1] if n & 1 else [-1, 9, 8, 0])):
                    b = blocks[0] if v == 0 else blocks[-1] if v == 1 else blocks[n % len(blocks)]
                    pos = [b + d for d in prio if 0 <= b + d < n]
                    assert len(pos) >= j
                    variants.append(sorted(pos[:j]))
            for pos in variants:
                parts.append(_with_mismatches(rng, site, pos) + rand_seq(rng, 1))
                planted += 1
        body = "".join(parts)
        assert len(body) <= 600 - 12, len(body)
        seqs.append(rand_seq(rng, 6) + body + rand_seq(rng, 600 - 6 - len(body)))
    _, want = _agree(trio, oracle, capfd, seqs, pairs, min_entries=planted)
    assert {e[3] for e in want} == set(range(8))


def test_sub_runs_longer_than_one_and_two_chunks(trio, oracle, capfd):
    """One site repeated 70, 130 and 200 times over three sequences, every copy with exactly one mismatch (so all tie and all
    are kept): at the tenth base of the first block window in 35 % (one replacement base) and 15 % (another) of the copies, in
    the other block -- the tenth base as the primer has it -- in the rest; the fourth base never follows that 9-gram, and its
    code lies between two that do.  The 9-gram's sub-runs then hold about 200, 140, 60 and 0 entries: more than one and more than two
    64-entry chunks, with an empty sub-run between two full ones."""
    rng = random.Random(70130)
    f, r = rand_seq(rng, 20), rand_seq(rng, 20)
    wf = oracle.centered_word(f)
    blocks, k = _fold_blocks(wf, 20)
    assert k == 2 and len(blocks) == 2
    t = blocks[0] + 9                                                  # the tenth base of the first block window
    other = blocks[1] + 4                                              # a base well inside the other block
    assert 0 <= t < 20 and 0 <= other < 20 and other != t
    order = "ACGT"
    here = order.index(f[t])
    absent = 1 if here != 1 else 2                                     # C, or G where the primer has C: between two bases that appear
    alts = [b for i, b in enumerate(order) if i not in (here, absent)]
    seqs = []
    for copies in (70, 130, 200):
        parts = []
        for c in range(copies):
            x = (c * 20) // copies if copies >= 20 else c              # 0 ... 19, in order: 7 of 20 -> first replacement, 3 of 20 -> second
            s = list(f)
            if x < 7:
                s[t] = alts[0]
            elif x < 10:
                s[t] = alts[1]
            else:
                s[other] = rng.choice([b for b in "ACGT" if b != f[other]])
            parts.append("".join(s) + rng.choice("ACGT"))
        seqs.append(rand_seq(rng, 40) + "".join(parts) + rand_seq(rng, 40))
    seqs.append(rand_seq(rng, 300) + revcomp(r) + rand_seq(rng, 50))
    pairs = [(wf, oracle.centered_word(r))]
    _, want = _agree(trio, oracle, capfd, seqs, pairs, min_entries=401)
    per_seq = [sum(1 for e in want if e[3] == q) for q in range(3)]
    assert per_seq == [70, 130, 200], per_seq


def test_nine_grams_at_the_end_of_a_sequence(trio, oracle, capfd):
    """Sequences of 32, 40 and 41 bases.  The last 9-gram of a sequence (p = L - 9) has no base behind it inside the sequence and is
    sorted under what follows in memory: here the NEXT sequence starts with the very base that would complete the primer's
    10-gram (and goes on with the rest of the primer), so a scan that read across the end would find a site that is not there.
    Also the 9-gram one before the last, the one regular window of a 32-base sequence, the last regular window of a 41-base
    one, and sites hanging over either end by 1 ... k bases: the irregular words, through their index."""
    rng = random.Random(324041)
    f, g = rand_seq(rng, 20), rand_seq(rng, 19)
    pairs = [(oracle.centered_word(f), oracle.centered_word(g))]
    first = (33 - 20) // 2
    seqs = []
    s = list(rand_seq(rng, 32)); s[first:first + 20] = f; seqs.append("".join(s))                 # 32 bases: its only window is the site
    seqs.append(rand_seq(rng, 21) + f[:19])                          # 40: ends with all but the last base of the primer (9-gram f[10:19] at p = L - 9)
    seqs.append(f[19:] + rand_seq(rng, 40))                          # 41: ... and the next sequence starts with that base
    seqs.append(rand_seq(rng, 20) + f)                               # 40: the whole primer at the very end (its last 9-gram at p = L - 9)
    seqs.append(rand_seq(rng, 20) + f + rand_seq(rng, 1))            # 41: one base before the end (p = L - 10)
    s = list(rand_seq(rng, 41)); s[41 - 32 + first:41 - 32 + first + 20] = f; seqs.append("".join(s))   # 41: the last regular window
    for h in (1, 2):                                                  # hanging over the end / the start by h bases (k = 2)
        seqs.append(rand_seq(rng, 20 + h) + f[:20 - h])              # 40
        seqs.append(f[h:] + rand_seq(rng, 21 + h))                   # 41
        seqs.append(revcomp(g)[h:] + rand_seq(rng, 40 - 19 + h))     # 40: the reverse primer's site over the start
    seqs.append(rand_seq(rng, 22) + f[:10])                          # 32: the first half of the primer at the end
    seqs.append(f[10:] + rand_seq(rng, 30))                          # 40: the other half behind the border
    assert sorted({len(q) for q in seqs}) == [32, 40, 41]
    _, want = _agree(trio, oracle, capfd, seqs, pairs, min_entries=6)
    hit = {e[3] for e in want}
    assert {0, 3, 4, 5} <= hit                                        # the whole sites are found
    assert 2 not in hit and len(seqs) - 1 not in hit                  # and nothing is made of a primer cut in two by a sequence border


def test_eos_split_and_inactive_sequence_after_the_index_was_built(trio, oracle, capfd):
    """The index is built by the first select; then an EOS is put into a site, another sequence is cut beside one and two
    sequences are switched off.  The index is not rebuilt: the validity bits and the per-block words say what has changed."""
    rng = random.Random(40004)
    root = rand_seq(rng, 700)
    seqs = [root] + [mutate(rng, root, 0.03) for _ in range(6)] + [rand_seq(rng, 500)]
    txt = []
    for i in range(10):
        a = 30 + 60 * i
        txt.append((root[a:a + 18 + i % 8], revcomp(root[a + 100:a + 100 + 25 - i % 8])))
    pairs = [(oracle.centered_word(x), oracle.centered_word(y)) for x, y in txt]
    so, before = _agree(trio, oracle, capfd, seqs, pairs, min_entries=50)
    cuts = [(0, 35), (2, 30 + 60 * 3 + 9), (2, 400), (5, 131)]        # inside a site (at its tenth base), inside another, between sites, beside one
    active = np.array([q not in (1, 6) for q in range(len(seqs))], dtype=np.uint8)
    for q, p in cuts:
        so.split(q, p)
    for q in range(len(seqs)):
        so.set_active(q, bool(active[q]))
    so.select(pairs)
    want = so.db_entries()
    capfd.readouterr()
    for d in trio:
        for q, p in cuts:
            d.split(q, p)
        d.set_active(active)
    got = [_entries_only(d, pairs, THR) for d in trio]
    err = capfd.readouterr().err
    forms = re.findall(r"scan plan: form=([\w-]+),", err)
    assert len(forms) >= 2 and set(forms) == {"seed3"}
    assert 0 < len(want) < len(before) and not any(e[3] in (1, 6) for e in want)
    assert got[0] == want and got[1] == want and got[2] == want


def test_more_orientations_than_one_launch_holds(trio, oracle, capfd):
    """250 pairs = 1 000 orientations: more than the 448 one launch of the third form takes, so the pass runs in several launch
    groups and each reads its own part of the span bytes."""
    rng = random.Random(250448)
    root = rand_seq(rng, 2400)
    seqs = [root] + [mutate(rng, root, 0.04) for _ in range(5)] + [rand_seq(rng, 800)]
    pairs = []
    for i in range(250):
        a = rng.randrange(0, 2100)
        f = root[a:a + rng.randint(18, 25)]
        r = revcomp(root[a + 110:a + 110 + rng.randint(18, 25)])
        pairs.append((oracle.centered_word(f), oracle.centered_word(r)))
    _agree(trio, oracle, capfd, seqs, pairs, min_entries=1000)


def test_iupac_primers(trio, oracle, capfd):
    """Primers with three two-fold slots each: their 10-gram codes fold into seeds whose span covers a base that is not in the
    slot's set (A|G covers C), and slots at the tenth base of a block widen the span."""
    rng = random.Random(353)
    root = rand_seq(rng, 1500)
    seqs = [root] + [mutate(rng, root, 0.04) for _ in range(7)] + [rand_seq(rng, 600)]
    two = {"A": "MRW", "C": "MSY", "G": "RSK", "T": "WYK"}
    pairs = []
    for i in range(16):
        a = 20 + 70 * i
        f, r = list(root[a:a + 18 + i % 8]), list(revcomp(root[a + 100:a + 100 + 25 - i % 8]))
        for o in (f, r):
            for p in rng.sample(range(len(o)), 3):
                o[p] = rng.choice(two[o[p]])
        pairs.append((oracle.centered_word("".join(f)), oracle.centered_word("".join(r))))
    _agree(trio, oracle, capfd, seqs, pairs, min_entries=100)
