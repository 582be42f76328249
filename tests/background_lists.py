"""Background sets whose candidate amplicon lists are as long as the caller says (TEST INFRASTRUCTURE, plain helper module, no GPU).

pcr_background_match pairs the word-DB entries of every sequence into candidate amplicons (PCR::collect_candidates,
pcr_assay.cpp:12-69), keeps them in per-wave lists, sub-lists and one list whose overflow repeats the pass, and has four
ways of getting there (k_bg_emit<64>, <128>, <0> by bucket size, <0> by batch width).  The random inputs of the other
tests form a handful of candidates per pair.  Here a **rack** sequence holds, for every distinct pair of a case, `nF`
copies of the site F binds and then `nR` copies of the reverse complement of the site R binds, each copy behind random
flank bases, all of it inside amp_max = 2000: the pair forms exactly nF * nR candidates on the rack (every F site with
every R site) and none in the other orientation.  F is its own reverse complement: find_background_match multiplies
the score of an oligo on its own strand with one on the opposite strand (background_match.cpp:82-83), so at the
reference's threshold of 0.8 -- where random bases add no candidates to the planted ones -- only such a pair sets a bit.
An F site is therefore a DB entry on either strand (2 nF + nR entries per pair in the rack's bucket).  Around the rack:

* a mutated rack (MF x MR sites, every site with MUT substitutions so that they tie in the word DB): the substitutions
  of the last F site and of one R site sit at the 5' end, where Smith-Waterman clips them, those of the others in the
  middle -- one of its MF * MR candidates scores above the others, and it has an odd index past the number of
  sequences, which the reference's index rule (background_match.cpp:122) never scores: where it alone reaches the
  background threshold the two modes differ (the host test asserts that they do);
* an inactive copy of the rack (no candidates), and a copy cut by a split() in the flank behind its first F site (the
  candidates of that site are cut: (nF - 1) * nR remain);
* unrelated random sequences (no entries).

Four sequences at most receive DB entries, so one workgroup of the pairing kernel -- and with it ONE of its 16 sub-lists
-- takes every record: a sub-list overflows long before the sum does.

A batch is the case's distinct pairs repeated cyclically (`batch`), and for the histogram cases filler pairs of random
primers behind them.  The word DB is selected with `select` -- the distinct pairs, once each: a repeated pair is a pair
of the batch like any other, but the hit buckets of the selection count hits per candidate oligo, so selecting with the
repeats would multiply the bucket size by the number of repeats and no wide batch could meet small buckets.  The oracle
answers per distinct pair; the rows of the repeats must equal the row of their original.

    c = cases(lib)["class64"]          # lib: anything with centered_word() (the oracle)
    c.seqs, c.inactive, c.splits       # the background set
    c.select, c.batch, c.origin        # pairs to select with; pairs of the call; batch index -> index into c.unique
    c.unique                           # the pairs the oracle is asked for: the c.n_distinct pairs of the rack, then the fillers
    c.per_pair                         # planted candidate count of unique pair k (None for a filler pair: ask the oracle)
    c.slots, c.form                    # bucket slots the set must end with, form of the pairing kernel that must run
    c.hook                             # PCRAMP_DEBUG_AMP_CAP to create the handle under (None: the library's own 2^20)

tests/test_background_lists_host.py holds the oracle to the planted counts and the bands; tests/test_gpu_background_lists.py
runs the cases on the device.
"""
import random
import re
from collections import namedtuple

from testdata import rand_seq, revcomp
from amplicon_edges import _primer, largest_bucket  # noqa: F401  (largest_bucket: re-exported for the tests)

BT, MULT = 0.8, 0.9                     # background threshold and search multiplier of every case (the reference's defaults)
AMP = (0, 2000)                         # opt.background_amplicon_range
MIN_LEN = 16                            # the 0.9 x min length of the background selection (main.cpp:592-601)
SITE = 20                               # primer length
MF, MR, MUT = 3, 4, 3                   # the mutated rack: sites per distinct pair, substitutions per site
N_UNRELATED = 5
SUB_LISTS = 16                          # BGE_SUB: sub-lists of the candidate list, amp_cap / 16 records each
DEFAULT_CAP = 1 << 20                   # pcr_ctx::amp_cap

Case = namedtuple("Case", "name seqs inactive splits select batch origin unique per_pair n_f n_r slots form hook racks n_distinct")

# Bucket slots by the entries of the largest bucket.  The hit buckets of a selection count HITS (pcr_select_words grows them to the
# next power of two that holds the largest fill), and on these sets every entry is found HITS_PER_ENTRY times, so the entries
# of the rack decide the slots: (entries of the largest bucket) -> slots the set ends with.
HITS_PER_ENTRY = 1


def slots_for(entries):
    fill = entries * HITS_PER_ENTRY
    s = 64
    while s < fill:
        s *= 2
    return s


def band(slots):
    """The entries the largest bucket may hold for the set to end at `slots` slots."""
    lo = 1 if slots == 64 else slots // 2 // HITS_PER_ENTRY + 1
    return lo, slots // HITS_PER_ENTRY


def _mutated(rng, o, where):
    """o with MUT substitutions: where = '5' (its first bases: clipped by the local alignment) or 'mid'."""
    t = list(o)
    js = range(MUT) if where == "5" else rng.sample(range(6, len(o) - 6), MUT)
    for j in js:
        t[j] = rng.choice([c for c in "ACGT" if c != o[j]])
    return "".join(t)


def _rack(rng, txt, n_f, n_r, mutated=False, cut_after_first=False, good_r=0):
    """-> (text, split position or None).  One segment per distinct pair: n_f F sites, then n_r revcomp(R) sites."""
    out, cut = [rand_seq(rng, 40)], None
    # every (F site, R site) combination of a segment within amp_max: sites of SITE bases behind 1-3 flank bases
    for f, r in txt:
        for i in range(n_f):
            out.append(_mutated(rng, f, "5" if i == n_f - 1 else "mid") if mutated else f)
            if cut_after_first and cut is None:
                flank = rand_seq(rng, 60)
                cut = sum(len(x) for x in out) + 30
                out.append(flank)
            else:
                out.append(rand_seq(rng, rng.randint(1, 3)))
        for j in range(n_r):
            # the plus strand holds revcomp(R): R's 5' end is the END of that text
            out.append(revcomp(_mutated(rng, r, "5" if j == good_r else "mid")) if mutated else revcomp(r))
            out.append(rand_seq(rng, rng.randint(1, 3)))
        out.append(rand_seq(rng, 30))
    s = "".join(out)
    return s + rand_seq(rng, 40 + len(s) % 2), cut


_SETS = {}


def _background_set(lib, n_f, n_r, n_distinct, seed):
    """The primers and sequences of a rack of n_f x n_r sites per distinct pair.  Random primers now and then match a site of
    another oligo at the collect threshold (10 of 20 bases) and add a candidate nobody planted, or an entry to an unrelated
    sequence: the set is drawn again until the oracle counts exactly the planted candidates and only the rack, the mutated
    rack and the cut copy hold entries (tests/test_background_lists_host.py asserts both)."""
    key = (n_f, n_r, n_distinct, seed)
    if key in _SETS:
        return _SETS[key]
    assert (n_f + n_r) * (SITE + 3) + 100 <= AMP[1]                       # every (F site, R site) combination inside amp_max
    for draw in range(50):
        rng = random.Random("%d rack %d %d %d %d" % (seed, n_f, n_r, n_distinct, draw))
        txt = []
        for _ in range(n_distinct):
            h = _primer(rng, SITE // 2)
            txt.append((h + revcomp(h), _primer(rng, SITE)))               # (F reads the same on either strand, see above)
        seqs, inactive, splits = [], [], []
        seqs.append(rand_seq(rng, 200))
        rack_i = len(seqs)
        seqs.append(_rack(rng, txt, n_f, n_r)[0])
        seqs.append(rand_seq(rng, 150))
        mut_i = len(seqs)
        # its one good candidate is number n_f n_r + (MF - 1) MR + good_r of the pair: odd, and past the number of sequences
        seqs.append(_rack(rng, txt, MF, MR, mutated=True, good_r=(n_f * n_r + (MF - 1) * MR + 1) % 2)[0])
        inactive.append(len(seqs))
        seqs.append(_rack(rng, txt, n_f, n_r)[0])
        s, cut = _rack(rng, txt, n_f, n_r, cut_after_first=True)
        cut_i = len(seqs)
        splits.append((len(seqs), cut))
        seqs.append(s)
        for _ in range(N_UNRELATED - 2):
            seqs.append(rand_seq(rng, rng.randint(120, 300)))
        distinct = [(lib.centered_word(f), lib.centered_word(r)) for f, r in txt]
        planted = n_f * n_r + MF * MR + n_f * n_r                         # rack + mutated rack + the cut copy ...
        per_pair = [planted - n_r] + [planted] * (n_distinct - 1)         # ... whose split is behind the first pair's first F site
        so = session(lib, seqs, inactive, splits, distinct)
        if [so.background_candidates(p, collect_threshold(), *AMP) for p in distinct] == per_pair \
                and {e[3] for e in so.db_entries()} == {rack_i, mut_i, cut_i}:     # (and no entry in an unrelated sequence)
            break
    else:
        raise AssertionError("no clean rack in 50 draws")
    _SETS[key] = (seqs, inactive, splits, distinct, per_pair, dict(rack=rack_i, mutated=mut_i, cut=cut_i))
    return _SETS[key]


def collect_threshold():
    """bg_threshold * bg_multiplier as the callers form it: a float32 product."""
    import numpy as np
    return float(np.float32(BT) * np.float32(MULT))


def session(lib, seqs, inactive, splits, select):
    """An oracle session holding the set as the device holds it (inactive flags and splits before the selection), its DB selected."""
    so = lib.session()
    for q in seqs:
        so.add_target(q)
    for i in inactive:
        so.set_active(i, False)
    for i, pos in splits:
        so.split(i, pos)
    so.select(select, threshold=collect_threshold(), min_len_override=MIN_LEN)
    return so


def _ballast(lib, seqs, inactive, splits, distinct, per_pair, n_sites, seed):
    """-> (a sequence of n_sites sites of a decoy oligo on one strand, the decoy pair): selected with the decoy pair, the set's
    largest bucket has n_sites entries and no candidate of any pair -- the same batch meets larger buckets."""
    for draw in range(50):
        rng = random.Random("%d ballast %d %d" % (seed, n_sites, draw))
        d1, d2 = _primer(rng, SITE), _primer(rng, SITE)
        q = rand_seq(rng, 30) + "".join(d1 + rand_seq(rng, 3) for _ in range(n_sites)) + rand_seq(rng, 30)
        decoy = (lib.centered_word(d1), lib.centered_word(d2))
        so = session(lib, seqs + [q], inactive, splits, distinct + [decoy])
        ent = so.db_entries()
        if [so.background_candidates(p, collect_threshold(), *AMP) for p in distinct + [decoy]] == per_pair + [0] \
                and sum(1 for e in ent if e[3] == len(seqs)) == n_sites and len({e[3] for e in ent}) == 4:
            return q, decoy
    raise AssertionError("no clean ballast in 50 draws")


def build(lib, name, n_f, n_r, n_distinct=3, n_batch=None, n_filler=0, hook=None, seed=20261020, ballast=0):
    seqs, inactive, splits, distinct, per_pair, racks = _background_set(lib, n_f, n_r, n_distinct, seed)
    select = distinct
    if ballast:
        q, decoy = _ballast(lib, seqs, inactive, splits, distinct, per_pair, ballast, seed)
        seqs, select, racks = seqs + [q], distinct + [decoy], dict(racks, ballast=len(seqs))
    n_batch = n_distinct if n_batch is None else n_batch
    n_rep = n_batch - n_filler
    frng = random.Random("%d filler" % seed)
    filler = [(lib.centered_word(_primer(frng, SITE)), lib.centered_word(_primer(frng, SITE))) for _ in range(n_filler)]
    batch = [distinct[i % n_distinct] for i in range(n_rep)] + filler
    origin = [i % n_distinct for i in range(n_rep)] + [n_distinct + i for i in range(n_filler)]
    slots = slots_for(max(n_distinct * (2 * n_f + n_r), ballast))         # (an F site is an entry on either strand)
    form = "emit<0>" if (2 * n_batch + 31) // 32 > 8 or slots > 128 else "emit<%d>" % slots   # pcr_background_match's choice
    return Case(name, seqs, inactive, splits, select, batch, origin, distinct + filler, per_pair + [None] * n_filler, n_f, n_r,
                slots, form, hook, racks, n_distinct)


def expected_records(c, filler_counts=()):
    """The records one pass must emit: the planted count of every batch pair (filler pairs: the oracle's, in batch order)."""
    fc = list(filler_counts)
    return sum(c.per_pair[o] if c.per_pair[o] is not None else fc[o - c.n_distinct] for o in c.origin)


def attempts(cap, n):
    """The list capacities pcr_background_match goes through when ONE sub-list takes all n records: a pass overflows when the
    sub-list (cap // 16 records) or the list is too small, and the next one has max(2 cap, 2 n) records."""
    caps = [cap]
    while n > caps[-1] // SUB_LISTS or n > caps[-1]:
        caps.append(max(2 * caps[-1], 2 * n))
        assert len(caps) < 12
    return caps


# (n_f, n_r) per distinct pair of the three-pair racks by the bucket slots the set must end with
RACK = {64: (5, 5), 128: (10, 12), 256: (15, 20)}
SPILL_NR = (13, 21, 32, 43, 63, 64)
LIMIT_PAIRS = 16384
LDS_PER_WORKGROUP = 160 * 1024          # what a workgroup of an MI355X may declare; 8 bytes of it per pair of a batch


def cases(lib):
    """name -> Case, every case of sections a-f."""
    out = {}

    def add(c):
        out[c.name] = c
    # a. the three forms by bucket class, three pairs
    for slots, (nf, nr) in RACK.items():
        add(build(lib, "class%d" % slots, nf, nr))
    # ... and the batch of class64 at larger buckets: the same sequences and a ballast sequence that no pair of the batch matches
    for slots, sites in ((128, 100), (256, 200)):
        add(build(lib, "ballast%d" % slots, *RACK[64], ballast=sites))
    # b. a wide batch on the 64-slot rack; 128 pairs is the widest batch of the staged forms
    for p in (128, 129, 200):
        add(build(lib, "wide%d" % p, *RACK[64], n_batch=p))
    # c. the wave list: one distinct pair repeated P times, so that an F site and a 64-lane chunk of its partners emit
    # P * nR records at once -- 63, 64, 65, 127, 128, 129 among them -- and thousands at P = 128
    for nr in SPILL_NR:
        for p in range(1, 6):
            add(build(lib, "spill_%d_%d" % (nr, p), max(1, (67 - nr) // 2), nr, n_distinct=1, n_batch=p))
    add(build(lib, "spill_24_128", (67 - 24) // 2, 24, n_distinct=1, n_batch=128))
    # d. more than 65 536 records in one sub-list at the library's own capacity
    add(build(lib, "natural", 4, 13, n_batch=600))
    # e. the list shrunk by the hook: n = the records of class64
    n = expected_records(out["class64"])
    for tag, hook in (("16", 16), ("256", 256), ("_n-1", n - 1), ("_n", n), ("_16n-1", 16 * n - 1), ("_16n", 16 * n)):
        add(build(lib, "hook" + tag, *RACK[64], hook=hook))
    # f. k_bg_compact's histogram on either side of 8192 pairs
    for p in (8192, 8193):
        add(build(lib, "hist%d" % p, 2, 2, n_batch=p, n_filler=p - 600))
    # g. as many pairs as the library takes in one call (16 384, if it takes more): mostly pairs that match nothing
    add(build(lib, "limit", 2, 2, n_batch=LIMIT_PAIRS, n_filler=LIMIT_PAIRS - 300))
    return out


Answers = namedtuple("Answers", "session entries counts records bits")
_ANSWERS = {}


def oracle_answers(lib, c):
    """What the oracle says about case c, computed once: its session (DB selected), db_entries(), the candidate count of every
    unique pair, the records a pass over the batch must emit, and bits[(evaluate_all, use_taq_mama)] = one row per UNIQUE pair
    (background_match with emulate_index_bug = not evaluate_all).  A pair without candidates has no bit: its rows are zero."""
    import numpy as np
    key = (c.name, id(lib))
    if key in _ANSWERS:
        return _ANSWERS[key]
    so = session(lib, c.seqs, c.inactive, c.splits, c.select)
    counts = [so.background_candidates(p, collect_threshold(), *AMP) for p in c.unique]
    bits = {}
    for ev in (False, True):
        for taq in (0, 1):
            rows = np.zeros((len(c.unique), len(c.seqs)), bool)
            for k, p in enumerate(c.unique):
                if counts[k]:
                    rows[k] = so.background_match(p, BT, MULT, AMP[0], AMP[1], taq, emulate_index_bug=int(not ev))[0].astype(bool)
            bits[(ev, taq)] = rows
    _ANSWERS[key] = Answers(so, so.db_entries(), counts, sum(counts[o] for o in c.origin), bits)
    return _ANSWERS[key]


# The "[pcramp] background_match:" line pcr_background_match writes per attempt under PCRAMP_DEBUG=1
LINE = re.compile(r"\[pcramp\] background_match: attempt (\d+), (emit<\d+>), (\d+)-slot buckets, (\d+) pairs, list of (\d+) records "
                  r"in sub-lists of (\d+), (\d+) records emitted, (\d+) kept, overflow (\d): ([a-z ]+)")
FIELDS = ("attempt", "form", "slots", "pairs", "cap", "sub_cap", "emitted", "kept", "overflow", "end")


def debug_lines(err):
    """The debug lines of a call's stderr -> one dict per attempt: the form that ran, the capacities, the records, how it ended."""
    out = []
    for m in LINE.finditer(err):
        g = m.groups()
        out.append(dict(zip(FIELDS, [int(g[0]), g[1]] + [int(x) for x in g[2:9]] + [g[9].strip()])))
    return out
