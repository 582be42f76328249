"""A sequence set whose largest word-DB bucket is chosen by the caller AND holds labelled amplicons (TEST INFRASTRUCTURE,
plain helper module, no GPU).

amplicon_edges.padded() grows a bucket with sites of one oligo on one strand: the sequence with the long bucket never
forms an amplicon.  Here the **dense sequence** carries, in the order of its bucket:

* a labelled amplicon at the very start of the bucket (pair 0, FR) and one at its very end (pair 2, RF, at amp_max);
* a run of revcomp(d2) copies, then runs of `n_sites` copies of the decoy oligo d1 (a minus site in front of a plus
  site never pairs: these are the far-outside majority); every 8th copy of the d1 run is followed by a near-copy with
  one or two substitutions, which the scan records while it has seen nothing better and the arg-max filter must drop;
* isolated blocks with one (d1, d2) amplicon each at amp_min - 1, amp_min, 140, amp_max, amp_max + 1, both orientations;
* a pair (`out`) whose only candidate amplicons are one base outside the window on either side;
* a pair (`cut`) with an EOS written as '-' inside one amplicon and a split() inside the other;
* a labelled amplicon (pair 1, FR) whose two sites enclose a poly-A stretch that the pair `lc` = (A20, T20) matches at
  every position in both roles: 2 x (LC_LEN - 19) = 1 162 entries between a site and its partner, admitted only under
  the wide window WIDE (0 .. 2000, the background screen's).

Around it: the window cases of amplicon_edges for pairs 0 and 2, sequences without entries, an inactive one, one whose
best d1 site is a near-copy (in the DB, below the identity threshold), and the sites of the `sparse` pair, which the
dense sequence does not hold.  `two=True` adds a second dense sequence.

    d = build(lib, "8k")               # lib: anything with centered_word() (the oracle)
    d.sc                                # an amplicon_edges.Scenario: expected(), expected_bounds() and the labels apply
    d.dense                             # indices of the dense sequences
    d.k                                 # pair indices by name: d, out, cut, lc, sparse (the labelled pairs are 0, 1, 2)
    wide(d.sc)                          # the same scenario under the wide window, labels recomputed

The size classes are named after the bucket size the set ends with.  The hit buckets start at 64 slots; a pass that
overflows them is repeated at the next power of two that holds the largest fill, and a pass that leaves them four times
too large is repeated with smaller ones.  The fill of a sequence counts hits, not entries: every hit that attained the
running maximum of its (sequence, candidate) when it was recorded, once per candidate word that found it.  On these
scenarios that is twice the entries of the dense sequence (+3), and with optimize_5 = optimize_3 = 1 about 39 hits per
planted site and 78 per position of the poly-A stretch, so the classes `s4k` / `s8k` that are selected that way have a
short stretch and few sites.  `n_sites` puts the fill at about 0.72 of the class's slots.
"""
import random
from collections import namedtuple

import amplicon_edges as AE
from testdata import rand_seq

Dense = namedtuple("Dense", "cls sc dense k n_near")
Class = namedtuple("Class", "n_sites lc_len entries cap")

LC_LEN = 600                            # the poly-A stretch: 2 * (LC_LEN - 19) entries of the pair `lc`
STEP = 23                               # a 20-mer and three random bases, as amplicon_edges.padded()
GAP = 260                               # more than amp_max: what lies on either side of a gap forms no amplicon under NARROW
NARROW = dict(amp_min=80, amp_max=200)
WIDE = dict(amp_min=0, amp_max=2000)

# class -> (n_sites, length of the poly-A stretch, band of DB entries in the dense sequence, slots per bucket the set ends
# with).  The band is what the oracle must count (tests/test_dense_buckets_host.py); the slots are what the device
# must report ("[pcramp] pass done: N-slot buckets, largest fill F"), asserted by every test of
# tests/test_gpu_dense_buckets.py.  Observed on an MI355X, (entries of the dense sequence, largest fill, slots):
#   4k: (1488, 2981, 4096)    8k: (2938, 5879, 8192)    32k: (11788, 23579, 32768)    64k: (23488, 46979, 65536)
#   s4k: (525, 2970, 4096)    s8k: (1500, 5895, 8192)        (selected with optimize_5 = optimize_3 = 1)
# With the bit-sliced scan alone (PCRAMP_SCAN=2) the fill is the number of entries and the four classes end one size lower.
# n_sites = 30000 (38698 entries) is refused: more than 65536 candidate sites in one sequence.
CLASSES = {
    "4k": Class(232, LC_LEN, (1100, 1900), 4096),
    "8k": Class(1392, LC_LEN, (2200, 3800), 8192),
    "32k": Class(8472, LC_LEN, (9000, 15000), 32768),
    "64k": Class(17832, LC_LEN, (18000, 30000), 65536),
    "s4k": Class(0, 40, (300, 900), 4096),
    "s8k": Class(60, 40, (1000, 2000), 8192),
}

def _near(rng, o, k):
    t = list(o)
    for j in rng.sample(range(3, len(o) - 3), k):
        t[j] = rng.choice([c for c in "ACGT" if c != o[j]])
    return "".join(t)


def _dense_sequence(lib, rng, txt, k, n_sites, lc_len):
    """-> (text, sites, eos in the text, split positions, labels as (pair, orient, amp_len, what), near-copies written)."""
    plan, raw, text_eos, split_eos, labels = [], [], [], [], []
    cur = [40]

    def site(role, pos, pair, which):
        plan.append((role, pos, txt[pair][0 if which == "F" else 1], (pair, which)))

    def amplicon(pair, orient, amp, what=None):
        f, r = txt[pair]
        plus, minus = ("F", "R") if orient == "FR" else ("R", "F")
        lm = len(r if orient == "FR" else f)
        a = cur[0]
        site("P", a, pair, plus)
        site("M", a + amp - lm, pair, minus)
        if what:
            labels.append((pair, orient, amp, what))
        cur[0] = a + amp + GAP
        return a

    def run(pair, which, role, n, near_every=0):
        n_near = 0
        for i in range(n):
            site(role, cur[0], pair, which)
            cur[0] += STEP
            if near_every and i % near_every == near_every - 1:
                raw.append((cur[0], _near(rng, txt[pair][0], 1 + (i // near_every) % 2)))
                cur[0] += STEP
                n_near += 1
        cur[0] += GAP
        return n_near

    amplicon(0, "FR", 150, "start of the dense bucket")
    run(k["d"], "R", "M", n_sites // 4)
    n_near = run(k["d"], "F", "P", n_sites // 2, near_every=8)
    for orient in ("FR", "RF"):
        for amp in (79, 80, 140, 200, 201):
            amplicon(k["d"], orient, amp, "decoy length %d in the dense bucket" % amp)
    amplicon(k["out"], "FR", 79, "only one base outside the window")
    amplicon(k["out"], "FR", 201)
    amplicon(k["out"], "RF", 201, "only one base outside the window")
    a = amplicon(k["cut"], "FR", 120, "EOS (text) inside, dense bucket")
    text_eos.append(a + 60)
    a = amplicon(k["cut"], "RF", 120, "EOS (split) inside, dense bucket")
    split_eos.append(a + 60)
    # the labelled amplicon across the low-complexity stretch
    f1, r1 = txt[1]
    a = cur[0]
    lc0 = a + len(f1) + 5
    site("P", a, 1, "F")
    for pos in range(lc0, lc0 + lc_len - 19):
        site("P", pos, k["lc"], "F")
        site("M", pos, k["lc"], "R")
    m = lc0 + lc_len + 5
    site("M", m, 1, "R")
    labels.append((1, "FR", m + len(r1) - a, "across the low-complexity stretch"))
    cur[0] = m + len(r1) + GAP
    n_near += run(k["d"], "F", "P", n_sites - n_sites // 2, near_every=8)
    amplicon(2, "RF", 200, "end of the dense bucket")
    L = cur[0] - GAP + 40
    L += L % 2
    s = list(rand_seq(rng, L))
    s[lc0 - 1] = s[lc0 + lc_len] = "C"                                     # the stretch ends where it is said to
    for pos, t in raw:
        s[pos:pos + len(t)] = list(t)
    sites = [AE.plant(lib, s, role, pos, o, None, oligo) for role, pos, o, oligo in plan]
    for e in text_eos:
        s[e] = "-"
    return "".join(s), sites, text_eos, split_eos, labels, n_near


def build(lib, cls, two=False, seed=20261016, n_sites=None, lc_len=None):
    """The dense scenario of size class `cls` (a key of CLASSES), deterministic from `seed`."""
    rng = random.Random("%d %s %d" % (seed, cls, two))
    n_sites = CLASSES[cls].n_sites if n_sites is None else n_sites
    lc_len = CLASSES[cls].lc_len if lc_len is None else lc_len
    lens = ((18, 18), (25, 25), (18, 25))                                 # the primer lengths of amplicon_edges' window cases
    txt = [(AE._primer(rng, lf), AE._primer(rng, lr)) for lf, lr in lens]
    k = {}
    for name in ("d", "out", "cut", "sparse"):
        k[name] = len(txt)
        txt.append((AE._primer(rng, 20), AE._primer(rng, 20)))
    k["lc"] = len(txt)
    txt.append(("A" * 20, "T" * 20))
    b = AE._Builder(lib, rng, txt)
    dense = []

    def add_dense():
        s, sites, text_eos, split_eos, labels, n_near = _dense_sequence(lib, rng, txt, k, n_sites, lc_len)
        i = len(b.seqs)
        b.seqs.append(s)
        b.sites.append(sites)
        b.eos.append(sorted(text_eos + split_eos))
        b.splits += [(i, e) for e in split_eos]
        b.labels += [AE.Label(i, p, orient, amp, None, what, False) for p, orient, amp, what in labels]
        dense.append(i)
        return n_near

    AE._window_cases(b, 0, 18, 18, 80, 200)
    b.seqs.append(rand_seq(rng, 300)); b.sites.append([]); b.eos.append([])                   # no entries
    n_near = add_dense()
    # its best d1 site is a near-copy: in the DB (the maximum of this sequence), below the identity threshold
    d1 = txt[k["d"]][0]
    b.add(300, [("P", 40, AE.identity(19, 20)), ("M", 40 + 120 - 20, None)], "near-copy is the best site", "FR", k["d"], 120,
          mutate={"P": _near(rng, d1, 1)})
    b.add(300, [("P", 40, None), ("M", 40 + 120 - 20, None)], "inactive", "FR", k["d"], 120, inactive=True)
    b.add(300, [("P", 40, None), ("M", 40 + 120 - 20, None)], "decoy pair in an ordinary sequence", "FR", k["d"], 120)
    for orient in ("FR", "RF"):
        b.add(260, [("P", 30, None), ("M", 30 + 150 - 20, None)], "sparse pair", orient, k["sparse"], 150)
    if two:
        n_near += add_dense()
    AE._window_cases(b, 2, 18, 25, 80, 200)
    b.seqs.append(rand_seq(rng, 120)); b.sites.append([]); b.eos.append([])
    sc = AE._finish("dense %s%s" % (cls, ", two dense sequences" if two else ""), b, txt, lib, NARROW)
    assert 8 <= len(sc.seqs) - len(dense) <= 40 and 0 < dense[0] and dense[-1] < len(sc.seqs) - 1
    return Dense(cls, sc, dense, k, n_near)


def wide(sc):
    """The scenario under the wide window: the labels' answers recomputed from the planted geometry."""
    sc = sc._replace(opts=dict(sc.opts, **WIDE), name=sc.name + ", wide window")
    fr, rf = AE.expected(sc)
    return sc._replace(labels=[l._replace(admitted=bool((fr if l.orient == "FR" else rf)[l.pair, l.seq])) for l in sc.labels])


def bucket(entries, seq):
    """The entries of one sequence, in bucket order (WordMatch::loc, then strand), of a sorted entries() / db_entries() list."""
    return sorted((e for e in entries if e[3] == seq), key=lambda e: (e[2], e[4]))
