"""The independent expectation for pcr_select_sites, and the inputs its tests share.

expected_entries() restates the call's definition with the CPU oracle's pack and plain numpy: every entry Sequence::pack emits
for an active sequence, kept when some oligo c of the batch has (c & entry) >= unsigned(c.size() * threshold).  Nothing here
touches the library under test.
"""
import numpy as np

from testdata import mutate, rand_seq, revcomp

_M1 = np.uint64(0x1111111111111111)
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def _popcount64(x):
    return _POP8[np.ascontiguousarray(x, dtype=np.uint64).view(np.uint8).reshape(x.shape + (8,))].sum(axis=-1, dtype=np.uint32)


def _nonzero_nibbles(x):
    """Per u64: how many of its sixteen 4-bit slots are non-zero."""
    y = (x | (x >> np.uint64(1)) | (x >> np.uint64(2)) | (x >> np.uint64(3))) & _M1
    return _popcount64(y)


def word_and_np(c, w0, w1):
    """Word::operator& (word.cpp:151-154) of the word c with every word (w0[i], w1[i]): slots whose base sets intersect."""
    return _nonzero_nibbles(w0 & np.uint64(c[0])) + _nonzero_nibbles(w1 & np.uint64(c[1]))


def word_size_np(c):
    a = np.array([c[0], c[1]], dtype=np.uint64)
    return int(_nonzero_nibbles(a).sum())


def floor_of(c, thr):
    """select_words.cpp:83: unsigned(c.size() * threshold), a float product."""
    return int(np.float32(word_size_np(c)) * np.float32(thr))


def oligos_of(pairs):
    out = []
    for f, r in pairs:
        out.append((int(f[0]), int(f[1])))
        out.append((int(r[0]), int(r[1])))
    return out


def packed_entries(oracle, seqs, min_len=18, active=None, **pack_kw):
    """Sequence::pack of every active sequence -> structured columns (w0, w1, loc, index, strand) as numpy arrays."""
    rows = []
    for i, s in enumerate(seqs):
        if active is not None and not active[i]:
            continue
        rows.extend(oracle.pack(s, i, min_len=min_len, **pack_kw))
    if not rows:
        z = np.zeros(0, np.uint64)
        return z, z, []
    w0 = np.array([r[0] for r in rows], dtype=np.uint64)
    w1 = np.array([r[1] for r in rows], dtype=np.uint64)
    return w0, w1, rows


def counts_matrix(packed, oligos):
    """[n_oligos, n_entries] match counts."""
    w0, w1, _ = packed
    return np.stack([word_and_np(c, w0, w1) for c in oligos]) if len(oligos) else np.zeros((0, w0.size), np.uint32)


def expected_entries(oracle, seqs, pairs, thr, min_len=18, active=None, packed=None, counts=None, **pack_kw):
    """The sorted (w0, w1, loc, index, strand) tuples pcr_select_sites must leave.  packed / counts: results of
    packed_entries() / counts_matrix() for the same inputs, when several thresholds share them."""
    if packed is None:
        packed = packed_entries(oracle, seqs, min_len, active, **pack_kw)
    oligos = oligos_of(pairs)
    if counts is None:
        counts = counts_matrix(packed, oligos)
    keep = np.zeros(packed[0].size, dtype=bool)
    for k, c in enumerate(oligos):
        keep |= counts[k] >= floor_of(c, thr)
    rows = packed[2]
    return sorted(set(rows[i] for i in np.nonzero(keep)[0]))


def sites_per_oligo_and_sequence(oracle, seqs, pairs, thr, min_len=18):
    """max over (oligo, sequence) of the number of entries at or above the oligo's floor."""
    packed = packed_entries(oracle, seqs, min_len)
    idx = np.array([r[3] for r in packed[2]], dtype=np.int64)
    worst = 0
    for c in oligos_of(pairs):
        hit = word_and_np(c, packed[0], packed[1]) >= floor_of(c, thr)
        if hit.any():
            worst = max(worst, int(np.bincount(idx[hit]).max()))
    return worst


def argmax_filter(entries, pairs, thr):
    """select_words' filter (select_words.cpp:100-117) over a list of DB entries: per (oligo, sequence) the entries that
    attain the maximum count among those at or above the floor; the union over the oligos."""
    if not entries:
        return []
    w0 = np.array([e[0] for e in entries], dtype=np.uint64)
    w1 = np.array([e[1] for e in entries], dtype=np.uint64)
    idx = np.array([e[3] for e in entries], dtype=np.int64)
    keep = np.zeros(len(entries), dtype=bool)
    for c in oligos_of(pairs):
        cnt = word_and_np(c, w0, w1).astype(np.int64)
        cnt[cnt < floor_of(c, thr)] = -1
        best = np.full(int(idx.max()) + 1, -1, dtype=np.int64)
        np.maximum.at(best, idx, cnt)
        keep |= (cnt >= 0) & (cnt == best[idx])
    return sorted(entries[i] for i in np.nonzero(keep)[0])


# ---------------------------------------------------------------------------------------------------------------- inputs

def substitute(rng, s, k):
    """s with exactly k substitutions at distinct places."""
    out = list(s)
    for i in rng.sample(range(len(s)), k):
        out[i] = rng.choice([b for b in "ACGT" if b != out[i]])
    return "".join(out)


def plant(seq, at, site):
    assert 0 <= at and at + len(site) <= len(seq)
    return seq[:at] + site + seq[at + len(site):]


BORDER_LENGTHS = (1023, 1024, 1025, 1055, 1056, 1057, 2047, 2048, 2080, 5000)
BORDER_STARTS = (0, 1, 1000, 1020, 1023, 1024, 1025, 2047, 2048)


def border_case(rng, oracle):
    """Tile and block edges: on every sequence, 20-25-mer oligos cut so that the 32-slot window holding the centred oligo
    starts at each of BORDER_STARTS (where the sequence is long enough) and at the last regular window, plus the oligos at
    the very start and the very end of the sequence (irregular words), alternating strands; then four 3 % mutants of the
    5 000-base sequence, so that its oligos have sites with 0-3 mismatches elsewhere."""
    seqs = [rand_seq(rng, L) for L in BORDER_LENGTHS]
    oligo_txt = []
    for s in seqs:
        L = len(s)
        for p in [q for q in BORDER_STARTS if q + 32 <= L] + [L - 32]:
            n = rng.randint(20, 25)
            b = p + (33 - n)//2                         # Word::center(): the first base sits at slot (33 - n)/2
            oligo_txt.append(s[b:b + n])
        n = rng.randint(20, 25)
        oligo_txt.append(s[:n])
        n = rng.randint(20, 25)
        oligo_txt.append(s[L - n:])
    oligo_txt = [t if k % 2 else revcomp(t) for k, t in enumerate(oligo_txt)]
    base = seqs[-1]
    for _ in range(4):
        seqs.append(mutate(rng, base, 0.03))
    if len(oligo_txt) % 2:
        oligo_txt.append(revcomp(oligo_txt[0]))
    words = [oracle.centered_word(t) for t in oligo_txt]
    pairs = [(words[i], words[i + 1]) for i in range(0, len(words), 2)]
    return seqs, pairs


def single_site_case(rng, oracle, n_seq=6, L=700):
    """Sequences that each hold at most one site of each oligo: exact copies of two primer pairs in unrelated random sequences."""
    seqs, txt = [], []
    donor = rand_seq(rng, 400)
    pair_txt = [(donor[20:41], revcomp(donor[150:172])), (donor[200:219], revcomp(donor[330:354]))]
    for i in range(n_seq):
        s = rand_seq(rng, L + 13*i)
        for k, (f, r) in enumerate(pair_txt):
            if (i + k) % 3 == 2:
                continue                                # some sequences lack a pair
            at = 60 + 250*k + 7*i
            s = plant(s, at, f)
            s = plant(s, at + 120, revcomp(r))
        seqs.append(s)
    pairs = [(oracle.centered_word(f), oracle.centered_word(r)) for f, r in pair_txt]
    return seqs, pairs


def has_entry(entries, index, loc, strand):
    return any(e[2] == loc and e[3] == index and e[4] == strand for e in entries)


def window_loc(site_begin, n):
    """loc of the plus-strand DB entry (the 32-slot window) in which an n-mer at site_begin sits where Word::center() puts it."""
    return site_begin - (33 - n)//2


FLOOR_SITES = ((100, 0), (400, 2), (700, 3), (1000, 4))     # (where, substitutions)


def floor_case(rng, oracle):
    """One 20-mer; one sequence holding it with 0, 2, 3 and 4 substitutions."""
    s = rand_seq(rng, 1500)
    oligo = rand_seq(rng, 20)
    for at, k in FLOOR_SITES:
        s = plant(s, at, substitute(rng, oligo, k))
    other = rand_seq(rng, 21)                              # the pair's second oligo: no site anywhere
    return [s], [(oracle.centered_word(oligo), oracle.centered_word(other))]


SHORT_LENGTHS = (17, 18, 23, 31, 32, 33, 34, 35, 77)


def short_case(rng, oracle, min_n=18):
    """Sequences of a few words, oligos cut from both of their ends (both strands)."""
    seqs = [rand_seq(rng, L) for L in SHORT_LENGTHS]
    txt = []
    for k, s in enumerate(seqs):
        if len(s) < min_n:
            continue
        n = rng.randint(min_n, min(25, len(s)))
        txt.append(s[:n] if k % 2 else revcomp(s[:n]))
        n = rng.randint(min_n, min(25, len(s)))
        txt.append(revcomp(s[-n:]) if k % 2 else s[-n:])
    words = [oracle.centered_word(t) for t in txt]
    return seqs, [(words[i], words[i + 1]) for i in range(0, len(words) - 1, 2)]


def degenerate(rng, site, codes="RYN", k=2):
    """site with k slots widened to an IUPAC code that still holds the base (R = AG, Y = CT, N)."""
    holds = {"R": "AG", "Y": "CT", "N": "ACGT"}
    out = list(site)
    for i in rng.sample(range(len(site)), len(site)):
        fit = [c for c in codes if out[i] in holds[c]]
        if fit and k:
            out[i] = rng.choice(fit)
            k -= 1
    return "".join(out)


N_RUN_SITES = ((300, 5), (900, 4))                         # (site begin, length of the N run inside it)


def iupac_case(rng, oracle):
    """Degenerate oligos against plain targets, targets with IUPAC codes, a site holding a run of 5 N (every window over it
    exceeds pack_max_degen = 256 and is dropped) and one holding a run of 4 N (kept), an AT-rich and a GC-rich stretch with
    sites for the GC filter."""
    plain = rand_seq(rng, 1400)
    coded = rand_seq(rng, 1400, p_degen=0.01)
    oligo = rand_seq(rng, 22)
    nrun = rand_seq(rng, 1300)
    for at, k in N_RUN_SITES:
        nrun = plant(nrun, at, oligo[:8] + "N"*k + oligo[8 + k:])
    at_rich = "".join(rng.choice("AAATTTCG") for _ in range(200))
    gc_rich = "".join(rng.choice("CCCGGGAT") for _ in range(200))
    skew = rand_seq(rng, 300) + at_rich + rand_seq(rng, 300) + gc_rich + rand_seq(rng, 300)
    seqs = [plain, coded, nrun, skew]
    txt = [degenerate(rng, plain[200:221]), revcomp(degenerate(rng, plain[330:352])),
           degenerate(rng, plain[1379:1400], k=3), revcomp(coded[400:420].replace("N", "A")),
           oligo, revcomp(degenerate(rng, coded[40:63].replace("N", "C"), codes="N", k=1)),
           skew[380:400], revcomp(skew[1000:1024])]
    txt = [t if set(t) <= set("ACGTRYN") else "".join(c if c in "ACGTRYN" else "N" for c in t) for t in txt]
    words = [oracle.centered_word(t) for t in txt]
    return seqs, [(words[i], words[i + 1]) for i in range(0, len(words), 2)]


def groups_case(rng, oracle, n_pairs=130):
    """n_pairs pairs (every fifth a duplicate of an earlier one) cut from six sequences, a third of the oligos damaged."""
    seqs = [rand_seq(rng, 1500 + 37*i) for i in range(6)]
    pairs = []
    while len(pairs) < n_pairs:
        if len(pairs) % 5 == 4:
            pairs.append(pairs[rng.randrange(len(pairs))])
            continue
        s = rng.choice(seqs)
        a = rng.randrange(0, len(s) - 200)
        f = s[a:a + rng.randint(18, 25)]
        r = revcomp(s[a + 110:a + 110 + rng.randint(18, 25)])
        if rng.random() < 0.33:
            f = substitute(rng, f, 2)
        pairs.append((oracle.centered_word(f), oracle.centered_word(r)))
    return seqs, pairs


def blind_spot_case(rng, oracle):
    """Sequence 0: an exact F site, rc(R) with 2 substitutions 120 bases downstream, an exact rc(R) 3 000 bases away.
    Sequence 1: the exact pair only.  -> (seqs, pair, (begin, end) of the amplicon on both sequences)."""
    f, r_site = rand_seq(rng, 20), rand_seq(rng, 20)
    s0 = rand_seq(rng, 4200)
    s0 = plant(s0, 500, f)
    s0 = plant(s0, 620, substitute(rng, r_site, 2))
    s0 = plant(s0, 3500, r_site)
    s1 = rand_seq(rng, 1500)
    s1 = plant(s1, 500, f)
    s1 = plant(s1, 620, r_site)
    return [s0, s1], (oracle.centered_word(f), oracle.centered_word(revcomp(r_site))), (500, 639)


def pool_case(rng, oracle):
    """Pairs A and B with their exact products on both sequences; on sequence 0 a 2-mismatch site of A.F 150 bases upstream of
    B's rc(R) site.  -> (seqs, pool, (begin, end) of the spurious (A.F, B.R) product)."""
    af, ar, bf, br = (rand_seq(rng, n) for n in (20, 21, 22, 20))
    seqs = []
    for i in range(2):
        s = rand_seq(rng, 3000)
        s = plant(s, 300, af)
        s = plant(s, 420, ar)
        s = plant(s, 1500, bf)
        s = plant(s, 1620, br)
        seqs.append(s)
    seqs[0] = plant(seqs[0], 1470, substitute(rng, af, 2))
    w = oracle.centered_word
    pool = [(w(af), w(revcomp(ar))), (w(bf), w(revcomp(br)))]
    return seqs, pool, (1470, 1620 + len(br) - 1)
