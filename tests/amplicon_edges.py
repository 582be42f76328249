"""Planted amplicon geometry at the edges of the pairing rule (TEST INFRASTRUCTURE, plain helper module).

PCR::find_amplicon_match (pcr_assay.cpp:338-441) decides whether plus-strand site i and minus-strand site j of one
sequence form an admissible amplicon; PCR::extract_amplicon_seq (:443-542) is its multiplex twin.  The random
inputs of the other tests rarely land on an edge of that decision.  This module builds sequences that do: every
sequence is random background with primer sites planted at chosen positions, and carries a label -- what the
reference's rule answers for it, computed here from the planted geometry alone (`expected`).

    cases = scenarios(lib, seed)     # lib: anything with centered_word() (the oracle)
    for c in cases: c.seqs, c.weights, c.pairs, c.splits, c.inactive, c.labels, c.opts

A label is (pair index, orientation 'FR' / 'RF', built amplicon length, admitted, what it tests).  `expected(c)` gives
the bits per pair and orientation; `expected_bounds(c)` the (sequence, begin, end) records of collect_amplicons.
tests/test_amplicon_edges_host.py holds the oracle to these labels, so that no case drifts off its edge unnoticed.
"""
import bisect
import random
from collections import namedtuple

import numpy as np

from testdata import rand_seq, revcomp

PAD = 4                                   # MULTIPLEX_AMPLICON_PADDING (pcramp.h)
BASE_CODE = {"A": 1, "C": 2, "G": 4, "T": 8}

Scenario = namedtuple("Scenario", "name opts seqs weights pairs splits inactive labels sites eos")
Label = namedtuple("Label", "seq pair orient amp_len admitted what split_first_cut")
# split_first_cut: an EOS split() right after the minus site.  The labels hold for splits made after the word selection
# (has_split alone decides); made before it, Sequence::pack cuts the words around that EOS so that none holds the minus
# site at its position any more, and the case is refused (the only EOS case whose answer depends on the order)
# a planted site: role 'P' (plus-role primer on the plus strand) or 'M' (minus-role primer, reverse complement on the
# plus strand); pos = first template base of the site (may be < 0 or run past the end); n = primer length;
# ident = the float32 identity of the primer at that site; oligo = (pair, 'F' / 'R')
Site = namedtuple("Site", "role pos n ident oligo loc")


def f32(x):
    return np.float32(x)


def identity(cnt, n, taq=1.0):
    """update_identity (optimize.cpp:209-261) in float32: cnt * (float)(1.0/len), times the TaqMAMA factor."""
    v = f32(cnt) * f32(1.0 / n)
    return f32(v * f32(taq))


def pair_score(f, r):
    """sqrtf(f * r), correctly rounded: the identity test of pcr_assay.cpp:572-576 (the kernels' sqrtf(__fmul_rn(f, r)))."""
    return f32(np.sqrt(f32(f32(f) * f32(r))))


def plant(lib, s, role, pos, o, ident, oligo):
    """Write oligo text `o` (plus role) or its reverse complement (minus role) into the base list `s` at pos, cut where it runs
    off the sequence -> the Site the reference sees there."""
    L = len(s)
    t = o if role == "P" else revcomp(o)
    for j, c in enumerate(t):
        if 0 <= pos + j < L:
            s[pos + j] = c
    w = lib.centered_word(o)
    ws, we = lib.word_start(w), lib.word_stop(w)
    loc = pos - ws if role == "P" else pos + we                            # WordMatch::loc (sequence.h:57-75)
    if L % 2 and (loc + 31 > L - 1 if role == "P" else loc > L - 1):
        # a site that only a trailing partial word holds, in a sequence of odd length: Sequence::pack's position
        # counter has also stepped over the padding nibble of the last byte (sequence.cpp:198-263), so the
        # reference places the site one base towards the 3' end (plus role: towards the 5' end)
        loc += 1 if role == "M" else -1
    geo = loc + ws if role == "P" else loc - we                            # the template_loc5 the reference sees
    return Site(role, geo, len(o), f32(1.0) if ident is None else f32(ident), oligo, loc)


class _Builder:
    """Sequences of one scenario: each holds one planted geometry (or a few sites for the partner cases)."""

    def __init__(self, lib, rng, pairs_txt):
        self.lib = lib
        self.rng = rng
        self.pairs_txt = pairs_txt
        self.seqs, self.labels, self.sites, self.eos, self.splits, self.inactive = [], [], [], [], [], []

    def oligo(self, k, orient, role):
        f, r = self.pairs_txt[k]
        plus, minus = (f, r) if orient == "FR" else (r, f)
        return plus if role == "P" else minus

    def add(self, L, sites, what, orient, pair, amp_len, text_eos=(), split_eos=(), inactive=False, mutate=None,
            split_first_cut=False):
        """sites: [(role, pos, ident or None)] for oligos of `pair` in `orient`; the site text is the oligo (plus
        role) or its reverse complement (minus role), cut where it runs off the sequence; mutate: {role: text}."""
        s = list(rand_seq(self.rng, L))
        placed = []
        for role, pos, ident in sites:
            o = (mutate or {}).get(role) or self.oligo(pair, orient, role)
            which = ("F" if role == "P" else "R") if orient == "FR" else ("R" if role == "P" else "F")
            placed.append(plant(self.lib, s, role, pos, o, ident, (pair, which)))
        for e in text_eos:
            s[e] = "-"
        i = len(self.seqs)
        self.seqs.append("".join(s))
        self.sites.append(placed)
        self.eos.append(sorted(set(text_eos) | set(split_eos)))
        self.splits += [(i, e) for e in split_eos]
        if inactive:
            self.inactive.append(i)
        self.labels.append(Label(i, pair, orient, amp_len, None, what, split_first_cut))
        return i


def _site_pairs(sites, L, eos, amp_min, amp_max, collect=False):
    """The reference's loop over the planted sites of one orientation, sorted by WordMatch::loc (a plus and a minus site at
    one loc always overlap, so their order does not matter) -> list of (plus site, minus site, begin, end)."""
    out = []
    plus = sorted((s for s in sites if s.role == "P"), key=lambda s: s.loc)
    minus = sorted((s for s in sites if s.role == "M"), key=lambda s: s.loc)
    m_locs = [s.loc for s in minus]
    for p in plus:
        for q in minus[bisect.bisect_left(m_locs, p.loc):]:
            p3, m5 = p.pos + p.n - 1, q.pos
            if p3 >= m5:
                continue                                                   # overlap (:367-370)
            amp_start = p.pos
            m3 = q.pos + q.n - 1
            amp_stop = m3 if collect else min(m3, L - 1)
            amp_len = amp_stop - amp_start + 1
            if amp_len < amp_min:
                continue
            if amp_len > amp_max:
                break
            if collect:
                lo, hi = p3 + 1 - PAD, m5 + 2 * PAD                        # padded inner stretch (:489-497): the
                # start moves PAD bases left and the length grows by 2 PAD, so the stretch ends 2 PAD past the minus site
                if lo < 0 or hi > L or any(lo <= e < hi for e in eos):
                    break
                out.append((p, q, p.pos, m3))
                continue
            if amp_start < 0:
                amp_len += amp_start
                amp_start = 0
            if any(amp_start <= e < amp_start + amp_len for e in eos):
                break                                                      # has_split (:407-409)
            out.append((p, q, p.pos, m3))
    return out


def expected(sc):
    """-> (fr, rf): bool [n_pairs, n_seqs] of PCR::find_target_match over the planted sites."""
    o = sc.opts
    n, P = len(sc.seqs), len(sc.pairs)
    fr, rf = np.zeros((P, n), bool), np.zeros((P, n), bool)
    thr = f32(o["target_threshold"])
    for i, sites in enumerate(sc.sites):
        if i in sc.inactive:
            continue
        for k in range(P):
            for orient, dst in (("FR", fr), ("RF", rf)):
                plus_o, minus_o = ("F", "R") if orient == "FR" else ("R", "F")
                mine = [s for s in sites if s.oligo[0] == k and
                        ((s.role == "P" and s.oligo[1] == plus_o) or (s.role == "M" and s.oligo[1] == minus_o))]
                for p, q, _, _ in _site_pairs(mine, len(sc.seqs[i]), sc.eos[i], o["amp_min"], o["amp_max"]):
                    f, r = (p.ident, q.ident) if orient == "FR" else (q.ident, p.ident)
                    if pair_score(f, r) >= thr:
                        dst[k, i] = True
    return fr, rf


def split_first_answer(label):
    """What target_match answers for a labelled case when its splits are made before the word selection."""
    return label.admitted and not label.split_first_cut


def expected_bounds(sc, k):
    """-> sorted set of (sequence, begin, end) of PCR::extract_amplicon_seq for pair k over the planted sites (collect
    threshold = the scenario's target threshold; a planted site below its square is not matched).  A set: where Sequence::pack cuts
    two words at one position (the partial words at a 3' end) the reference lists the amplicon once per word."""
    o = sc.opts
    out = []
    per_oligo = f32(o["target_threshold"]) * f32(o["target_threshold"])   # an oligo's sites are matched at threshold^2 (:775-776)

    def matched(s):
        """A site takes part when it matches (unsigned)(length * threshold^2) bases of its oligo.  (Without TaqMAMA the
        identity is that count over the length; with it, every planted site of these scenarios matches.)"""
        return bool(o["use_taq_mama"]) or round(float(s.ident) * s.n) >= int(f32(s.n) * per_oligo)
    for orient in ("FR", "RF"):
        plus_o, minus_o = ("F", "R") if orient == "FR" else ("R", "F")
        for i, sites in enumerate(sc.sites):
            if i in sc.inactive:
                continue
            mine = [s for s in sites if s.oligo[0] == k and matched(s) and
                    ((s.role == "P" and s.oligo[1] == plus_o) or (s.role == "M" and s.oligo[1] == minus_o))]
            for p, q, b, e in _site_pairs(mine, len(sc.seqs[i]), sc.eos[i], o["amp_min"], o["amp_max"], collect=True):
                out.append((i, b & 0xFFFFFFFF, e))                      # begin is unsigned there (a 5' hang wraps)
    return sorted(set(out))


def _primer(rng, n):
    """A random primer without long runs (no low-complexity self-matches)."""
    while True:
        s = rand_seq(rng, n)
        if all(s[j:j + 4] != s[j] * 4 for j in range(n - 3)):
            return s


def _finish(name, b, pairs_txt, lib, opts, decoys=()):
    o = dict(target_threshold=1.0, search_multiplier=0.9, amp_min=80, amp_max=200, use_taq_mama=0,
             pack_max_degen=256, pack_min_gc=0.0, pack_max_gc=1.0, min_primer=18, optimize_5=0, optimize_3=0)
    o.update(opts)
    pairs = [(lib.centered_word(f), lib.centered_word(r)) for f, r in list(pairs_txt) + list(decoys)]
    sc = Scenario(name, o, b.seqs, [1.0 + 0.25 * (i % 7) for i in range(len(b.seqs))], pairs, b.splits,
                  b.inactive, b.labels, b.sites, b.eos)
    fr, rf = expected(sc)
    labels = [l._replace(admitted=bool((fr if l.orient == "FR" else rf)[l.pair, l.seq])) for l in b.labels]
    return sc._replace(labels=labels)


def _window_cases(b, k, lf, lr, amp_min, amp_max, flank=30):
    """amp_len at amp_min - 1 .. amp_max + 1, both orientations; adjacent and overlapping primers."""
    for orient in ("FR", "RF"):
        lp, lm = (lf, lr) if orient == "FR" else (lr, lf)
        for amp in (amp_min - 1, amp_min, amp_min + 1, amp_max - 1, amp_max, amp_max + 1):
            if amp < lp + lm:
                continue
            a = flank
            L = a + amp + flank
            b.add(L, [("P", a, None), ("M", a + amp - lm, None)], "length %d" % amp, orient, k, amp)
        for d, what in ((0, "adjacent primers"), (-1, "primers overlap by one"), (-3, "primers overlap by three")):
            a = flank
            amp = lp + lm + d
            if amp_min <= amp <= amp_max:
                b.add(a + amp + flank, [("P", a, None), ("M", a + lp + d, None)], what, orient, k, amp)


def _length_scenarios(lib, rng):
    out = []
    for amp_min, amp_max, lens in ((80, 200, ((18, 18), (25, 25), (18, 25))), (60, 61, ((18, 25), (25, 18))),
                                   (0, 2000, ((18, 25),))):
        pairs_txt = [(_primer(rng, lf), _primer(rng, lr)) for lf, lr in lens]
        b = _Builder(lib, rng, pairs_txt)
        for k, (lf, lr) in enumerate(lens):
            _window_cases(b, k, lf, lr, amp_min, amp_max)
            if amp_min == 0:                                               # the overlap edge under the wide window
                continue
            for orient in ("FR", "RF"):                                    # a whole sequence of amp_min -1 / 0 / +1
                lp, lm = (lf, lr) if orient == "FR" else (lr, lf)
                for L in (amp_min - 1, amp_min, amp_min + 1):
                    if L >= lp + lm:
                        b.add(L, [("P", 0, None), ("M", L - lm, None)], "sequence of length %d" % L, orient, k, L)
        out.append(_finish("window %d/%d" % (amp_min, amp_max), b, pairs_txt, lib, dict(amp_min=amp_min, amp_max=amp_max)))
    return out


def _partner_cases(b, k, lf, lr, amp_min, amp_max, decoy_txt):
    for orient in ("FR", "RF"):
        lp, lm = (lf, lr) if orient == "FR" else (lr, lf)
        a = 20
        # nearer minus site too short, farther one admissible
        b.add(a + amp_min + 60, [("P", a, None), ("M", a + amp_min - 1 - lm, None), ("M", a + amp_min + 10 - lm, None)],
              "near too short, far admissible", orient, k, amp_min + 10)
        # nearer admissible, farther too long
        b.add(a + amp_max + 40, [("P", a, None), ("M", a + amp_min + 5 - lm, None), ("M", a + amp_max + 1 - lm, None)],
              "near admissible, far too long", orient, k, amp_min + 5)
        # nearer too long only (the far one is farther still)
        b.add(a + amp_max + 80, [("P", a, None), ("M", a + amp_max + 1 - lm, None), ("M", a + amp_max + 30 - lm, None)],
              "both partners too long", orient, k, amp_max + 1)
        # two plus sites, one minus site: only the nearer plus site is in range
        b.add(a + amp_max + 80, [("P", a, None), ("P", a + 60, None), ("M", a + amp_max + 30 - lm, None)],
              "second plus site in range", orient, k, amp_max - 29)
        # an admissible partner behind many entries of other oligos (decoy sites between the two primers)
        i = b.add(a + amp_max + 40, [("P", a, None), ("M", a + amp_max - lm, None)], "behind decoy entries", orient, k, amp_max)
        s = list(b.seqs[i])
        d = decoy_txt
        for pos in range(a + lp + 2, a + amp_max - lm - len(d), len(d) + 1):
            s[pos:pos + len(d)] = list(d if (pos // (len(d) + 1)) % 2 else revcomp(d))
        b.seqs[i] = "".join(s)


def _partner_scenario(lib, rng):
    lens = ((18, 18), (25, 20))
    pairs_txt = [(_primer(rng, lf), _primer(rng, lr)) for lf, lr in lens]
    decoy = (_primer(rng, 20), _primer(rng, 20))
    b = _Builder(lib, rng, pairs_txt)
    for k, (lf, lr) in enumerate(lens):
        _partner_cases(b, k, lf, lr, 80, 200, decoy[0])
        for orient in ("FR", "RF"):                                        # inactive sequences with admissible amplicons
            b.add(200, [("P", 30, None), ("M", 30 + 120 - (lr if orient == "FR" else lf), None)], "inactive", orient, k, 120,
                  inactive=True)
    # two entries at one position on opposite strands: R = revcomp(F), so every F site is also an R site
    x = _primer(rng, 20)
    pairs_txt.append((x, revcomp(x)))
    k = len(pairs_txt) - 1
    b.pairs_txt = pairs_txt
    for amp in (79, 80, 150, 200, 201):
        b.add(30 + amp + 30, [("P", 30, None), ("M", 30, None), ("P", 30 + amp - 20, None), ("M", 30 + amp - 20, None)],
              "same position, opposite strands, length %d" % amp, "FR", k, amp)
    sc = _finish("partners", b, pairs_txt, lib, dict(), decoys=[decoy])
    return sc


def _clamp_scenario(lib, rng, opts=None, name="clamps and EOS"):
    """Primers hanging off either end (25-mers: a centred partial word of 26 - 2k bases holds the sites), and EOS
    (text '-' or split()) on both sides of each end of the amplicon and of the padded inner stretch.  The threshold lets
    a primer lose a few bases."""
    lens = ((25, 25), (25, 20))
    pairs_txt = [(_primer(rng, lf), _primer(rng, lr)) for lf, lr in lens]
    b = _Builder(lib, rng, pairs_txt)
    amp_min, amp_max = 80, 200
    for k, (lf, lr) in enumerate(lens):
        for orient in ("FR", "RF"):
            lp, lm = (lf, lr) if orient == "FR" else (lr, lf)
            if lp == 25:
                for hang in (1, 2, 3):                                     # plus primer off the 5' end
                    for amp in (amp_min - 1, amp_min, amp_min + hang, amp_max, amp_max + 1):
                        # built length = unclamped; the clamped length is amp - hang
                        b.add(amp - hang + 40, [("P", -hang, None), ("M", amp - hang - lm, None)],
                              "5' hang %d, length %d (clamped %d)" % (hang, amp, amp - hang), orient, k, amp)
            if lm == 25:
                for hang in (1, 2, 3):                                     # minus primer past the 3' end
                    for amp in (amp_min - 1, amp_min, amp_max, amp_max + 1):
                        a = 30
                        L = a + amp                                        # clamped amp_stop = L - 1
                        b.add(L, [("P", a, None), ("M", L - lm + hang, None)],
                              "3' hang %d, clamped length %d" % (hang, amp), orient, k, amp)
            # EOS on both sides of both ends of the amplicon and of the padded inner stretch, by split() after the word
            # selection (has_split alone decides: an EOS inside a primer's 32-base window also changes the words
            # Sequence::pack cuts there), and as text '-' inside the amplicon and just outside both windows
            a, amp = 40, 120
            L = a + amp + 40
            m = a + amp - lm
            for e in sorted({a - 1, a, a + amp - 1, a + amp, a + lp - PAD - 1, a + lp - PAD, m + PAD, m + 2 * PAD - 1, m + 2 * PAD}):
                b.add(L, [("P", a, None), ("M", m, None)], "EOS (split) at %d of [%d, %d)" % (e, a, a + amp), orient, k, amp,
                      split_eos=(e,), split_first_cut=(e == a + amp))
            for e in (a - 10, a + amp // 2, a + amp + 9):
                b.add(L, [("P", a, None), ("M", m, None)], "EOS (text) at %d of [%d, %d)" % (e, a, a + amp), orient, k, amp,
                      text_eos=(e,))
    o = dict(target_threshold=0.85)
    o.update(opts or {})
    return _finish(name, b, pairs_txt, lib, o)


def _identity_scenarios(lib, rng):
    """Primers with exactly k mismatches; target_threshold = the float32 score those mismatches give, and the floats
    on either side of it.  With TaqMAMA, the mismatch sits in one of the last two 3' bases."""
    out = []
    for lf, k_mis, taq in ((18, 1, 0), (25, 2, 0), (20, 1, 1), (22, 1, 1)):
        f, r = _primer(rng, lf), _primer(rng, 20)
        fm = list(f)
        if taq:
            j = lf - 1 if lf % 2 == 0 else lf - 2                           # the last or the penultimate 3' base
            js = [j]
        else:
            js = rng.sample(range(3, lf - 3), k_mis)
        for j in js:
            fm[j] = rng.choice([c for c in "ACGT" if c != f[j]])
        fm = "".join(fm)
        if taq:
            p1, p2, t1, t2 = (BASE_CODE[c] for c in (f[-2], f[-1], fm[-2], fm[-1]))
            fac_f = lib.taq_mama(p1, p2, t1, t2)
            fac_r = lib.taq_mama(BASE_CODE[r[-2]], BASE_CODE[r[-1]], BASE_CODE[r[-2]], BASE_CODE[r[-1]])
        else:
            fac_f = fac_r = 1.0
        idf, idr = identity(lf - len(js), lf, fac_f), identity(20, 20, fac_r)
        score = pair_score(idf, idr)
        for thr, tag in ((score, "at"), (np.nextafter(score, f32(2)), "above"), (np.nextafter(score, f32(0)), "below")):
            b = _Builder(lib, rng, [(f, r)])
            for orient in ("FR", "RF"):
                lp, lm = (lf, 20) if orient == "FR" else (20, lf)
                mut = {"P": fm} if orient == "FR" else {"M": fm}
                sites = [("P", 30, idf if orient == "FR" else idr), ("M", 30 + 100 - lm, idr if orient == "FR" else idf)]
                b.add(160, sites, "identity %s the threshold" % tag, orient, 0, 100, mutate=mut)
                b.add(160, [("P", 30, None), ("M", 30 + 100 - lm, None)], "exact primers", orient, 0, 100)
            out.append(_finish("identity %d-mer, %d mismatch(es), taq %d, threshold %s" % (lf, len(js), taq, tag), b, [(f, r)],
                               lib, dict(target_threshold=float(thr), use_taq_mama=taq)))
    return out


N_SCENARIOS = 18


def scenarios(lib, seed=20261016):
    """Every planted scenario, deterministic from `seed`."""
    rng = random.Random(seed)
    out = _length_scenarios(lib, rng)
    out.append(_partner_scenario(lib, rng))
    out.append(_clamp_scenario(lib, rng))
    out.append(_clamp_scenario(lib, random.Random(seed + 1), dict(optimize_5=1, optimize_3=1), "clamps and EOS, shift candidates"))
    out += _identity_scenarios(lib, rng)
    return out


def padded(sc, lib, n_copies, seed=7):
    """The scenario plus one decoy sequence holding n_copies sites of a decoy oligo (and a decoy pair that selects them):
    its DB bucket grows with n_copies, so the largest bucket -- and with it the form of the fused tail and of the move
    kernels -- is chosen by the caller.  The labels and expected bits of the planted sequences are unchanged; the decoy
    sequence has no amplicon of any planted pair."""
    rng = random.Random(seed)
    d1, d2 = _primer(rng, 20), _primer(rng, 20)
    sc = sc._replace(name="%s + %d decoy sites" % (sc.name, n_copies), pairs=list(sc.pairs) + [(lib.centered_word(d1), lib.centered_word(d2))])
    if n_copies == 0:                                                      # the decoy pair alone
        return sc
    s = "".join(d1 + rand_seq(rng, 3) for _ in range(n_copies))
    return sc._replace(seqs=list(sc.seqs) + [s], weights=list(sc.weights) + [1.0], sites=list(sc.sites) + [[]],
                       eos=list(sc.eos) + [[]])


def largest_bucket(entries):
    """Largest number of DB entries of one sequence in a sorted entries() / db_entries() list."""
    from collections import Counter
    c = Counter(e[3] for e in entries)
    return max(c.values()) if c else 0
