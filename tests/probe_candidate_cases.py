"""The independent expectation for pcr_pool_probe_candidates, and the inputs its tests share.

Everything is restated from the scenario's texts with dictionaries and pcramp_amd.words: the insert of a record, its windows on
both strands, the rules on the word as oriented, the candidates of a group with their distinct sequences and records and their
first occurrence, the order and the cut.  The thermodynamic half takes a `melt` function (words -> results): the tests give it
the oracle's NucCruc or the device's own pcr_thermo.  Nothing here touches the call under test.

A scenario is dict(seqs=[text], splits=[(sequence, position)], records=PRODUCT array, group=uint32 array or None,
args=[dict of the call's arguments, ...]); every dict of `args` is one call the GPU test compares in full.
"""
import functools
import random

import numpy as np

import amplicon_seq_cases as AC
from amplicon_seq_cases import codes_of, plant, record, region_of, revcomp_text
from pcramp_amd import words as W

CANDIDATE = np.dtype([("word", np.uint64, (2,)), ("group", np.uint32), ("length", np.uint32), ("gc", np.uint32),
                      ("sequences", np.uint32), ("records", np.uint32), ("first_record", np.uint32), ("first_loc5", np.int32),
                      ("first_strand", np.uint32), ("tm", np.float32), ("hairpin_tm", np.float32), ("homodimer_tm", np.float32),
                      ("dG", np.float32)])
NO_5G, C_GE_G = 1, 2
NO_GROUP = 0xFFFFFFFF
MAX_GROUPS = 1024
A, C_, G, T = 1, 2, 4, 8                          # words._CODE
INSERT = AC.REGION_INSERT

# the call's arguments, with every rule off: a scenario's dicts override what they are about
OPEN = dict(len_min=20, len_max=30, strands=3, rules=0, max_run=0, gc_min=0.0, gc_max=1.0, min_sequences=1, per_group=0)
PROBE_RULES = dict(rules=NO_5G | C_GE_G, max_run=4, gc_min=0.3, gc_max=0.8)   # Screener.probe_candidates' defaults


def args_of(**kw):
    a = dict(OPEN)
    a.update(kw)
    return a


# ---------------------------------------------------------------------------------------------------------------- the model
def longest_run(w):
    best = run = 1
    for i in range(1, len(w)):
        run = run + 1 if w[i] == w[i - 1] else 1
        best = max(best, run)
    return best


def passes(w, a):
    """The rules on the word w (codes, 5' -> 3') as oriented."""
    n = len(w)
    c, g = int((w == C_).sum()), int((w == G).sum())
    frac = np.float32(c + g) / np.float32(n)
    if not (np.float32(a["gc_min"]) <= frac <= np.float32(a["gc_max"])):
        return False
    if a["max_run"] and longest_run(w) > a["max_run"]:
        return False
    if (a["rules"] & NO_5G) and w[0] == G:
        return False
    if (a["rules"] & C_GE_G) and c < g:
        return False
    return True


def insert_words(codes, start, length, a):
    """Every word an insert holds -> {word bytes: (loc5, strand) of its lowest occurrence in (loc5, strand)}."""
    out = {}
    ins = codes[start:start + length] if length else np.zeros(0, np.uint8)
    assert len(ins) == length, "the insert leaves the sequence"
    plain = np.isin(ins, (A, C_, G, T))
    for n in range(a["len_min"], a["len_max"] + 1):
        for off in range(0, length - n + 1):
            if not plain[off:off + n].all():
                continue
            w = ins[off:off + n]
            for strand in (1, 2):
                if not (a["strands"] & strand):
                    continue
                text = w if strand == 1 else W.revcomp_codes(w)
                if passes(text, a):
                    key = np.ascontiguousarray(text).tobytes()
                    at = (start + off, strand)
                    if key not in out or at < out[key]:
                        out[key] = at
    return out


def candidates(case, a, records=None, group=None):
    """-> the candidates before the thermodynamics and the cut: a list of dict(group, text (code bytes), length, gc, sequences,
    records, first = (sequence, record, loc5, strand), support = the set of sequences), in the call's order."""
    codes = codes_of(case)
    rec = case["records"] if records is None else records
    grp = case.get("group") if group is None else group
    by_interval = {}                                                         # (group, sequence, start, length) -> [record, ...]
    for k in range(len(rec)):
        g = 0 if grp is None else int(grp[k])
        if g == NO_GROUP:
            continue
        assert g < MAX_GROUPS
        start, length = region_of(rec[k], INSERT)
        s = int(rec[k]["sequence"])
        assert length >= 0 and (length == 0 or (0 <= start and start + length <= len(codes[s])))
        by_interval.setdefault((g, s, start, length), []).append(k)
    words_at = {}
    found = {}                                                               # (group, text) -> [(sequence, first record, loc5, strand, n records)]
    for (g, s, start, length), ks in by_interval.items():
        if (s, start, length) not in words_at:
            words_at[(s, start, length)] = insert_words(codes[s], start, length, a)
        for text, (loc5, strand) in words_at[(s, start, length)].items():
            found.setdefault((g, text), []).append((s, ks[0], loc5, strand, len(ks)))
    out = []
    for (g, text), occ in found.items():
        seqs = {o[0] for o in occ}
        if len(seqs) < a["min_sequences"]:
            continue
        w = np.frombuffer(text, np.uint8)
        out.append(dict(group=g, text=text, length=len(w), gc=int(np.isin(w, (C_, G)).sum()), sequences=len(seqs),
                        records=sum(o[4] for o in occ), first=min(o[:4] for o in occ), support=seqs))
    out.sort(key=lambda c: (c["group"], -c["sequences"], -c["records"], c["length"], c["text"]))   # codes 1 < 2 < 4 < 8: A < C < G < T
    return out


def word_of(c):
    return W.centered_word(np.frombuffer(c["text"], np.uint8))


def finish(cands, a, melt=None, limits=None, check_homo_dimer=False):
    """The thermodynamic filter and the cut -> CANDIDATE records.  melt(words) -> [dict(tm, hairpin_tm, homodimer_tm, dG)];
    limits = dict(tm_min, tm_max, max_hairpin, max_dimer)."""
    res = melt([word_of(c) for c in cands]) if melt is not None else None
    out, taken = [], {}
    for i, c in enumerate(cands):
        r = np.zeros(1, CANDIDATE)[0]
        if res is not None:
            m = res[i]
            hd = np.float32(m["homodimer_tm"]) if check_homo_dimer else np.float32(0)
            ok = (np.float32(limits["tm_min"]) <= m["tm"] <= np.float32(limits["tm_max"]) and m["hairpin_tm"] <= np.float32(limits["max_hairpin"])
                  and (not check_homo_dimer or hd <= np.float32(limits["max_dimer"])))
            if not ok:
                continue
            r["tm"], r["hairpin_tm"], r["homodimer_tm"], r["dG"] = m["tm"], m["hairpin_tm"], hd, m["dG"]
        if a["per_group"] and taken.get(c["group"], 0) >= a["per_group"]:
            continue
        taken[c["group"]] = taken.get(c["group"], 0) + 1
        r["word"] = word_of(c)
        r["group"], r["length"], r["gc"], r["sequences"], r["records"] = c["group"], c["length"], c["gc"], c["sequences"], c["records"]
        _, r["first_record"], r["first_loc5"], r["first_strand"] = c["first"]
        out.append(r)
    return np.array(out, CANDIDATE) if out else np.zeros(0, CANDIDATE)


def oracle_melt(oracle, salt, strand):
    """melt() from the oracle's NucCruc (orc_thermo_full)."""
    def melt(words):
        out = []
        for w in words:
            t = oracle.thermo_full(W.word_text(w), salt, strand)
            out.append(dict(tm=t[0], hairpin_tm=t[4], homodimer_tm=t[7], dG=t[3]))
        return out
    return melt


def groups_of(pool_len, ids, rec):
    """A record's group from the pool: the first pair i with {ids[2i], ids[2i + 1]} = {plus_oligo, minus_oligo}, else NO_GROUP."""
    first = {}
    for i in range(pool_len):
        first.setdefault(frozenset((int(ids[2 * i]), int(ids[2 * i + 1]))), i)
    return np.array([first.get(frozenset((int(p), int(m))), NO_GROUP) for p, m in zip(rec["plus_oligo"], rec["minus_oligo"])], np.uint32)


def as_bits(rec):
    """Records -> rows of sixteen uint32: every field, the floats as their bit patterns."""
    return np.ascontiguousarray(rec).view(np.uint32).reshape(-1, 16).tolist()


def window_count(case, a):
    """The windows the host adds up before the rules: sum over the participating records and L of max(0, insert - L + 1), times
    the strands."""
    grp = case.get("group")
    total = 0
    for k, r in enumerate(case["records"]):
        if grp is not None and int(grp[k]) == NO_GROUP:
            continue
        n = region_of(r, INSERT)[1]
        total += sum(max(0, n - L + 1) for L in range(a["len_min"], a["len_max"] + 1))
    return total * (2 if a["strands"] == 3 else 1)


# ---------------------------------------------------------------------------------------------------------------- scenarios
def _rand(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def _inserts(triples):
    return np.array([record(INSERT, *t) for t in triples], AC.PRODUCT)


EDGE_TAIL = 77


def edges_case():
    """Inserts of len_min - 1, len_min and len_min + 1 bases and an empty one; inserts that start at offsets 0, 1, 30 and 31 of a
    32-base block; one that ends on the last base of a 77-base sequence."""
    rng = random.Random(7101)
    triples = [(0, 64, 19), (0, 96, 20), (0, 130, 21), (0, 50, 0), (0, 64, 26), (0, 65, 26), (0, 94, 26), (0, 95, 26),
               (1, EDGE_TAIL - 23, 23), (1, EDGE_TAIL - 20, 20)]
    return dict(seqs=[_rand(rng, 200), _rand(rng, EDGE_TAIL)], records=_inserts(triples),
                args=[args_of(len_max=22), args_of(len_max=22, strands=1), args_of(len_max=22, strands=2), args_of(len_max=22, **PROBE_RULES)])


def lengths_case():
    """A 40-base insert at len_min = len_max = 1, = 32, and the whole range 1 .. 32."""
    rng = random.Random(7102)
    return dict(seqs=[_rand(rng, 120)], records=_inserts([(0, 37, 40)]),
                args=[args_of(len_min=1, len_max=1), args_of(len_min=32, len_max=32), args_of(len_min=1, len_max=32),
                      args_of(len_min=1, len_max=32, max_run=2, rules=NO_5G | C_GE_G, gc_min=0.25, gc_max=0.75)])


def long_case():
    """Inserts of 65 and 2 049 bases: start positions in a third block and in a 65th, some with an ambiguity code in reach."""
    rng = random.Random(7103)
    s = _rand(rng, 2300, "ACGT" * 40 + "RN")
    return dict(seqs=[s], records=_inserts([(0, 31, 65), (0, 120, 2049)]), args=[args_of(len_max=24), args_of(len_min=28, len_max=32, **PROBE_RULES)])


HOLE_AT = (40, 62, 83)                           # the first, a middle and the last base of the insert 40 .. 83


def holes_case():
    """One 44-base insert in seven copies of a sequence: whole; an EOS from a split at its first, a middle and its last base; an
    ambiguity code at the same three places.  Every copy is a group of its own."""
    rng = random.Random(7104)
    s = _rand(rng, 110)
    seqs = [s] * 4 + [plant(s, p, "N") for p in HOLE_AT]
    return dict(seqs=seqs, splits=[(1 + i, p) for i, p in enumerate(HOLE_AT)], records=_inserts([(i, 40, 44) for i in range(7)]),
                group=np.arange(7, dtype=np.uint32), args=[args_of(len_max=24), args_of(len_max=24, strands=1)])


def palindrome_case():
    """A 20-base insert that is its own reverse complement: one window, two occurrences, one candidate with records = 1."""
    rng = random.Random(7105)
    half = _rand(rng, 10)
    return dict(seqs=[plant(_rand(rng, 90), 33, half + revcomp_text(half))], records=_inserts([(0, 33, 20)]),
                args=[args_of(len_max=20), args_of(len_max=20, strands=1), args_of(len_max=20, strands=2)])


def twice_case():
    """One 20-mer twice in one insert (at 30 and at 57 of a 47-base insert from 30); and one sequence in two records of a group
    whose inserts overlap in that 20-mer's second copy."""
    rng = random.Random(7106)
    w = _rand(rng, 20)
    s = plant(plant(_rand(rng, 140), 30, w), 57, w)
    return dict(seqs=[s], records=_inserts([(0, 30, 47), (0, 50, 40)]), args=[args_of(len_max=20, strands=1), args_of(len_max=21)],
                word=w)


def both_strands_case():
    """One 24-base insert on the plus strand of sequence 0 and reverse-complemented in sequence 1."""
    rng = random.Random(7107)
    x = _rand(rng, 24)
    return dict(seqs=[plant(_rand(rng, 100), 40, x), plant(_rand(rng, 100), 51, revcomp_text(x))], records=_inserts([(0, 40, 24), (1, 51, 24)]),
                args=[args_of(len_min=24, len_max=24), args_of(len_min=24, len_max=24, strands=1), args_of(len_min=22, len_max=24, strands=2)])


def groups_case():
    """The same insert in two groups (5 and 1023), in a record that takes no part, and a NO_GROUP record whose interval lies
    outside its sequence."""
    rng = random.Random(7108)
    x = _rand(rng, 22)
    seqs = [plant(_rand(rng, 90), 30, x), plant(_rand(rng, 90), 44, x), plant(_rand(rng, 90), 12, x)]
    rec = _inserts([(0, 30, 22), (1, 44, 22), (2, 12, 22), (2, 80, 30), (7, 0, 25)])
    return dict(seqs=seqs, records=rec, group=np.array([5, 1023, NO_GROUP, NO_GROUP, NO_GROUP], np.uint32),
                args=[args_of(len_max=22), args_of(len_max=22, min_sequences=2)])


RULE_WORDS = dict(
    five_g="GACTACATCATTCAGTCAAC",           # 5' G as read; its reverse complement starts with G too (the last base is C)
    five_g_rc="AACTACATCATTCAGTCAAC",         # only the reverse complement starts with G
    c_gt_g="ACCTACATCATTCAGTCAAT",            # C 6, G 1: the plus strand passes C >= G, the reverse complement does not
    c_eq_g="ACGTACATGATTCAGTAAAT",            # C 3, G 3: a tie passes on both strands
    run4_first="AAAATCATCGTTCAGTCAGT",        # a run of exactly 4 at the first bases
    run5_first="AAAAACATCGTTCAGTCAGT",        # ... of 5
    run4_last="ACTATCATCGTTCAGCTTTT",         # ... of exactly 4 at the last bases
    run5_last="ACTATCATCGTTCAGTTTTT",
    gc_6="ACATACATCATTCAGTCAAT",              # 6 of 20: exactly gc_min = 0.3
    gc_5="ACATACATCATTCAGTAAAT",              # 5 of 20
    gc_16="GCGCCCGTCGCCGAGCCAGT",             # 16 of 20: exactly gc_max = 0.8
    gc_17="GCGCCCGTCGCCGAGCCGGT",             # 17 of 20
)


def rules_case():
    """One insert per word of RULE_WORDS, each a group of its own: every rule alone and all together."""
    rng = random.Random(7109)
    names = list(RULE_WORDS)
    seqs, triples = [], []
    for i, name in enumerate(names):
        w = RULE_WORDS[name]
        seqs.append(plant(_rand(rng, 80), 25 + i, w))
        triples.append((i, 25 + i, len(w)))
    return dict(seqs=seqs, records=_inserts(triples), group=np.arange(len(names), dtype=np.uint32), names=names,
                args=[args_of(len_max=20), args_of(len_max=20, rules=NO_5G), args_of(len_max=20, rules=C_GE_G), args_of(len_max=20, max_run=4),
                      args_of(len_max=20, gc_min=0.3, gc_max=0.8), args_of(len_max=20, **PROBE_RULES), args_of(len_max=20, max_run=1),
                      args_of(len_max=20, max_run=40)])


SUPPORT_TOP = 3


def support_case():
    """A 24-base insert shared by three sequences of group 0 (five 20-mers with sequences = records = 3: only the text orders
    them), two of which share two more bases; min_sequences at, below and above the top support; per_group through the tie."""
    rng = random.Random(7110)
    x = _rand(rng, 26)
    seqs = [plant(_rand(rng, 100), 30, x), plant(_rand(rng, 100), 41, x), plant(_rand(rng, 100), 52, x[:24]), _rand(rng, 100)]
    rec = _inserts([(0, 30, 26), (1, 41, 26), (2, 52, 24), (3, 20, 22)])
    base = dict(len_max=20, strands=1)
    return dict(seqs=seqs, records=rec,
                args=[args_of(**base), args_of(min_sequences=SUPPORT_TOP, **base), args_of(min_sequences=2, **base), args_of(min_sequences=SUPPORT_TOP + 1, **base),
                      args_of(per_group=2, **base), args_of(per_group=2, min_sequences=SUPPORT_TOP, **base), args_of(per_group=6, **base),
                      args_of(per_group=1, len_max=22, strands=3)])


def seq_ids_case():
    """amplicon_seq_cases' shared 37-base insert on sequences 0, 1, 63, 64 and 128 of 130."""
    sc = AC.classes_case("same")
    return dict(seqs=sc["seqs"], records=sc["records"], args=[args_of(len_max=21), args_of(len_max=21, min_sequences=5, per_group=3, **PROBE_RULES)])


MANY_RECORDS = 70001
MANY_INTERVALS = 300
MANY_LEN_MIN = 18                               # 8 start positions per 25-base insert: 560 008 in all, 2 188 chunks of 256


@functools.lru_cache(None)
def many_case():
    """70 001 records of 25-base inserts (300 intervals of the classes scenario's sequences, repeated in a scrambled order) in
    three groups: more chunks of 256 start positions than the enumeration's grid has blocks on an MI355X (8 per CU, 256 CUs), so its
    blocks take a second chunk."""
    seqs, _ = AC._class_seqs()
    rng = random.Random(7111)
    ivs = [(i % AC.CLASS_SEQS, 4 + (i * 7) % 50, 25) for i in range(MANY_INTERVALS)]
    one = [record(INSERT, *iv) for iv in ivs]
    pick = [rng.randrange(MANY_INTERVALS) for _ in range(MANY_RECORDS)]
    return dict(seqs=list(seqs), records=np.array([one[i] for i in pick], AC.PRODUCT), group=np.array([i % 3 for i in pick], np.uint32),
                args=[args_of(len_min=MANY_LEN_MIN, len_max=25, per_group=5, **PROBE_RULES)])


LOOP_AMP = (80, 200)
LOOP_GROUP_SEQS = ((0, 1, 2, 3), (2, 3, 4, 5))   # the sequences each pair amplifies


@functools.lru_cache(None)
def loop_case(oracle=None):
    """A panel of two exact-match pairs over six 420-base sequences.  Pair g's amplicon -- F_g, a 70-base insert, the reverse
    complement of R_g -- stands at 60 (pair 0) or 250 (pair 1) of every sequence of LOOP_GROUP_SEQS[g]: every insert lies more
    than 40 bases from either end of its sequence, so every window of it is a whole word of the DB.  The inserts of a group are
    one text, except that the last sequence of each group has one base changed in the middle: the candidates beside the change
    are held by all four sequences, the ones across it by three."""
    rng = random.Random(7112)
    seqs = [_rand(rng, 420) for _ in range(6)]
    panel = []
    for g, at in enumerate((60, 250)):
        f, r, ins = _rand(rng, 21), _rand(rng, 22), _rand(rng, 70)
        for s in LOOP_GROUP_SEQS[g]:
            x = ins
            if s == LOOP_GROUP_SEQS[g][-1]:
                x = plant(ins, 35, "A" if ins[35] != "A" else "C")
            seqs[s] = plant(seqs[s], at, f + x + revcomp_text(r))
        panel.append((W.centered_word(W.codes_from_text(f)), W.centered_word(W.codes_from_text(r))))
    return dict(seqs=seqs, panel=panel)


PANEL_SCENARIOS = ("random", "ladder")          # of products_tm_cases, through amplicon_seq_cases: real products, grouped by pool pair
PANEL_ARGS = dict(random=[args_of(len_min=22, len_max=23, per_group=8, **PROBE_RULES), args_of(len_min=18, len_max=19, strands=1, min_sequences=2)],
                  ladder=[args_of(len_max=24, per_group=8, **PROBE_RULES), args_of(len_min=18, len_max=20, strands=1)])
SYNTHETIC = ("edges", "lengths", "long", "holes", "palindrome", "twice", "both_strands", "groups", "rules", "support", "seq_ids", "many")
SCENARIO_NAMES = SYNTHETIC + PANEL_SCENARIOS
_MAKERS = dict(edges=edges_case, lengths=lengths_case, long=long_case, holes=holes_case, palindrome=palindrome_case, twice=twice_case,
               both_strands=both_strands_case, groups=groups_case, rules=rules_case, support=support_case, seq_ids=seq_ids_case, many=many_case)
_CASES = {}


def scenario(oracle, name):
    """name -> scenario; the panel scenarios need the oracle (products_tm_cases computes their products with it)."""
    if name not in _CASES:
        if name in PANEL_SCENARIOS:
            import products_tm_cases as PC
            sc = AC.scenario(oracle, name)
            ids = PC.all_products(oracle, name)[0]
            panel = sc["case"]["panel"]
            _CASES[name] = dict(seqs=sc["seqs"], splits=sc["splits"], records=sc["records"], group=groups_of(len(panel), ids, sc["records"]),
                                panel=panel, ids=ids, args=PANEL_ARGS[name])
        else:
            _CASES[name] = _MAKERS[name]()
            _CASES[name]["records"].setflags(write=False)
    return _CASES[name]


@functools.lru_cache(None)
def expected_candidates(oracle, name, i):
    """candidates() of a scenario's i-th argument set, computed once and shared (leave it unchanged)."""
    sc = scenario(oracle, name)
    return candidates(sc, sc["args"][i])


def expected(oracle, name, i):
    sc = scenario(oracle, name)
    return finish(expected_candidates(oracle, name, i), sc["args"][i])
