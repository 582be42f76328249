"""The independent expectation for pcr_pool_amplicons, and the inputs its tests share.

Everything is restated from the scenario's texts: codes from words.codes_from_text ('-' and every split position are code 0),
the region of a record, its spelling and canonical choice, length / gc / other, the classes by first appearance with their
copies and distinct sequences, and the packed unique amplicons.  Nothing here touches the library under test.

A scenario is dict(seqs=[text], splits=[(sequence, position)], records=PRODUCT array, regions=(region, ...)); the scenarios
that come from products_tm_cases also carry that case (panel, thr, amp) under "case".
"""
import functools
import random

import numpy as np

from pcramp_amd import words as W

PRODUCT = np.dtype([("plus_oligo", np.uint32), ("minus_oligo", np.uint32), ("sequence", np.uint32), ("begin", np.int32),
                    ("end", np.int32), ("inner_start", np.int32), ("inner_length", np.int32), ("intended", np.uint32)])
INFO = np.dtype([("length", np.uint32), ("gc", np.uint32), ("other", np.uint32), ("flags", np.uint32),
                 ("amplicon", np.uint32), ("first", np.uint32), ("copies", np.uint32), ("sequences", np.uint32)])
INFO_FIELDS = ("length", "gc", "other", "flags", "amplicon", "first", "copies", "sequences")
REVERSED = 1
REGION_PRODUCT, REGION_INSERT, REGION_INNER = 0, 1, 2
REGIONS = (REGION_PRODUCT, REGION_INSERT, REGION_INNER)


# ---------------------------------------------------------------------------------------------------------------- the model
def codes_of(case):
    """The set as the device holds it: one uint8 code array per sequence, '-' and the split positions 0."""
    codes = [W.codes_from_text(s).copy() for s in case["seqs"]]
    for s, p in case.get("splits", ()):
        codes[s][p] = 0
    return codes


def region_of(rec, region):
    """-> (first position, length) of the record's region."""
    if region == REGION_PRODUCT:
        return int(rec["begin"]), int(rec["end"]) - int(rec["begin"]) + 1
    if region == REGION_INSERT:
        return int(rec["inner_start"]) + 4, int(rec["inner_length"]) - 12
    assert region == REGION_INNER
    return int(rec["inner_start"]), int(rec["inner_length"])


def spell(codes, start, length, canonical):
    """-> (the spelling as a uint8 code array, reversed?): forward, or with canonical the smaller of forward and reverse
    complement compared position by position as unsigned codes (bytes compare that way)."""
    f = codes[start:start + length] if length else np.zeros(0, np.uint8)
    assert len(f) == length, "the region leaves the sequence"
    if canonical:
        rc = W.revcomp_codes(f)
        if rc.tobytes() < f.tobytes():
            return np.ascontiguousarray(rc), True
    return np.ascontiguousarray(f), False


def first_difference(codes, start, length):
    """The first position at which a region's forward and reverse-complement spellings differ (None: reverse-palindromic)."""
    f = codes[start:start + length]
    d = np.nonzero(f != W.revcomp_codes(f))[0]
    return int(d[0]) if len(d) else None


def model(case, region, canonical, records=None):
    """-> dict(info, n_classes, class_length, class_byte_offset, packed, packed_bytes, texts, spellings) for the scenario's
    records (or `records`) by the definition in include/pcramp_hip.h."""
    codes = codes_of(case)
    rec = case["records"] if records is None else records
    n = len(rec)
    info = np.zeros(n, INFO)
    first_of, members = {}, []
    spelled = {}
    for k in range(n):
        s = int(rec[k]["sequence"])
        start, length = region_of(rec[k], region)
        assert length >= 0 and (length == 0 or (0 <= start and start + length <= len(codes[s])))
        key = (s, start, length)
        if key not in spelled:
            sp, rev = spell(codes[s], start, length, canonical)
            spelled[key] = (sp.tobytes(), rev, int(np.isin(sp, (2, 4, 6)).sum()), int((~np.isin(sp, (1, 2, 4, 8))).sum()))
        text, rev, gc, other = spelled[key]
        c = first_of.setdefault(text, len(first_of))                          # one byte per code: equal bytes = equal length and codes
        if c == len(members):
            members.append([])
        members[c].append(k)
        info[k]["length"], info[k]["gc"], info[k]["other"], info[k]["flags"] = length, gc, other, REVERSED if rev else 0
        info[k]["amplicon"] = c
    for c, ks in enumerate(members):
        info["first"][ks] = ks[0]
        info["copies"][ks] = len(ks)
        info["sequences"][ks] = len({int(rec[k]["sequence"]) for k in ks})
    spellings = [np.frombuffer(t, np.uint8) for t in first_of]                # (insertion order: class order)
    packs = [W.pack_codes(sp) if len(sp) else np.zeros(0, np.uint8) for sp in spellings]
    lengths = np.array([len(sp) for sp in spellings], np.uint64)
    sizes = np.array([len(p) for p in packs], np.uint64)
    offsets = np.concatenate([np.zeros(1, np.uint64), np.cumsum(sizes, dtype=np.uint64)])[:len(packs)]
    packed = np.concatenate(packs) if packs else np.zeros(0, np.uint8)
    return dict(info=info, n_classes=len(spellings), class_length=lengths, class_byte_offset=offsets, packed=packed,
                packed_bytes=int(sizes.sum()), texts=[W.text_from_codes(sp) for sp in spellings], spellings=spellings)


# ---------------------------------------------------------------------------------------------------------------- scenarios
def _rand(rng, n, letters="ACGT"):
    return "".join(rng.choice(letters) for _ in range(n))


def revcomp_text(text):
    return W.text_from_codes(W.revcomp_codes(W.codes_from_text(text)))


def plant(seq, at, text):
    return seq[:at] + text + seq[at + len(text):]


def record(kind, seq, start, length):
    """A record whose `kind` region is start .. start + length - 1 of sequence seq (the fields of the other regions are 0)."""
    r = np.zeros(1, PRODUCT)[0]
    r["sequence"] = seq
    if kind == REGION_PRODUCT:
        r["begin"], r["end"] = start, start + length - 1
    elif kind == REGION_INSERT:
        r["inner_start"], r["inner_length"] = start - 4, length + 12
    else:
        r["inner_start"], r["inner_length"] = start, length
    return r


def _records(kind, triples):
    return np.array([record(kind, *t) for t in triples], PRODUCT)


ALIGN_STARTS = (64, 65, 95)                      # offsets 0, 1 and 31 of a 32-base block
ALIGN_LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 2049, 4097)   # the last two: more than 64 lanes x 32 bases, a lane takes a second block
ALIGN_TAIL_LEN = 77                              # a sequence whose length is no multiple of 32


def alignment_case():
    """Regions at every alignment of their first and last base within a 32-base block and at every block count up to a second
    pass of the wave; a region that ends at the last base of a 77-base sequence, that whole sequence, and a region in the last
    sequence of the set.  The long sequence carries a few ambiguity codes."""
    rng = random.Random(6101)
    s0 = _rand(rng, 4300, "ACGT" * 12 + "RYN")
    s1 = _rand(rng, ALIGN_TAIL_LEN)
    s2 = _rand(rng, 100)
    triples = [(0, a, n) for a in ALIGN_STARTS for n in ALIGN_LENGTHS]
    triples += [(1, 40, ALIGN_TAIL_LEN - 40), (1, 0, ALIGN_TAIL_LEN), (2, 3, 50), (2, 68, 32)]
    return dict(seqs=[s0, s1, s2], records=_records(REGION_PRODUCT, triples), regions=(REGION_PRODUCT,))


STRANDS = dict(fwd=0, rev=1, palindrome=2, single=3, middle=4, middle_long=5, iupac=6, iupac_rev=7, whole=8, split=9)
STRANDS_SPLIT_AT = 25


def strands_case():
    """One insert forward in sequence 0 and reverse-complemented in sequence 1; a reverse-palindromic insert; a single base (its
    two spellings differ at the last = only position); inserts that are reverse-palindromic except for their two central bases, so
    that the spellings first differ at length/2 - 1 -- the last position at which a first difference can stand, since the
    complement is an involution and a difference at i is one at length - 1 - i -- one of them 4 200 bases long: the deciding
    block is the wave's second pass; an insert of ambiguity codes and its reverse complement; and sequence 0's insert again in
    a copy of the sequence that is split inside it."""
    rng = random.Random(6102)
    x = _rand(rng, 45)
    half = _rand(rng, 20)
    pal = half + revcomp_text(half)
    h35 = _rand(rng, 34)
    mid = h35 + "AC" + revcomp_text(h35)                                     # A.. vs rc: position 34 holds A, rc holds G (comp of C)
    h2k = _rand(rng, 2099)
    mid_long = h2k + "TG" + revcomp_text(h2k)                                # forward T (8) > rc C (2): REVERSED
    iu = "ACRYMKSWNNBDHVGT" + _rand(rng, 24, "RYMKSWN")
    seqs = [plant(_rand(rng, 120), 20, x), plant(_rand(rng, 120), 30, revcomp_text(x)), plant(_rand(rng, 90), 10, pal),
            _rand(rng, 64), plant(_rand(rng, 130), 33, mid), plant(_rand(rng, 4300), 50, mid_long),
            plant(_rand(rng, 100), 31, iu), plant(_rand(rng, 100), 7, revcomp_text(iu))]
    seqs += [seqs[0], seqs[0]]                                               # 8: a copy; 9: a copy split inside the insert
    triples = [(0, 20, 45), (1, 30, 45), (2, 10, 40), (3, 17, 1), (4, 33, 70), (5, 50, 4200), (6, 31, 40), (7, 7, 40),
               (8, 20, 45), (9, 20, 45)]
    return dict(seqs=seqs, splits=[(9, STRANDS_SPLIT_AT)], records=_records(REGION_INSERT, triples), regions=(REGION_INSERT,))


CLASS_SEQS = 130
CLASS_INSERT_AT = 40
CLASS_SHARED = (0, 1, 63, 64, 128)               # the sequences that hold the shared insert


@functools.lru_cache(None)
def _class_seqs():
    """130 sequences of 140 bases.  CLASS_SHARED hold one 37-base insert X at 40; sequence 5 holds X twice (at 40 and 90);
    sequence 6 holds X with its last base changed, sequence 7 X followed by one more planted base."""
    rng = random.Random(6103)
    x = _rand(rng, 37)
    seqs = [_rand(rng, 140) for _ in range(CLASS_SEQS)]
    for s in CLASS_SHARED:
        seqs[s] = plant(seqs[s], CLASS_INSERT_AT, x)
    seqs[5] = plant(plant(seqs[5], 40, x), 90, x)
    seqs[6] = plant(seqs[6], 40, x[:-1] + ("A" if x[-1] != "A" else "C"))
    seqs[7] = plant(seqs[7], 40, x + "G")
    seqs[0] = plant(seqs[0], CLASS_INSERT_AT + 37, "T")                      # X + T on sequence 0, X + G on sequence 7
    seqs[100] = plant(seqs[100], 12, "A")
    seqs[129] = plant(seqs[129], 139, "C")
    return tuple(seqs), x


def classes_case(which):
    seqs, x = _class_seqs()
    n = len(x)
    if which == "same":                          # one class: 9 records, 5 sequences
        triples = [(s, CLASS_INSERT_AT, n) for s in CLASS_SHARED] + [(63, CLASS_INSERT_AT, n)] * 2 + [(128, CLASS_INSERT_AT, n), (0, CLASS_INSERT_AT, n)]
    elif which == "distinct":                    # 12 records, 12 classes
        triples = [(s, 3 + 5 * s, 20 + s) for s in range(8, 20)]
    elif which == "empty":                       # an empty INSERT alone
        triples = [(64, 50, 0)]
    else:
        assert which == "mixed"
        triples = [(5, 40, n), (5, 90, n),       # equal regions on one sequence: copies 2 (+ the shared ones), sequences counted once
                   (6, 40, n),                   # differs at the last base only
                   (7, 40, n + 1), (0, 40, n + 1),   # one more base: G on 7, T on 0
                   (63, 40, n), (64, 40, n), (128, 40, n),
                   (100, 12, 0), (3, 77, 0),     # two empty inserts: one class
                   (7, 40, n),                   # X again, as a prefix of the longer one
                   (100, 12, 1), (129, 139, 1)]  # single bases A and C; the last base of the last sequence
    return dict(seqs=list(seqs), records=_records(REGION_INSERT, triples), regions=(REGION_INSERT,))


PACKING_LENGTHS = (3, 5, 4, 6, 7, 2, 1, 9, 8, 33, 64, 65, 31, 32, 11, 10, 12, 96, 40)   # odd-odd, odd-even, even-even, even-odd neighbours; long ones at byte offsets that are and are not multiples of 4


def packing_case():
    """INNER stretches of odd and even lengths in every order of neighbours, all of different lengths: byte offsets after padded tails."""
    rng = random.Random(6104)
    seqs = [_rand(rng, 900), _rand(rng, 333)]
    triples, at = [], [5, 2]
    for i, n in enumerate(PACKING_LENGTHS):
        s = i & 1
        triples.append((s, at[s], n))
        at[s] += n + 3
    return dict(seqs=seqs, records=_records(REGION_INNER, triples), regions=(REGION_INNER,))


MANY_RECORDS = 70001
MANY_INTERVALS = 300


@functools.lru_cache(None)
def many_case():
    """70 001 records that repeat 300 intervals of the classes scenario's sequences in a scrambled order: more than 65 536."""
    seqs, _ = _class_seqs()
    rng = random.Random(6105)
    ivs = [(i % CLASS_SEQS, 4 + (i * 7) % 50, 20 + i % 37) for i in range(MANY_INTERVALS)]
    one = {iv: record(REGION_PRODUCT, *iv) for iv in ivs}
    rec = np.array([one[ivs[rng.randrange(MANY_INTERVALS)]] for _ in range(MANY_RECORDS)], PRODUCT)
    return dict(seqs=list(seqs), records=rec, regions=(REGION_PRODUCT,))


PANEL_SCENARIOS = ("random", "words", "ladder")  # of products_tm_cases: realistic records, all three regions
ORACLE_SCENARIOS = PANEL_SCENARIOS + ("split_wide",)   # the last: a select_words DB (the oracle's own) over a split sequence
SYNTHETIC = ("alignment", "strands", "classes_same", "classes_distinct", "classes_mixed", "classes_empty", "packing", "many")
SCENARIO_NAMES = SYNTHETIC + PANEL_SCENARIOS

# the number of classes each synthetic scenario was built to have: (canonical = 0, canonical = 1); alignment's single bases at 65
# and 95 are each other's complement
CLASS_COUNTS = dict(alignment=(34, 33), many=(MANY_INTERVALS, MANY_INTERVALS), strands=(9, 7), classes_same=(1, 1), classes_distinct=(12, 12), classes_mixed=(7, 7), classes_empty=(1, 1),
                    packing=(len(PACKING_LENGTHS), len(PACKING_LENGTHS)))

_CASES = {}


def scenario(oracle, name):
    """name -> scenario; the panel scenarios need the oracle (products_tm_cases computes their products with it)."""
    if name not in _CASES:
        if name in ORACLE_SCENARIOS:
            import products_tm_cases as PC
            case = PC.scenario(oracle, name)
            rec = PC.all_products(oracle, name)[1]
            out = np.zeros(len(rec), PRODUCT)
            for f in PRODUCT.names:
                out[f] = rec[f]
            _CASES[name] = dict(seqs=list(case["seqs"]), splits=list(case.get("splits", ())), records=out, regions=REGIONS, case=case)
        elif name.startswith("classes_"):
            _CASES[name] = classes_case(name[len("classes_"):])
        else:
            _CASES[name] = {"alignment": alignment_case, "strands": strands_case, "packing": packing_case, "many": many_case}[name]()
        _CASES[name]["records"].setflags(write=False)
    return _CASES[name]


@functools.lru_cache(None)
def expected(oracle, name, region, canonical):
    """The model of a scenario, computed once and shared (leave it unchanged)."""
    return model(scenario(oracle, name), region, bool(canonical))


def check_against_oracle(oracle, name, result):
    """`result` (info and the classes' spellings for REGION_INNER, canonical = 0, of the scenario's records; the model's or the
    device's) against PCR::collect_unique_amplicons as the oracle restates it, which always spells the plus strand
    (pcr_assay.cpp:501-517).  For every pool pair i, the distinct INNER spellings of the records whose (plus, minus) is pair i in
    either orientation == the unique amplicons the oracle cuts for the pair.  The oracle reads a select_words DB, which keeps the
    best site per (oligo, sequence); on a scenario whose records come from an all-sites DB the records are first narrowed to the
    oracle's own bounds (sequence, begin, end), every one of which must be a record."""
    import products_tm_cases as PC
    import site_tm_cases as SC
    sc = scenario(oracle, name)
    case = sc["case"]
    ids = PC.all_products(oracle, name)[0]
    rec, info = sc["records"], result["info"]
    so = oracle.session()
    active = case.get("active")
    for i, s in enumerate(case["seqs"]):
        so.add_target(s, 1.0, True if active is None else bool(active[i]))
    for s, p in case.get("splits", ()):
        so.split(s, p)
    so.select(case["panel"], SC.SQ(case["thr"]))
    lo, hi = PC.amp_of(case)
    seen = 0
    for i, pair in enumerate(case["panel"]):
        f, r = ids[2 * i], ids[2 * i + 1]
        mine = np.nonzero(((rec["plus_oligo"] == f) & (rec["minus_oligo"] == r)) | ((rec["plus_oligo"] == r) & (rec["minus_oligo"] == f)))[0]
        bounds, unique = so.collect_amplicons(pair, case["thr"], lo, hi)
        at = {(int(s), int(b) & 0xFFFFFFFF, int(e)) for s, b, e in bounds}
        have = {(int(rec[k]["sequence"]), int(rec[k]["begin"]) & 0xFFFFFFFF, int(rec[k]["end"])) for k in mine}
        assert at <= have, (name, i, "a bound of the oracle is no record")
        if case["select"] != "all":
            assert at == have, (name, i)
        got = {tuple(int(v) for v in result["spellings"][info["amplicon"][k]]) for k in mine
               if (int(rec[k]["sequence"]), int(rec[k]["begin"]) & 0xFFFFFFFF, int(rec[k]["end"])) in at}
        assert got == {tuple(int(v) for v in u) for u in unique}, (name, i)
        seen += len(got)
    assert seen > 0, name
