"""pcr_pool_amplicons without a device: the symbol, the record layout and the Python names, the refusals that come before the
handle in their order, the model of tests/amplicon_seq_cases.py held to the oracle's collect_amplicons (itself held to the
compiled reference by test_oracle_vs_reference.py::test_collect_unique_amplicons), and the properties of the scenarios that
tests/test_gpu_pool_amplicons.py relies on."""
import numpy as np
import pytest

import amplicon_seq_cases as AC
from pcramp_amd import api, words as W

PCR_ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    return api.load_library()


def test_symbol_is_exported(lib):
    assert "pcr_pool_amplicons" in api.ABI_SYMBOLS
    assert hasattr(lib, "pcr_pool_amplicons"), "libpcramp_hip.so does not export pcr_pool_amplicons"
    assert api.AMPLICON_INFO_DTYPE.itemsize == 32 and api.AMPLICON_INFO_DTYPE == AC.INFO
    assert api.AMPLICON_INFO_DTYPE.names == AC.INFO_FIELDS
    assert (api.REGION_PRODUCT, api.REGION_INSERT, api.REGION_INNER) == AC.REGIONS == (0, 1, 2)
    assert api.AMPLICON_REVERSED == AC.REVERSED == 1
    assert callable(api.Screener.product_amplicons)
    assert AC.PRODUCT == api.PRODUCT_DTYPE


def _call(lib, which, n=1, products=True, region=0, class_cap=0, class_off=True, class_len=True, packed_cap=0, packed=False):
    rec = np.zeros(max(min(n, 4), 1), api.PRODUCT_DTYPE)                      # (n may lie: nothing is read before the handle)
    off, ln, pk = np.zeros(4, np.uint64), np.zeros(4, np.uint64), np.zeros(16, np.uint8)
    rc = lib.pcr_pool_amplicons(None, which, rec.ctypes.data if products else None, n, region, 0, None,
                                off.ctypes.data if class_off else None, ln.ctypes.data if class_len else None, class_cap,
                                pk.ctypes.data if packed else None, packed_cap, None)
    return rc, api._err(lib)


def test_refusals_before_the_handle(lib):
    """The set, the pointers, the region, the count, then the handle: each call below is wrong in one thing and in the
    handle, and the message names the one thing; two things wrong name the earlier."""
    rc, msg = _call(lib, api.TARGET)
    assert rc == PCR_ERR_ARG and "null handle" in msg                         # every argument is fine: only the handle is missing
    rc, msg = _call(lib, api.BACKGROUND, n=0, products=False)                 # n = 0 needs no records, but a handle
    assert rc == PCR_ERR_ARG and "null handle" in msg
    rc, msg = _call(lib, 7, products=False)
    assert rc == PCR_ERR_ARG and "unknown sequence set" in msg                # ... comes before the pointers
    rc, msg = _call(lib, api.MULTIPLEX, region=9)
    assert rc == PCR_ERR_ARG and "PCR_SET_MULTIPLEX" in msg                   # ... and before the region
    rc, msg = _call(lib, api.TARGET, products=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, class_cap=2, class_off=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, class_cap=2, class_len=False)
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, packed_cap=8)                            # packed_cap without a buffer
    assert rc == PCR_ERR_ARG and "bad argument" in msg
    rc, msg = _call(lib, api.TARGET, packed_cap=8, region=3)
    assert rc == PCR_ERR_ARG and "bad argument" in msg                        # ... comes before the region
    rc, msg = _call(lib, api.TARGET, class_cap=2, packed_cap=8, packed=True)  # all given: fine
    assert rc == PCR_ERR_ARG and "null handle" in msg
    for bad in (3, -1, 1 << 20):
        rc, msg = _call(lib, api.TARGET, region=bad)
        assert rc == PCR_ERR_ARG and "unknown region" in msg
    rc, msg = _call(lib, api.TARGET, region=3, n=1 << 31)
    assert rc == PCR_ERR_ARG and "unknown region" in msg                      # ... comes before the count
    for n in (1 << 31, 1 << 40):
        rc, msg = _call(lib, api.TARGET, n=n)
        assert rc == PCR_ERR_ARG and "2^31" in msg
    rc, msg = _call(lib, api.TARGET, n=(1 << 31) - 1)
    assert rc == PCR_ERR_ARG and "null handle" in msg
    for region in AC.REGIONS:
        rc, msg = _call(lib, api.TARGET, region=region)
        assert rc == PCR_ERR_ARG and "null handle" in msg


# ------------------------------------------------------------------ the model against the oracle (and so the reference)
@pytest.mark.parametrize("name", AC.ORACLE_SCENARIOS)
def test_model_inner_spellings_are_the_oracles_unique_amplicons(oracle, name):
    AC.check_against_oracle(oracle, name, AC.expected(oracle, name, AC.REGION_INNER, False))


# ------------------------------------------------------------------ what the GPU tests rely on
@pytest.mark.parametrize("name", sorted(AC.CLASS_COUNTS))
def test_scenarios_have_the_classes_they_were_built_for(name):
    sc = AC.scenario(None, name)
    (region,) = sc["regions"]
    for canonical in (0, 1):
        m = AC.expected(None, name, region, canonical)
        assert m["n_classes"] == AC.CLASS_COUNTS[name][canonical], (name, canonical)
        assert sorted(set(m["info"]["amplicon"].tolist())) == list(range(m["n_classes"]))
        assert m["info"]["first"].tolist() == [int(np.nonzero(m["info"]["amplicon"] == c)[0][0]) for c in m["info"]["amplicon"]]
        assert int(m["class_byte_offset"][-1] + (m["class_length"][-1] + 1) // 2) == m["packed_bytes"] == len(m["packed"])


def test_alignment_reaches_every_edge():
    sc = AC.scenario(None, "alignment")
    rec = sc["records"]
    assert {int(b) & 31 for b in rec["begin"]} >= {0, 1, 31} and {int(e) & 31 for e in rec["end"]} >= {0, 30, 31}
    lengths = (rec["end"] - rec["begin"] + 1).tolist()
    assert set(lengths) >= set(AC.ALIGN_LENGTHS) and max(lengths) > 64 * 32 * 2   # a lane takes a second and a third block
    last = len(sc["seqs"]) - 1
    assert AC.ALIGN_TAIL_LEN % 32 and any(r["sequence"] == 1 and r["end"] == AC.ALIGN_TAIL_LEN - 1 for r in rec)
    assert any(r["sequence"] == last for r in rec)
    m = AC.expected(None, "alignment", AC.REGION_PRODUCT, 0)
    assert m["info"]["other"].any() and (m["info"]["gc"] > 0).any()


def test_strands_scenario():
    sc = AC.scenario(None, "strands")
    codes = AC.codes_of(sc)
    rec = sc["records"]
    S = AC.STRANDS
    plain, canon = (AC.expected(None, "strands", AC.REGION_INSERT, c)["info"] for c in (0, 1))
    # one insert on both strands: two classes as read, one canonical, exactly one of the two reversed
    assert plain["amplicon"][S["fwd"]] != plain["amplicon"][S["rev"]] and canon["amplicon"][S["fwd"]] == canon["amplicon"][S["rev"]]
    assert sorted((int(canon["flags"][S["fwd"]]), int(canon["flags"][S["rev"]]))) == [0, 1]
    assert canon["amplicon"][S["whole"]] == canon["amplicon"][S["fwd"]] and canon["copies"][S["fwd"]] == 3 and canon["sequences"][S["fwd"]] == 3
    assert canon["amplicon"][S["iupac"]] == canon["amplicon"][S["iupac_rev"]] and plain["amplicon"][S["iupac"]] != plain["amplicon"][S["iupac_rev"]]
    start = lambda k: AC.region_of(rec[k], AC.REGION_INSERT)
    where = lambda k: AC.first_difference(codes[int(rec[k]["sequence"])], *start(k))
    assert where(S["palindrome"]) is None and canon["flags"][S["palindrome"]] == 0          # reverse-palindromic: not REVERSED
    # the tie-break at the last position: a single base, and the last position at which a first difference can stand
    assert start(S["single"])[1] == 1 and where(S["single"]) == 0
    for k, n in ((S["middle"], 70), (S["middle_long"], 4200)):
        assert start(k)[1] == n and where(k) == n // 2 - 1
    assert canon["flags"][S["middle"]] == 0 and canon["flags"][S["middle_long"]] == AC.REVERSED
    assert (4200 // 2 - 1) // 32 >= 64                                                       # decided in the wave's second pass
    iu = codes[6][31:71]
    assert {W._CODE[c] for c in "RYMKSWN"} <= set(iu.tolist())
    assert plain["other"][S["iupac"]] == int((~np.isin(iu, (1, 2, 4, 8))).sum()) > 20
    # the split: an EOS inside the insert, which leaves the class of its unsplit copy
    s, p = sc["splits"][0]
    b, n = start(S["split"])
    assert s == rec[S["split"]]["sequence"] and b <= p < b + n and codes[s][p] == 0
    assert plain["amplicon"][S["split"]] != plain["amplicon"][S["whole"]] == plain["amplicon"][S["fwd"]]
    assert plain["other"][S["split"]] == 1 and plain["other"][S["whole"]] == 0


def test_classes_scenarios():
    same = AC.expected(None, "classes_same", AC.REGION_INSERT, 0)["info"]
    assert (same["copies"] == 9).all() and (same["sequences"] == len(AC.CLASS_SHARED)).all() and not same["first"].any()
    sc = AC.scenario(None, "classes_mixed")
    assert {63, 64, 128} <= set(sc["records"]["sequence"].tolist())
    m = AC.expected(None, "classes_mixed", AC.REGION_INSERT, 0)
    info = m["info"]
    assert info["amplicon"][0] == info["amplicon"][1] and info["copies"][0] == 6 and info["sequences"][0] == 5   # sequence 5 twice
    assert info["amplicon"][2] != info["amplicon"][0] and info["length"][2] == info["length"][0]
    a, b = m["spellings"][info["amplicon"][0]], m["spellings"][info["amplicon"][2]]
    assert (a[:-1] == b[:-1]).all() and a[-1] != b[-1]                         # the last base only
    longer = m["spellings"][info["amplicon"][3]]
    assert len(longer) == len(a) + 1 and (longer[:-1] == a).all() and info["amplicon"][3] != info["amplicon"][4]
    empties = np.nonzero(info["length"] == 0)[0]
    assert len(empties) == 2 and len(set(info["amplicon"][empties].tolist())) == 1 and (info["copies"][empties] == 2).all()
    assert AC.expected(None, "classes_empty", AC.REGION_INSERT, 0)["packed_bytes"] == 0


def test_packing_and_many():
    m = AC.expected(None, "packing", AC.REGION_INNER, 0)
    odd = [int(n) & 1 for n in m["class_length"]]
    assert {(odd[i], odd[i + 1]) for i in range(len(odd) - 1)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert any(int(o) & 3 for o in m["class_byte_offset"]) and any(int(o) % 4 == 0 and int(n) >= 32 for o, n in zip(m["class_byte_offset"], m["class_length"]))
    many = AC.scenario(None, "many")
    assert len(many["records"]) == AC.MANY_RECORDS > 65536
    info = AC.expected(None, "many", AC.REGION_PRODUCT, 0)["info"]
    assert info["copies"].min() > 100 and int(info["first"].max()) < 65536      # every class has members on both sides of 65 536
    assert all(int(info["amplicon"][k]) in set(info["amplicon"][65536:].tolist()) for k in range(0, 65536, 997))


def test_panel_scenarios(oracle):
    assert len(AC.scenario(oracle, "random")["records"]) == 6647
    for name in AC.PANEL_SCENARIOS:
        sc = AC.scenario(oracle, name)
        assert sc["regions"] == AC.REGIONS and len(sc["records"])
        n = {r: AC.expected(oracle, name, r, 0)["n_classes"] for r in AC.REGIONS}
        assert 0 < n[AC.REGION_INSERT] <= n[AC.REGION_INNER] <= len(sc["records"])
