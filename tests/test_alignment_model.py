"""Aligned-FASTA input without a device: the NumPy restatement (alignment_model.py) and the library's date parser against the reference's
own unit-test expectations (tests/golden/alignment_expectations.json), the FASTA framer on a host-only handle against the restatement, and
what the entry points refuse before they need a device."""
import ctypes as C
import datetime
import json
import os

import numpy as np
import pytest

import alignment_model as am
import delphy_amd as d
from delphy_amd.engine import _AlignReportC

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alignment_expectations.json")))
STATES = "ACGT"


def iso_days(s):
    y, m, dd = (int(x) for x in s.split("-"))
    return float((datetime.date(y, m, dd) - datetime.date(2020, 1, 1)).days)


def want_range(exp):
    return None if exp is None else (iso_days(exp[0]), iso_days(exp[1]))


# ---- the model against the reference's expectations ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", GOLDEN["consensus"], ids=lambda c: c["name"])
def test_model_consensus(case):
    got = am.finish(case["sequences"])["ref_sequence"]
    assert "".join(STATES[s] for s in got) == case["expected"]


@pytest.mark.parametrize("case", GOLDEN["delta_from_reference"], ids=lambda c: c["name"])
def test_model_delta_from_reference(case):
    ref = np.array([STATES.index(c) for c in case["ref"]], np.uint8)
    if "error" in case:
        with pytest.raises(Exception):
            am.tip_desc(am.CODE[am.as_rows([case["seq"]])[0]], ref)
        return
    (sites, to), (starts, ends), _ = am.tip_desc(am.CODE[am.as_rows([case["seq"]], 0)[0]], ref)
    assert [[int(s), STATES[ref[s]], STATES[t]] for s, t in zip(sites, to)] == case["deltas"]
    assert [l for a, b in zip(starts, ends) for l in range(a, b)] == case["missing_sites"]


def test_the_epoch_is_day_zero():
    assert am.days(2020, 1, 1) == 0.0 and am.days(2020, 3, 1) == 60.0 and am.days(2019, 12, 31) == -1.0


@pytest.mark.parametrize("case", GOLDEN["id_date_range"], ids=lambda c: c["id"])
def test_id_date_range(case):
    want = want_range(case["expected"])
    assert am.date_range(case["id"]) == want
    assert d.seq_id_date_range(case["id"]) == want


@pytest.mark.parametrize("case", GOLDEN["parse_iso_month"] + GOLDEN["parse_iso_year"], ids=lambda c: c.get("month") or c["year"])
def test_months_and_years(case):
    s = case.get("month") or case["year"]
    for sep in "|-":
        assert am.date_range("x" + sep + s) == want_range(case["expected"])
        assert d.seq_id_date_range("x" + sep + s) == want_range(case["expected"])


def test_dates_of_every_form_and_the_strings_that_are_none():
    ids = ["hCoV-19/England/PLYM-3258B175/2022|EPI_ISL_15330011|2022-10-01", "hRSV-A-England-160340212-2016-EPI_ISL_11428309-2016-01-19",
           "a|2024-02-29", "a|2023-02-29", "a|2024-13-01", "a|2024-00-10", "a|2024-04-31", "a|2024-13", "a|2024-00", "a|0001", "a|1999-12",
           "a|2024-01-01/2024-02-30", "a|2024-03-05/2024-01-01", "2024-12-10", "|2024-12-10", "a 2024-12-10", "a|2024-12-1", "a|2024-1-10",
           "a|2024-12-10 ", "", "|", "-2024", "a|20240", "a/2024", "x|2024-12-10|2024", "x-2024-12-10/2024-12-11", "x|1600-02-29", "x|9998"]
    for i in ids:
        assert d.seq_id_date_range(i) == am.date_range(i), i
    assert d.seq_id_date_range("a|2024-02-29") == (am.days(2024, 2, 29),) * 2 and d.seq_id_date_range("a|2023-02-29") is None
    assert d.seq_id_date_range("|2024-12-10") == (am.days(2024, 12, 10),) * 2 and d.seq_id_date_range("2024-12-10") is None


# ---- the framer on a host-only handle --------------------------------------------------------------------------------------------

def framed(text, L):
    b = d.EmatBackend(L, device=-1)
    try:
        names, lengths, t_min, t_max, dated = b.fasta_frame(text)
        return names, lengths.tolist(), t_min, t_max, dated.tolist()
    finally:
        b.close()


FRAMER_CASES = {
    "plain": b">a|2024-01-05\nACGT\nACGT\n>b\nAAAA\nCCCC\n",
    "crlf": b">a|2024-01-05\r\nACGT\r\nACGT\r\n>b\r\nAAAACCCC\r\n",
    "no_final_newline": b">a\nACGTACGT\n>b|2021\nAAAACCCC",
    "blank_and_comment_lines": b";a comment\n\n>a|2024-01\n\nACGT\n;ACGT is not read\nACGT\n\n\n>b\nAAAACCCC\n\n",
    "ids_with_spaces": b">  hCoV-19/some place/1 2 | x|2022-10-01  \t\nACGTACGT\n>\tb c\nACGTACGT\n",
    "white_space_inside_lines": b">a\nAC GT\tAC\x0bG\x0cT\n>b\n A C G T A C G T \n",
    "record_before_the_first_header": b"ACGT\nACGT\n>b|2020-02-02\nAAAACCCC\n",
    "empty_id": b">\nACGTACGT\n>   \nACGTACGT\n",
    "a_lone_carriage_return_starts_the_unnamed_record": b"\r\nACGTACGT\n>b\nAAAACCCC\n",
    "letters_the_store_will_judge": b">a\nACGTXX!1\n>b\nacgtunN-\n",
}


@pytest.mark.parametrize("name", sorted(FRAMER_CASES))
def test_framer_equals_the_model(name):
    text = FRAMER_CASES[name]
    want = am.frame(text)
    assert all(len(seq) == 8 for _, seq in want), "the case itself"
    names, lengths, t_min, t_max, dated = framed(text, 8)
    assert names == [n for n, _ in want] and lengths == [8] * len(want)
    for k, (n, _) in enumerate(want):
        r = am.date_range(n)
        assert dated[k] == (r is not None)
        if r is None:
            assert np.isnan(t_min[k]) and np.isnan(t_max[k])
        else:
            assert (t_min[k], t_max[k]) == (np.float32(r[0]), np.float32(r[1]))


def test_the_model_frames_what_the_cases_mean():
    assert am.frame(FRAMER_CASES["crlf"]) == [("a|2024-01-05", b"ACGTACGT"), ("b", b"AAAACCCC")]
    assert am.frame(FRAMER_CASES["blank_and_comment_lines"]) == [("a|2024-01", b"ACGTACGT"), ("b", b"AAAACCCC")]
    assert am.frame(FRAMER_CASES["ids_with_spaces"]) == [("hCoV-19/some place/1 2 | x|2022-10-01", b"ACGTACGT"), ("b c", b"ACGTACGT")]
    assert am.frame(FRAMER_CASES["record_before_the_first_header"]) == [("", b"ACGTACGT"), ("b|2020-02-02", b"AAAACCCC")]
    assert am.frame(b"") == [] and am.frame(b"\n\n;x\n") == []


def test_unequal_lengths_are_refused_with_both_ids_and_lengths():
    b = d.EmatBackend(8, device=-1)
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*'second one' has 7 sites, while 'first' has 8.*aligned"):
        b.fasta_frame(b">first\nACGTACGT\n>second one\nACGTACG\n")
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*'first' has 9 sites, while the handle has 8"):
        b.fasta_frame(b">first\nACGTACGTA\n")
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*'b' has 0 sites"):
        b.fasta_frame(b">a\nACGTACGT\n>b\n>c\nACGTACGT\n")
    names, *_ = b.fasta_frame(b">a\nACGTACGT\n")      # after a refusal the next call works
    assert names == ["a"]
    b.close()


@pytest.mark.parametrize("text", [b"", b"\n\n", b";only a comment\n"])
def test_an_empty_file_is_refused(text):
    b = d.EmatBackend(8, device=-1)
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*Input has no sequences!"):
        b.fasta_frame(text)
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*Input has no sequences!"):
        b.load_fasta(text)
    b.close()


def test_a_load_without_a_device_frames_the_text_and_stops_there(tmp_path):
    b = d.EmatBackend(8, device=-1)
    with pytest.raises(d.EmatError, match="STATE"):
        b.fasta_records()
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        b.load_fasta(FRAMER_CASES["crlf"])
    assert b.fasta_records()[0] == ["a|2024-01-05", "b"]
    p = tmp_path / "x.fasta"
    p.write_bytes(FRAMER_CASES["plain"])
    with pytest.raises(d.EmatError, match="NO_DEVICE"):
        b.load_fasta(str(p))
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*different lengths"):
        b.load_fasta(b">a\nACGT\n")
    with pytest.raises(d.EmatError, match="IO.*cannot open"):
        b.load_fasta(str(tmp_path / "missing.fasta"))
    b.close()


# ---- argument refusals -------------------------------------------------------------------------------------------------------------

def test_the_store_has_no_cpu_path():
    b = d.EmatBackend(8, device=-1)
    for call in (lambda: b.align_begin(4), lambda: b.align_begin(0), lambda: b.align_push(np.full((1, 8), 65, np.uint8)), lambda: b.align_finish()):
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            call()
    lib = d.load_library()
    rep = _AlignReportC()
    assert lib.emat_align_sizes(b.handle, C.byref(rep)) == 2 and lib.emat_align_num_sites(b.handle) == 8
    b.close()


def test_null_arguments():
    lib = d.load_library()
    b = d.EmatBackend(8, device=-1)
    lo, hi, ok = C.c_double(), C.c_double(), C.c_int32()
    assert lib.emat_seq_id_date_range(None, C.byref(lo), C.byref(hi), C.byref(ok)) == 1
    assert lib.emat_seq_id_date_range(b"x|2024", None, C.byref(hi), C.byref(ok)) == 1
    assert lib.emat_align_begin(None, 1) == 1 and lib.emat_align_push_rows(None, 0, None, 8) == 1 and lib.emat_align_finish(None, None, None, None) == 1
    assert lib.emat_align_sizes(b.handle, None) == 1 and lib.emat_align_get(b.handle, None) == 1
    assert lib.emat_fasta_frame_memory(b.handle, None, 5, None) == 1 and lib.emat_fasta_frame_memory(b.handle, None, -1, None) == 1
    assert lib.emat_fasta_load_memory(b.handle, None, 5, None, 0, None) == 1 and lib.emat_fasta_load(b.handle, None, None, 0, None) == 1
    text = np.frombuffer(b">a\nACGTACGT\n", np.uint8)
    assert lib.emat_fasta_load_memory(b.handle, text.ctypes.data_as(C.POINTER(C.c_uint8)), text.size, None, -1, None) == 1
    assert lib.emat_fasta_sizes(b.handle, None) == 1
    b.close()
