"""Aligned FASTA in, end to end: a 60-tip, 2 000-site scenario with uncertain tips is rendered as FASTA text from its tip descriptors
(the reference sequence with the deltas applied, N on the missing intervals, ids ending in |YYYY-MM-DD or a range), loaded, and must
come back as those descriptors -- deltas, intervals, dates -- and as the same initial tree; without a given reference the consensus is
the restatement's (alignment_model.py)."""
import datetime
import re

import numpy as np
import pytest

import alignment_model as am
import delphy_amd as d
from builder_cases import FIELDS
from delphy_amd.scenarios import make_scenario
from oracle_ffi import OracleBuild

pytestmark = pytest.mark.gpu


def iso(day):
    return (datetime.date(2020, 1, 1) + datetime.timedelta(days=int(day))).isoformat()


@pytest.fixture(scope="module")
def rendered():
    """(scenario, its descriptors with whole-day dates, names, rows, FASTA text)"""
    sc = make_scenario("C1", num_tips=60, num_sites=2000, uncertain_tips=0.2)
    ob = OracleBuild(sc.ref)
    try:
        tips = ob.tip_descs_of(sc.tree)
    finally:
        ob.close()
    exact = tips.t_max - tips.t_min < 1.0                                                                       # an id holds whole days
    tips.t_min = np.floor(tips.t_min).astype(np.float32); tips.t_max = np.where(exact, tips.t_min, np.ceil(tips.t_max)).astype(np.float32)
    assert (tips.t_min < tips.t_max).any() and (tips.t_min == tips.t_max).any() and tips.miss_offset[-1] > 0 and tips.delta_offset[-1] > 0
    names, rows = [], []
    for k in range(tips.num_tips):
        row = np.frombuffer(b"ACGT", np.uint8)[sc.ref].copy()
        lo, hi = tips.delta_offset[k], tips.delta_offset[k + 1]
        row[tips.delta_site[lo:hi]] = np.frombuffer(b"ACGT", np.uint8)[tips.delta_to[lo:hi]]
        for a, e in zip(tips.miss_start[tips.miss_offset[k]:tips.miss_offset[k + 1]], tips.miss_end[tips.miss_offset[k]:tips.miss_offset[k + 1]]):
            row[a:e] = ord("N")
        rows.append(row.tobytes())
        date = iso(tips.t_min[k]) if tips.t_min[k] == tips.t_max[k] else iso(tips.t_min[k]) + "/" + iso(tips.t_max[k])
        names.append("hCoV-19/some place/%d/2020|EPI_ISL_%d|%s" % (k, 400000 + k, date))
    return sc, tips, names, rows, am.render_fasta(names, rows, width=60)


def same_descriptors(got, want):
    for f in ("t_min", "t_max", "delta_offset", "delta_site", "delta_to", "miss_offset", "miss_start", "miss_end"):
        assert np.array_equal(getattr(got, f), getattr(want, f)), f


def test_the_loaded_descriptors_are_the_rendered_ones_and_build_the_same_tree(rendered, tmp_path):
    sc, tips, names, rows, text = rendered
    b = d.EmatBackend(sc.num_sites)
    try:
        got = b.load_fasta(text, ref=sc.ref)
        same_descriptors(got, tips)
        assert got.names == names and np.array_equal(got.ref, sc.ref)
        assert got.report["num_records"] == 60 and got.report["num_tips"] == 60 and got.report["num_precision_loss"] == 0
        b.set_ref_sequence(got.ref)
        t_loaded = b.build_usher_like(got, 7)
        t_orig = b.build_usher_like(tips, 7)
        assert t_loaded.root == t_orig.root
        for f in FIELDS:
            assert np.array_equal(getattr(t_loaded, f), getattr(t_orig, f)), f
        # the same from a file with DOS line ends, two rows a chunk (the last chunk is short: 60 = 29 x 2 + 2 ... and with 7, 60 = 8 x 7 + 4)
        p = tmp_path / "tips.fasta"
        p.write_bytes(am.render_fasta(names, rows, width=77, line_end="\r\n"))
        for chunk in (2, 7):
            same_descriptors(b.load_fasta(str(p), ref=sc.ref, chunk_rows=chunk), tips)
    finally:
        b.close()


def test_without_a_reference_the_consensus_is_the_models(rendered):
    sc, tips, names, rows, text = rendered
    # an undated and an invalid record among them: the first counts towards the consensus, the second does not; neither is a tip
    extra_names = names[:10] + ["no date here"] + names[10:20] + ["bad|2020-03-01"] + names[20:]
    extra_rows = rows[:10] + [rows[3].replace(b"A", b"G")] + rows[10:20] + [rows[4][:1234] + b"J" + rows[4][1235:]] + rows[20:]
    dated = [am.date_range(n) is not None for n in extra_names]
    assert dated.count(False) == 1
    want = am.finish(extra_rows, dated=dated)
    b = d.EmatBackend(sc.num_sites)
    try:
        got = b.load_fasta(am.render_fasta(extra_names, extra_rows), chunk_rows=16)
        assert np.array_equal(got.ref, want["ref_sequence"]) and np.array_equal(got.alignment.counts, want["counts"])
        for f in ("delta_offset", "delta_site", "delta_to", "miss_offset", "miss_start", "miss_end"):
            assert np.array_equal(getattr(got, f), want[f]), f
        for f in ("row_status", "row_bad_site", "row_bad_byte", "row_precision_loss"):
            assert np.array_equal(getattr(got.alignment, f), want[f]), f
        assert got.alignment.row_status[10] == -1 and got.alignment.row_status[21] == -2 and got.alignment.row_bad_site[21] == 1234 and got.alignment.row_bad_byte[21] == ord("J")
        assert got.names == names and got.num_tips == 60 and got.report["num_undated"] == 1 and got.report["num_invalid"] == 1
        want_dates = np.array([am.date_range(n) for n in names], np.float32)
        assert np.array_equal(got.t_min, want_dates[:, 0]) and np.array_equal(got.t_max, want_dates[:, 1])
        # a record of another length, in the middle of a chunk: refused, and the next load works
        with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*'short' has 1999 sites, while '%s' has 2000" % re.escape(names[0])):
            b.load_fasta(am.render_fasta(names[:5] + ["short"] + names[5:], rows[:5] + [rows[5][:-1]] + rows[5:]), chunk_rows=4)
        with pytest.raises(d.EmatError, match="STATE"):
            b._align_get(d.engine._AlignReportC())
        same_descriptors(b.load_fasta(text, ref=sc.ref), tips)
    finally:
        b.close()
