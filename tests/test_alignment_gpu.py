"""The alignment store on the device (emat_align_*: delphy_amd/csrc/emat_align_kernels.hpp) against the NumPy restatement
(alignment_model.py), integer for integer, at the smallest shapes where the kernels can go wrong: L around the wave's 64 sites, the
16 sites of a lane's load and the 1 024 sites of a pass, odd L (the half-filled last byte of a packed row), row counts around the 64 rows
of a tile; every chunking of the same matrix; placed deltas, runs, ties, invalid and undated rows; a given reference; the refusals."""
import numpy as np
import pytest

import alignment_model as am
import delphy_amd as d

pytestmark = pytest.mark.gpu

SITES = (1, 2, 63, 64, 65, 127, 128, 129, 1025)
ROWS = (1, 2, 3, 65, 257)
RATES = (0.0, 0.05, 0.9)
FIELDS = ("delta_offset", "delta_site", "delta_to", "miss_offset", "miss_start", "miss_end", "ref_sequence", "counts", "row_status", "row_bad_site",
          "row_bad_byte", "row_precision_loss")
UNAMBIGUOUS = np.frombuffer(b"ACGTUacgtu", np.uint8)
AMBIGUOUS = np.frombuffer(b"RYSWKMBDHVNryswkmbdhvn-?.", np.uint8)


def arrays_of(al):
    t = al.tips
    return dict(delta_offset=t.delta_offset, delta_site=t.delta_site, delta_to=t.delta_to, miss_offset=t.miss_offset, miss_start=t.miss_start, miss_end=t.miss_end,
                ref_sequence=al.ref, counts=al.counts, row_status=al.row_status, row_bad_site=al.row_bad_site, row_bad_byte=al.row_bad_byte,
                row_precision_loss=al.row_precision_loss)


def assert_equal(al, want, what=""):
    got = arrays_of(al)
    for f in FIELDS:
        assert got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), "%s differs %s" % (f, what)
    st = want["row_status"]
    assert al.report == dict(num_rows=len(st), num_tips=int((st >= 0).sum()), num_invalid=int((st == -2).sum()), num_undated=int((st == -1).sum()),
                             num_deltas=len(want["delta_site"]), num_intervals=len(want["miss_start"]), num_precision_loss=int(want["row_precision_loss"].sum()))


def run(b, rows, ref=None, dated=None, pieces=None, pad=0):
    """One begin / push ... / finish: `pieces` are the row counts of the pushes (None: all at once), `pad` bytes follow every row."""
    rows = am.as_rows(rows)
    R, L = rows.shape
    b.align_begin(R)
    stored = np.full((R, L + pad), ord("!"), np.uint8)   # (what follows a row is no sequence letter: it must never be read)
    stored[:, :L] = rows
    at = 0
    for n in (pieces or [R]):
        b.align_push(stored[at:at + n])
        at += n
    assert at == R
    return b.align_finish(ref, dated)


def random_rows(rng, R, L, rate):
    rows = UNAMBIGUOUS[rng.integers(0, len(UNAMBIGUOUS), (R, L))]
    amb = rng.random((R, L)) < rate
    # runs as well as single sites: half of the ambiguous sites drag their right neighbour along
    amb[:, 1:] |= amb[:, :-1] & (rng.random((R, L - 1)) < 0.5)
    rows[amb] = AMBIGUOUS[rng.integers(0, len(AMBIGUOUS), int(amb.sum()))]
    return rows


@pytest.fixture(scope="module")
def backends():
    made = {}
    def get(L):
        if L not in made:
            made[L] = d.EmatBackend(L)
        return made[L]
    yield get
    for b in made.values():
        b.close()


@pytest.mark.parametrize("L", SITES)
def test_random_rows_in_every_chunking(backends, L):
    b = backends(L)
    rng = np.random.default_rng(20261021 + L)
    for R in ROWS:
        for rate in RATES:
            rows = random_rows(rng, R, L, rate)
            dated = rng.random(R) < 0.8 if R > 1 else None
            if R >= 3:
                rows[rng.integers(0, R), rng.integers(0, L)] = ord("x")   # one invalid row
            want = am.finish(rows, dated=dated)
            what = "(L %d, rows %d, rate %g)" % (L, R, rate)
            assert_equal(run(b, rows, dated=dated), want, what + " in one push")
            assert_equal(run(b, rows, dated=dated, pieces=[1] * R, pad=3), want, what + " one row a push")
            if R >= 3:
                cuts = [1, (R - 1) // 3, R - 1 - (R - 1) // 3]
                assert_equal(run(b, rows, dated=dated, pieces=[c for c in cuts if c], pad=61), want, what + " in uneven pieces")
                ref = rng.integers(0, 4, L).astype(np.uint8)
                assert_equal(run(b, rows, ref=ref, dated=dated), am.finish(rows, ref=ref, dated=dated), what + " against a given reference")


def test_every_letter_in_both_cases(backends):
    letters = am.LETTERS.encode()
    L = len(letters)
    rows = [letters, letters.swapcase(), b"A" * L]
    al = run(backends(L) if L in SITES else d.EmatBackend(L), rows, ref=np.zeros(L, np.uint8))
    assert_equal(al, am.finish(rows, ref=np.zeros(L, np.uint8)))
    assert al.report["num_invalid"] == 0 and al.row_precision_loss[0] == sum(c in b"RYSWKMBDHVryswkmbdhv" for c in letters)


PLACED_L = 200


def placed(**sites):
    row = bytearray(b"A" * PLACED_L)
    for spec, ch in sites.items():
        lo, _, hi = spec.strip("s").partition("_")
        for l in range(int(lo), int(hi or lo) + 1):
            row[l] = ord(ch)
    return bytes(row)


def test_placed_deltas_and_runs():
    L = PLACED_L
    rows = [placed(s0="C", s63="G", s64="T", s199="c"),                 # deltas at 0, 63, 64, L - 1
            placed(s60_70="N"),                                           # a run across the wave's 64th site
            placed(s0_5="-"), placed(s190_199="?"),                       # a run from site 0, a run to L - 1
            b"N" * L,                                                     # a whole row missing
            placed(s10_12="N", s14_20="."),                               # two runs separated by one site
            placed(s30="R", s31="N", s32="y"),                            # R next to N: one run, two losses of precision
            placed(s15="N", s16="G", s17="N"),                            # a delta between two runs
            placed(s15_16="N", s31_32="K", s47_48="N", s63_64="S")]       # runs across the lanes' 16-site edges
    b = d.EmatBackend(L)
    ref = np.zeros(L, np.uint8)
    al = run(b, rows, ref=ref)
    assert_equal(al, am.finish(rows, ref=ref))
    t = al.tips
    def deltas(k): return list(zip(t.delta_site[t.delta_offset[k]:t.delta_offset[k + 1]].tolist(), t.delta_to[t.delta_offset[k]:t.delta_offset[k + 1]].tolist()))
    def runs(k): return list(zip(t.miss_start[t.miss_offset[k]:t.miss_offset[k + 1]].tolist(), t.miss_end[t.miss_offset[k]:t.miss_offset[k + 1]].tolist()))
    assert deltas(0) == [(0, 1), (63, 2), (64, 3), (199, 1)] and runs(0) == []
    assert runs(1) == [(60, 71)] and runs(2) == [(0, 6)] and runs(3) == [(190, 200)] and runs(4) == [(0, 200)] and deltas(4) == []
    assert runs(5) == [(10, 13), (14, 21)] and runs(6) == [(30, 33)] and al.row_precision_loss.tolist() == [0, 0, 0, 0, 0, 0, 2, 0, 4]
    assert deltas(7) == [(16, 2)] and runs(7) == [(15, 16), (17, 18)]
    assert runs(8) == [(15, 17), (31, 33), (47, 49), (63, 65)]
    b.close()


def test_consensus_ties_and_a_column_ambiguous_in_every_row():
    pairs = [(a, c) for a in range(4) for c in range(a + 1, 4)]       # the six two-way ties
    columns = [["ACGT"[a], "ACGT"[a], "ACGT"[c], "ACGT"[c]] for a, c in pairs]
    columns += [[x, y, y, x] for x, y in ("TC", "GA", "TA")]            # ... the later state seen first
    columns += [list("TGCA"), list("NRY-"), list("NNGN"), list("TTTC"), list("AANN")]   # the four-way tie; never unambiguous; one vote; a majority
    rows = ["".join(col[r] for col in columns) for r in range(4)]
    L = len(columns)
    b = d.EmatBackend(L)
    al = run(b, rows)
    assert_equal(al, am.finish(rows))
    assert "".join("ACGT"[s] for s in al.ref) == "AAACCG" + "CAA" + "AAGTA"
    assert al.counts[9].tolist() == [1, 1, 1, 1] and al.counts[10].tolist() == [0, 0, 0, 0]
    b.close()


@pytest.mark.parametrize("bad", [b"X", b"7", b"\0", b"\x80", b"\xff", b" ", b"\n", b">"])
def test_a_row_that_is_no_sequence(bad):
    L = 130
    good = b"ACGT" * 32 + b"AC"
    rows = [good, good[:77] + bad + good[78:], good.replace(b"A", b"G"), good[:129] + bad, good[:5] + bad + good[6:100] + b"Z" + good[101:]]
    b = d.EmatBackend(L)
    al = run(b, rows)
    assert_equal(al, am.finish(rows))
    assert al.row_status.tolist() == [0, -2, 1, -2, -2] and al.row_bad_site.tolist() == [-1, 77, -1, 129, 5] and al.row_bad_byte.tolist() == [0, bad[0], 0, bad[0], bad[0]]
    assert al.counts.sum() == 2 * L                                      # absent from the counts
    b.close()


def test_an_undated_row_counts_towards_the_consensus_and_is_no_tip():
    rows = ["ACGTA", "CCGTA", "CCGTT", "ACNTA", "AGGTA"]
    dated = [1, 0, 0, 1, 1]
    b = d.EmatBackend(5)
    al = run(b, rows, dated=dated)
    assert_equal(al, am.finish(rows, dated=dated))
    assert al.row_status.tolist() == [0, -1, -1, 1, 2] and al.counts[0].tolist() == [3, 2, 0, 0] and al.counts[1].tolist() == [0, 4, 1, 0]
    assert "".join("ACGT"[s] for s in al.ref) == "ACGTA" and al.tips.delta_offset.tolist() == [0, 0, 0, 1] and al.tips.delta_site.tolist() == [1]
    assert_equal(run(b, rows, dated=[0] * 5), am.finish(rows, dated=[0] * 5), "no tips at all")
    b.close()


def test_a_second_finish_and_more_rows_after_a_finish():
    rows = ["ACGTA", "CCGTA", "CCNTT"]
    b = d.EmatBackend(5)
    b.align_begin(5)
    b.align_push(am.as_rows(rows[:2]))
    assert_equal(b.align_finish(), am.finish(rows[:2]))
    assert_equal(b.align_finish(ref=[3, 3, 3, 3, 3]), am.finish(rows[:2], ref=[3, 3, 3, 3, 3]))
    b.align_push(am.as_rows(rows[2:]))
    with pytest.raises(d.EmatError, match="STATE"):
        b._align_get(d.engine._AlignReportC())                          # nothing valid between a push and the next finish
    assert_equal(b.align_finish(), am.finish(rows))
    b.close()


def test_refusals_and_the_call_after_each():
    L = 1025                                                              # (2^31 - 1 rows of it are a terabyte: more than any device has)
    rows = random_rows(np.random.default_rng(5), 4, L, 0.1)
    want = am.finish(rows)
    b = d.EmatBackend(L)
    for call in (lambda: b.align_push(rows), lambda: b.align_finish(), lambda: b._align_get(d.engine._AlignReportC())):
        with pytest.raises(d.EmatError, match="STATE"):
            b_call = call()
    b.align_begin(0)                                                      # releasing what was never bound is no error
    with pytest.raises(d.EmatError, match="INVALID_ARGUMENT"):
        b.align_begin(-1)
    with pytest.raises(d.EmatError, match=r"CAPACITY.*MB.*free"):
        b.align_begin(2**31 - 1)
    with pytest.raises(d.EmatError, match="STATE"):                       # ... and left nothing bound
        b.align_push(rows)
    assert_equal(run(b, rows), want, "after the refused begins")
    b.align_begin(4)
    lib = d.load_library()
    p = rows.ctypes.data_as(d.engine.C.POINTER(d.engine.C.c_uint8))
    assert lib.emat_align_push_rows(b.handle, -1, p, L) == 1 and "num_rows" in b.last_error()
    assert lib.emat_align_push_rows(b.handle, 4, p, L - 1) == 1 and "row_stride" in b.last_error()
    assert lib.emat_align_push_rows(b.handle, 4, None, L) == 1
    assert lib.emat_align_push_rows(b.handle, 0, None, L) == 0
    b.align_push(rows[:3])
    with pytest.raises(d.EmatError, match=r"CAPACITY.*nothing is pushed"):
        b.align_push(rows[2:])
    b.align_push(rows[3:])
    with pytest.raises(d.EmatError, match=r"INVALID_ARGUMENT.*given_ref\[7\] = 4"):
        b.align_finish(ref=[0] * 7 + [4] + [0] * (L - 8))
    with pytest.raises(d.EmatError, match="STATE"):
        b._align_get(d.engine._AlignReportC())
    assert_equal(b.align_finish(), want, "after the refused push and finish")
    b.align_begin(0)
    with pytest.raises(d.EmatError, match="STATE"):
        b.align_finish()
    assert_equal(run(b, rows), want, "after a release")
    b.close()
