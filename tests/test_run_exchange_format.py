"""The exchange format of part subtrees between processes (emat_run_pack_local_parts / emat_run_unpack_parts), byte for byte -- CPU only.

The layout the source states: per part a header of eight int32 {id, nodes, muts, intervals, from-states, root, 0, 0}, then the
seventeen arrays of the flat tree in the order of `emat_flat_tree`, each padded to 8 bytes.  The packer below is written from
that statement and from run.part(i) alone.
"""
import numpy as np
import pytest

import delphy_amd as d
from delphy_amd.scenarios import make_scenario

# (field, numpy type, which count: n nodes, n+1 offsets, m mutations, i intervals, f from-states) in the order of emat_flat_tree
ARRAYS = [("parent", np.int32, "n"), ("child0", np.int32, "n"), ("child1", np.int32, "n"), ("t", np.float64, "n"), ("t_min", np.float32, "n"), ("t_max", np.float32, "n"),
          ("mut_offset", np.int32, "n1"), ("mut_site", np.int32, "m"), ("mut_from", np.uint8, "m"), ("mut_to", np.uint8, "m"), ("mut_t", np.float64, "m"),
          ("miss_offset", np.int32, "n1"), ("miss_start", np.int32, "i"), ("miss_end", np.int32, "i"),
          ("mfs_offset", np.int32, "n1"), ("mfs_site", np.int32, "f"), ("mfs_state", np.uint8, "f")]
SEED, NUM_PARTS = 11, 4


def _counts(t):
    n = t.num_nodes
    return {"n": n, "n1": n + 1, "m": int(t.mut_offset[n]), "i": int(t.miss_offset[n]), "f": int(t.mfs_offset[n])}


def _pack_one(p, t):
    """(bytes of part p, offsets within them at which each of the seventeen arrays starts)"""
    c = _counts(t)
    out = [np.array([p, c["n"], c["m"], c["i"], c["f"], t.root, 0, 0], np.int32).tobytes()]
    starts = []
    for name, dt, cnt in ARRAYS:
        a = np.ascontiguousarray(getattr(t, name)[: c[cnt]], dt)
        assert a.shape[0] == c[cnt], name
        raw = a.tobytes()
        starts.append(sum(len(x) for x in out))
        out.append(raw + b"\0" * (-len(raw) % 8))
    return b"".join(out), starts


def _driver(sc):
    run = d.EmatRun(None, sc.tree, sc.ref, SEED)
    run.set_num_parts(NUM_PARTS)
    run.repartition()
    return run


def _parts(run):
    return [run.part(i) for i in range(run.num_parts()[0])]


def _assert_same_parts(a, b):
    assert len(a) == len(b)
    for (ta, ia, sa), (tb, ib, sb) in zip(a, b):
        assert ia == ib and sa == sb and ta.root == tb.root
        ca = _counts(ta)
        assert ca == _counts(tb)
        for name, dt, cnt in ARRAYS:
            assert np.array_equal(getattr(ta, name)[: ca[cnt]], getattr(tb, name)[: ca[cnt]]), name


@pytest.fixture(scope="module")
def sc():
    return make_scenario("C1", num_tips=200, num_sites=500, uncertain_tips=0.2, seed=1)   # (a seed with which the LAST part carries mutations, missing intervals and from-states)


@pytest.fixture(scope="module")
def packed(sc):
    """The first driver's parts, its buffer, and where the last part and each of its arrays start in the buffer."""
    run = _driver(sc)
    parts = _parts(run)
    buf = run.pack_local_parts()
    run.close()
    pieces = [_pack_one(p, t) for p, (t, _, _) in enumerate(parts)]
    last_start = sum(len(b) for b, _ in pieces[:-1])
    return parts, buf, b"".join(b for b, _ in pieces), last_start, [last_start + s for s in pieces[-1][1]]


def test_scenario_has_all_three_list_kinds(packed):
    parts = packed[0]
    assert len(parts) == NUM_PARTS
    tot = {k: sum(_counts(t)[k] for t, _, _ in parts) for k in ("m", "i", "f")}
    assert tot["m"] > 0 and tot["i"] > 0 and tot["f"] > 0, tot
    last = _counts(parts[-1][0])   # (the part whose array boundaries are cut below: a cut before an empty array would cut nothing off)
    assert last["m"] > 0 and last["i"] > 0 and last["f"] > 0, last


def test_pack_equals_the_stated_layout_byte_for_byte(packed):
    _, buf, expected, _, _ = packed
    assert buf.tobytes() == expected


def test_unpack_in_a_second_driver_returns_equal_parts(sc, packed):
    parts, buf, _, _, _ = packed
    run = _driver(sc)   # same seed, same cycle: the same partition
    for p, (t, _, _) in enumerate(parts):   # (its own parts are overwritten so that what comes back is what the buffer held)
        blank = d.FlatTree(**{**t.__dict__, "t": t.t + 1.0})
        run.part_put(p, blank)
    assert not np.array_equal(run.part(0)[0].t, parts[0][0].t)
    run.unpack_parts(buf)
    _assert_same_parts(_parts(run), parts)
    run.close()


def test_a_buffer_cut_inside_the_header_is_refused(sc, packed):
    _, buf, _, last_start, _ = packed
    run = _driver(sc)
    for cut in (16, last_start + 16):
        with pytest.raises(d.EmatError):
            run.unpack_parts(buf[:cut])
    run.close()


@pytest.mark.parametrize("k", range(17))
def test_a_buffer_cut_at_an_array_boundary_of_the_last_part_is_refused(sc, packed, k):
    _, buf, _, _, starts = packed
    assert starts[0] == packed[3] + 32 and starts[k] < buf.shape[0]
    run = _driver(sc)
    with pytest.raises(d.EmatError):
        run.unpack_parts(buf[: starts[k]])   # everything before array k of the last part, nothing of it
    run.close()
