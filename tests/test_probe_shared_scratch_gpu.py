"""The probers on the resident tree and the probers over the kept samples are one kernel family working in ONE scratch (ProbeScratch,
emat_probe_host.hpp).  What one call leaves there -- buffers grown for more cells, labels of another tree in `val`, descriptors of other
units -- must not reach the next: every call of a mixed sequence on one handle gives the bytes the same call gives as the first call of a
fresh handle.  And the resident calls need no store at all.

Bound: identical bytes (the same kernels on the same inputs; nothing is summed in an order that depends on the scratch)."""
import dataclasses

import numpy as np
import pytest

import delphy_amd as d
import samples_probe_model as SP
import samples_site_states_model as SS
from delphy_amd.scenarios import make_scenario

pytestmark = pytest.mark.gpu

TIPS, SAMPLES = 33, 5


def _with_mutations(tree, ref):
    """The tree with one mutation half way along the branch of every third node, each at a site of its own (so every `from` is the
    reference's state).  (The scenario's own mutation rate leaves a tree this small without any.)"""
    nodes = [v for v in range(tree.num_nodes) if v != tree.root][::3][:len(ref) - 1]
    count = np.zeros(tree.num_nodes, np.int64); count[nodes] = 1
    site = np.arange(len(nodes))
    frm = np.asarray(ref)[site]
    return dataclasses.replace(tree, mut_offset=np.concatenate([[0], np.cumsum(count)]).astype(tree.mut_offset.dtype), mut_site=site.astype(tree.mut_site.dtype),
                               mut_from=frm.astype(tree.mut_from.dtype), mut_to=((frm + 1) % 4).astype(tree.mut_to.dtype),
                               mut_t=(0.5 * (tree.t[tree.parent[nodes]] + tree.t[nodes])).astype(tree.mut_t.dtype))


class _Setup:
    """The resident tree, the 5 samples with their mutations, and windows for both: made once, at the first test."""

    def __init__(self):
        self.sc = sc = make_scenario("C1", num_tips=TIPS, num_sites=SS.NUM_SITES)
        self.tree = _with_mutations(sc.tree, sc.ref)
        self.samples, special = SS.sample_set(41, TIPS, SAMPLES)
        roots = [float(s.t[s.root]) for s in self.samples]
        t_end = max(float(s.t.max()) for s in self.samples) + 0.25
        self.window = (0.5 * (min(roots) + max(roots)), t_end)             # starts after some roots: cells are prepended, sample by sample
        family = SP.pops_for(t_end, min(roots))
        self.pops = [family[k % 3] for k in range(SAMPLES)]                 # constant, exponential, Skygrid in turn
        self.marks = [int(self.samples[0].root), 3, -1, 3, 17]
        self.sites = [special["root"], special["never"], special["tip"]]
        t_root = float(sc.tree.t[sc.tree.root])
        self.site = 2                                                      # a site the resident tree mutates
        self.before = (t_root - 0.4, sc.t_max_tip + 0.25)
        self.after = (t_root + 0.37 * (sc.t_max_tip - t_root), sc.t_max_tip + 0.25)
        self.res_pops = SP.pops_for(sc.t_max_tip, t_root)


_setup = []


def _s():
    if not _setup: _setup.append(_Setup())
    return _setup[0]


def _backend(store, chunk=0):
    sc = _s().sc
    b = d.EmatBackend(sc.num_sites)
    b.set_ref_sequence(sc.ref); b.tree_upload(_s().tree)
    if store:
        b.tree_samples_reserve(SAMPLES); b.tree_samples_reserve_mutations(sum(int(s.mut_offset[s.n]) for s in _s().samples) + 64)
        for s in _s().samples: b.tree_sample_push_flat_mutations(*s.push_args())
        b.set_option("samples_probe_chunk", chunk)
    return b


def _bytes(r):
    if isinstance(r, np.ndarray): return r.tobytes()
    return b"".join(a.tobytes() for a in (r.p, r.mean, r.order_stats, r.cells_to_skip))


_CALLS = {
    "batched ancestors, 7 cells": lambda b: b.tree_samples_probe_ancestors(_s().pops, _s().marks, *_s().window, 7, ranks=[0, 2, 4]),
    "resident site states, 200 cells": lambda b: b.tree_probe_site_states(_s().res_pops[2], _s().site, *_s().before, 200),
    "resident ancestors": lambda b: b.tree_probe_ancestors(_s().res_pops[1], _s().marks, *_s().after, 31),
    "batched site states": lambda b: b.tree_samples_probe_site_states(_s().pops[0], _s().sites, *_s().window, 12, ranks=[0, 2, 4]),
}
_ORDER = ["batched ancestors, 7 cells", "resident site states, 200 cells", "batched ancestors, 7 cells", "resident ancestors", "batched site states"]
_fresh = {}


def _first_on_a_fresh_handle(name, chunk):
    """The bytes of call `name` as the first prober call of a handle; made once and shared."""
    if (name, chunk) not in _fresh:
        b = _backend(True, chunk)
        try:
            _fresh[(name, chunk)] = _bytes(_CALLS[name](b))
        finally:
            b.close()
    return _fresh[(name, chunk)]


@pytest.mark.parametrize("chunk", [0, 1])
def test_a_mixed_sequence_gives_what_each_call_gives_first_on_a_fresh_handle(chunk):
    b = _backend(True, chunk)
    try:
        for step, name in enumerate(_ORDER):
            got = _bytes(_CALLS[name](b))
            assert got == _first_on_a_fresh_handle(name, chunk), "step %d (%s), chunk %d" % (step + 1, name, chunk)
    finally:
        b.close()
    assert _first_on_a_fresh_handle(_ORDER[0], 0) == _first_on_a_fresh_handle(_ORDER[0], 1)      # and the chunk changes nothing


def test_the_resident_calls_need_no_store():
    S = _s()
    b = _backend(False)
    try:
        s = b.tree_probe_site_states(S.res_pops[2], S.site, *S.before, 200)
        a = b.tree_probe_ancestors(S.res_pops[1], S.marks, *S.after, 31)
        counts, skip, x0 = b.tree_branch_counts(*S.after, 31, marked_nodes=S.marks)
    finally:
        b.close()
    assert s.tobytes() == _first_on_a_fresh_handle("resident site states, 200 cells", 0)
    assert a.tobytes() == _first_on_a_fresh_handle("resident ancestors", 0)
    assert counts.shape == (len(S.marks) + 1, 31 + skip) and skip > 0 and x0 <= float(S.sc.tree.t[S.sc.tree.root])
    assert np.all(np.abs(a.sum(axis=0) - 1.0) <= 1e-12) and np.all(np.abs(s.sum(axis=0) - 1.0) <= 1e-12)
    assert counts.sum() > 0 and len(np.unique(s)) > 4                          # the windows do meet the tree
