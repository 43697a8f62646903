"""The APOBEC (mpox) model in the run driver, without a backend: the site partition emat_run_set_mpox draws is the reference's rule
(Run::set_mpox_hack_enabled, core/run.cpp:370-382) on the sequence at node 0, restated here in Python from emat_run_tree_get; on and off; the two
mutual exclusions with the substitution-model moves.  No GPU."""
import numpy as np
import pytest

import delphy_amd as d

A, C, G, T = 0, 1, 2, 3


def tip0_sequence(tree, ref):
    """view_of_sequence_at(tree, 0): the reference sequence with the mutations on the path from the root down to node 0 applied in order (missations
    are not looked at).  Returns (the sequence, the path's mutations as (site, from, to) in that order)."""
    path, v = [], 0
    while v != -1:
        path.append(v); v = int(tree.parent[v])
    seq, muts = np.array(ref, np.uint8), []
    for v in reversed(path):
        for k in range(int(tree.mut_offset[v]), int(tree.mut_offset[v + 1])):
            l = int(tree.mut_site[k])
            assert seq[l] == tree.mut_from[k]
            seq[l] = tree.mut_to[k]; muts.append((l, int(tree.mut_from[k]), int(tree.mut_to[k])))
    return seq, muts


def apobec_partition(seq):
    """run.cpp:370-382 to the letter."""
    L = len(seq)
    out = np.zeros(L, np.int32)
    for l in range(L):
        apobec_context = ((l != 0) and (seq[l - 1] == T) and ((seq[l] == C) or (seq[l] == T))) or \
                         ((l + 1 != L) and (seq[l + 1] == A) and ((seq[l] == G) or (seq[l] == A)))
        out[l] = 1 if apobec_context else 0
    return out


def _run(tree, ref, mu=1e-3, seed=1):
    run = d.EmatRun(None, tree, ref, seed)
    run.set_hky(mu, 2.0, [0.1, 0.2, 0.3, 0.4])
    return run


SEED_2, SEED_60 = 1, 1      # (chosen so that the path to node 0 carries mutations into and out of a context: asserted below)


def _synthetic(num_tips, seed):
    par = d.SynthParams(num_tips=num_tips, num_sites=600, tip_span=365.0, pop_n0=365.0, pop_growth=0.0, mu=0.15 / 365.0, gaps_per_tip=2, mean_gap_len=12.0, seed=seed)
    tree, ref, _ = d.make_synthetic_emat(par)
    return tree, ref


@pytest.mark.parametrize("num_tips,seed", [(2, SEED_2), (60, SEED_60)])
def test_the_partition_is_the_references_rule_on_the_sequence_at_node_0(num_tips, seed):
    tree, ref = _synthetic(num_tips, seed)
    assert tree.num_nodes == 2 * num_tips - 1 and tree.child0[0] == -1
    run = _run(tree, ref)
    try:
        run.set_mpox(True, d.MpoxSpec())
        got, count = run.mpox_partition()
        t, r = run.tree()                                               # the tree as the driver holds it
        seq, muts = tip0_sequence(t, r)
        want = apobec_partition(seq)
        assert np.array_equal(got, want) and count == int(want.sum()) and 0 < count < len(seq)
        # the path's mutations matter: at least one carries a site into a context and one out of one, against the reference sequence's own partition
        of_ref = apobec_partition(r)
        assert len(muts) >= 2 and np.any((of_ref == 0) & (want == 1)) and np.any((of_ref == 1) & (want == 0))
        assert np.any(t.miss_offset[1] > t.miss_offset[0])              # node 0 has missations: they are not looked at
    finally:
        run.close()


def _two_tips(ref, muts_of_node=None, miss_of_node=None):
    """Tips 0 and 1 under the root 2; `muts_of_node` {node: [(site, from, to)]}, `miss_of_node` {node: [(start, end)]}."""
    muts_of_node, miss_of_node = muts_of_node or {}, miss_of_node or {}
    nm = sum(len(v) for v in muts_of_node.values()); ni = sum(len(v) for v in miss_of_node.values())
    t = d.FlatTree.empty(3, nm, ni, 0)
    t.root = 2
    t.parent[:] = [2, 2, -1]; t.child0[:] = [-1, -1, 0]; t.child1[:] = [-1, -1, 1]
    t.t[:] = [10.0, 12.0, 0.0]; t.t_min[:] = [10.0, 12.0, -1e30]; t.t_max[:] = [10.0, 12.0, 1e30]
    km = ki = 0
    for v in range(3):
        for j, (l, a, b) in enumerate(muts_of_node.get(v, [])):
            t.mut_site[km], t.mut_from[km], t.mut_to[km], t.mut_t[km] = l, a, b, (t.t[v] * (j + 1) / (len(muts_of_node[v]) + 1) if v != 2 else -1.0); km += 1
        for s, e in miss_of_node.get(v, []):
            t.miss_start[ki], t.miss_end[ki] = s, e; ki += 1
        t.mut_offset[v + 1] = km; t.miss_offset[v + 1] = ki
    return t, np.array(ref, np.uint8)


def _partition_of(ref, **kw):
    tree, ref = _two_tips(ref, **kw)
    run = _run(tree, ref)
    try:
        run.set_mpox(True, d.MpoxSpec())
        got, count = run.mpox_partition()
        assert count == int(got.sum())
        return got.tolist()
    finally:
        run.close()


@pytest.mark.parametrize("seq,want", [
    ([C], [0]), ([T], [0]), ([A], [0]),                       # L = 1: no neighbour on either side
    ([C, A], [0, 0]), ([G, A], [1, 0]), ([A, A], [1, 0]),     # a context at l = 0 comes from the right neighbour alone
    ([T, C], [0, 1]), ([T, T], [0, 1]), ([T, G], [0, 0]),     # ... and at l = L - 1 from the left one alone
    ([T, C, A], [0, 1, 0]),                                   # TCA: the C follows a T and precedes an A; one site, counted once (the second rule asks for G or A)
    ([T, G, A], [0, 1, 0]), ([T, T, A], [0, 1, 0]),           # the second rule alone; the first alone with A to the right
    ([T, A, A], [0, 1, 0]), ([T, T, T], [0, 1, 1]), ([A, A, A], [1, 1, 0]),          # already mutated: TT and AA
    ([G, T, C, A, A, C, T, T, G, A], [0, 0, 1, 1, 0, 0, 0, 1, 1, 0]),
])
def test_the_edges_on_hand_made_sequences(seq, want):
    assert apobec_partition(np.array(seq)).tolist() == want    # (the restatement itself, on cases worked out by hand)
    assert _partition_of(seq) == want


def test_the_paths_mutations_are_applied_in_order_and_missations_are_ignored():
    ref = [T, G, G, C, A, C]
    # the root turns site 3 C -> T, the branch to node 0 turns it on T -> A and site 1 G -> C; node 1's own mutation is not on the path
    muts = {2: [(3, C, T)], 0: [(3, T, A), (1, G, C)], 1: [(5, C, A)]}
    miss = {0: [(2, 4)], 2: [(5, 6)]}
    seq = [T, C, G, A, A, C]
    assert _partition_of(ref, muts_of_node=muts, miss_of_node=miss) == apobec_partition(np.array(seq)).tolist() == [0, 1, 1, 1, 0, 0]
    assert apobec_partition(np.array(ref)).tolist() == [0, 0, 0, 0, 0, 0]


def test_node_0_must_be_a_tip():
    t = d.FlatTree.empty(3, 0, 0, 0)
    t.root = 0
    t.parent[:] = [-1, 0, 0]; t.child0[:] = [1, -1, -1]; t.child1[:] = [2, -1, -1]
    t.t[:] = [0.0, 10.0, 12.0]; t.t_min[:] = [-1e30, 10.0, 12.0]; t.t_max[:] = [1e30, 10.0, 12.0]
    run = _run(t, np.array([T, C, A], np.uint8))
    try:
        with pytest.raises(d.EmatError, match="STATE.*emat_run_set_mpox.*node 0 of the tree is not a tip"):
            run.set_mpox(True, d.MpoxSpec())
        with pytest.raises(d.EmatError, match="STATE.*APOBEC model is off"):
            run.mpox()
    finally:
        run.close()


def test_on_and_off_restores_the_one_partition_model_and_mu():
    tree, ref = _synthetic(2, SEED_2)
    run = _run(tree, ref, mu=7e-4)
    try:
        for call in (run.mpox, run.mpox_partition):
            with pytest.raises(d.EmatError, match="STATE.*APOBEC model is off"):
                call()
        run.set_mpox(False)                                             # off while off: nothing happens
        assert run.hky()[0] == 7e-4
        run.set_mpox(True, d.MpoxSpec(mu=123.0, mu_star=3e-4, rounds=4))   # the spec's mu is ignored: the run's own is used
        assert run.mpox() == (7e-4, 3e-4)
        first = run.mpox_partition()
        run.set_mpox(True, d.MpoxSpec(mu_star=9.0, do_mu=False, rounds=2))  # on while on: the switches alone
        assert run.mpox() == (7e-4, 3e-4) and np.array_equal(run.mpox_partition()[0], first[0])
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            run.mpox_moves()                                            # no backend attached: the driver never runs moves itself
        run.set_mpox(False)
        assert run.hky() [0] == 7e-4 and run.hky()[1] == 2.0
        for call in (run.mpox, run.mpox_partition):
            with pytest.raises(d.EmatError, match="STATE.*APOBEC model is off"):
                call()
        run.set_hky(5e-4, 2.0, [0.1, 0.2, 0.3, 0.4])
        run.set_mpox(True, d.MpoxSpec())                                # on again: mu from the HKY model as it is now, mu* from the spec
        assert run.mpox() == (5e-4, 0.0) and np.array_equal(run.mpox_partition()[0], first[0])
    finally:
        run.close()


def test_the_setter_checks_its_arguments():
    tree, ref = _synthetic(2, SEED_2)
    run = d.EmatRun(None, tree, ref, 1)
    lib = d.load_library()
    try:
        with pytest.raises(d.EmatError, match="STATE.*emat_run_set_mpox.*emat_run_set_hky must be called first"):
            run.set_mpox(True, d.MpoxSpec())
        run.set_hky(0.0, 2.0, [0.1, 0.2, 0.3, 0.4])
        with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_run_set_mpox.*the run's mu must be finite and positive"):
            run.set_mpox(True, d.MpoxSpec())
        run.set_hky(1e-3, 2.0, [0.1, 0.2, 0.3, 0.4])
        for bad in (dict(mu_star=-1.0), dict(mu_star=float("nan")), dict(mu_prior_alpha=float("nan")), dict(mu_prior_beta=float("inf")), dict(rounds=-2), dict(rounds=4097)):
            with pytest.raises(d.EmatError, match="INVALID_ARGUMENT.*emat_run_set_mpox"):
                run.set_mpox(True, d.MpoxSpec(**bad))
        assert lib.emat_run_set_mpox(run._h, 1, None) == 1 and lib.emat_run_set_mpox(None, 1, None) == 1 and lib.emat_run_set_mpox(run._h, 0, None) == 0
        assert lib.emat_run_mpox_moves(None, None) == 1 and lib.emat_run_get_mpox(None, None, None) == 1 and lib.emat_run_get_mpox_partition(None, None, None) == 1
        with pytest.raises(d.EmatError, match="STATE.*APOBEC model is off"):
            run.mpox()                                                  # nothing of the refused calls took
    finally:
        run.close()


def test_the_two_mutual_exclusions_with_the_substitution_model_moves():
    tree, ref = _synthetic(2, SEED_2)
    run = _run(tree, ref)
    try:
        run.set_subst_moves(True, d.SubstSpec(rounds=2))
        with pytest.raises(d.EmatError, match="STATE.*emat_run_set_mpox.*substitution-model moves are on"):
            run.set_mpox(True, d.MpoxSpec())
        with pytest.raises(d.EmatError, match="STATE.*APOBEC model is off"):
            run.mpox()
        run.set_subst_moves(False, d.SubstSpec(rounds=2))
        run.set_mpox(True, d.MpoxSpec())
        with pytest.raises(d.EmatError, match="STATE.*APOBEC model is on"):
            run.set_subst_moves(True, d.SubstSpec(rounds=2))
        with pytest.raises(d.EmatError, match="STATE.*APOBEC model is on"):
            run.subst_moves()                                           # (asked before the backend is)
        run.set_subst_moves(False, d.SubstSpec(rounds=2))               # turning them off is no offence
        run.set_mpox(False)
        run.set_subst_moves(True, d.SubstSpec(rounds=2))                # ... and with the model off they come on as ever
        with pytest.raises(d.EmatError, match="NO_DEVICE"):
            run.subst_moves()
    finally:
        run.close()
