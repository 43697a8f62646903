"""tests/mcc_summary_model.py against numbers worked by hand: the three four-tip samples of test_mcc_model, the index rule at m = 1, 2, 3,
the HPD's tie rule and its two ends (the whole range, one value), and a mutation a sample carries twice on one branch.  The checks
`check_four_tip_node_times` and `check_four_tip_mutations` are what tests/test_mcc_summary_gpu.py holds the device to as well.  No GPU."""
import numpy as np

import mcc_model as M
import mcc_summary_model as S
from samples_site_states_model import MutSample
from test_mcc_model import four_tip_samples

HAND_QUANTILES = (0.0, 0.5, 1.0)
HAND_MASS = 0.5
HAND_SITES = 12


def check_four_tip_node_times(r):
    """((A,B),(C,D)) at cherries -1 / -2, root -5; the same at -3 / -1, -6; ((A,C),(B,D)) with root -4, which stands in for both cherries.
    `r`: q_* [3][7] for HAND_QUANTILES, hpd_* [2][7] for HAND_MASS, num_exact [7], times / is_exact [7][3]."""
    assert list(r.num_exact) == [3, 3, 3, 3, 2, 2, 3]
    for v in range(4):                                       # tips: 0 in every sample
        assert list(r.q_mrca[:, v]) == [0.0] * 3 and list(r.q_exact[:, v]) == [0.0] * 3 and list(r.hpd_mrca[:, v]) == [0.0, 0.0] and list(r.hpd_exact[:, v]) == [0.0, 0.0]
    # m = 3: indices 0, floor(0.5 * 2) = 1, 2;  m = 2: indices 0, floor(0.5 * 1) = 0, 1
    assert list(r.q_mrca[:, 4]) == [-4.0, -3.0, -1.0] and list(r.q_exact[:, 4]) == [-3.0, -3.0, -1.0]
    assert list(r.q_mrca[:, 5]) == [-4.0, -2.0, -1.0] and list(r.q_exact[:, 5]) == [-2.0, -2.0, -1.0]
    assert list(r.q_mrca[:, 6]) == [-6.0, -5.0, -4.0] and list(r.q_exact[:, 6]) == [-6.0, -5.0, -4.0]
    # mass 0.5: m = 3 -> w = ceil(1.5) = 2, m = 2 -> w = 1
    assert list(r.hpd_mrca[:, 4]) == [-4.0, -3.0] and list(r.hpd_exact[:, 4]) == [-3.0, -3.0]      # widths 1, 2
    assert list(r.hpd_mrca[:, 5]) == [-2.0, -1.0] and list(r.hpd_exact[:, 5]) == [-2.0, -2.0]      # widths 2, 1
    assert list(r.hpd_mrca[:, 6]) == [-6.0, -5.0] and list(r.hpd_exact[:, 6]) == [-6.0, -5.0]      # widths 1, 1: the first
    if r.times is not None:
        assert r.times.tolist() == [[0.0] * 3] * 4 + [[-1.0, -3.0, -4.0], [-2.0, -1.0, -4.0], [-5.0, -6.0, -4.0]]
        assert np.asarray(r.is_exact, bool).tolist() == [[True] * 3] * 4 + [[True, True, False]] * 2 + [[True] * 3]


def _with_mutations(s, lists):
    """lists: {node: [(site, from, to, t), ...]}."""
    off, flat = [0], []
    for v in range(s.n):
        flat += lists.get(v, []); off.append(len(flat))
    col = lambda i, dt: np.array([r[i] for r in flat], dt)
    ref = np.zeros(HAND_SITES, np.uint8); ref[7] = 2
    return MutSample(s, off, col(0, np.int32), col(1, np.uint8), col(2, np.uint8), col(3, np.float64), ref)


def four_tip_mut_samples():
    """The four-tip samples with mutations: the master (sample 0) carries site 3 twice on the branch of cherry 4, one mutation on tip 0,
    one on cherry 5 and one on its root's own list.  Sample 1 has the master's topology: it carries (5, 0 -> 1) twice on tip 0's branch
    (with the way back between them) and nothing on cherry 5, whose clade it has.  Sample 2 has other cherries: its root corresponds to the
    master's cherry 4, not exactly, and carries the master's (3, 0 -> 1)."""
    s0, s1, s2 = four_tip_samples()
    return [_with_mutations(s0, {0: [(5, 0, 1, -0.5)], 4: [(3, 0, 1, -2.0), (3, 1, 2, -1.5)], 5: [(1, 0, 2, -3.0)], 6: [(7, 2, 3, -5.5)]}),
            _with_mutations(s1, {0: [(5, 0, 1, -0.75), (5, 1, 0, -0.5), (5, 0, 1, -0.25)], 4: [(3, 0, 1, -4.0), (3, 1, 2, -3.5)], 6: [(7, 2, 3, -6.5)]}),
            _with_mutations(s2, {0: [(5, 0, 1, -0.3)], 6: [(3, 0, 1, -4.5), (7, 2, 3, -4.2)]})]


def check_four_tip_mutations(r):
    """Records in the master's node order: tip 0, cherry 4 (two), cherry 5, the root."""
    assert list(r.num_with) == [3, 2, 2, 1, 3]
    assert list(r.mean_t) == [(-0.5 + -0.75 + -0.3) / 3, (-2.0 + -4.0) / 2, (-1.5 + -3.5) / 2, -3.0, (-5.5 + -6.5 + -4.2) / 3]
    assert list(r.t_min) == [-0.75, -4.0, -3.5, -3.0, -6.5]
    assert list(r.t_max) == [-0.3, -2.0, -1.5, -3.0, -4.2]


def test_node_times_of_the_four_tip_samples_by_hand():
    ss = four_tip_samples()
    d = M.derive_sets(ss)
    assert d.master == 0
    r = S.node_times(ss, d.corr, d.exact, None, HAND_QUANTILES, HAND_MASS)
    check_four_tip_node_times(r)
    assert r.i_star_mrca[6] == 0 and r.i_star_mrca[5] == 1 and r.i_star_mrca[4] == 0
    picked = S.node_times(ss, d.corr, d.exact, [6, 4, 6], HAND_QUANTILES, HAND_MASS)         # out of order, with a repeat
    assert picked.q_mrca[:, 0].tolist() == picked.q_mrca[:, 2].tolist() == r.q_mrca[:, 6].tolist() and picked.q_exact[:, 1].tolist() == r.q_exact[:, 4].tolist()
    assert list(picked.num_exact) == [3, 2, 3]


def test_mutation_support_of_the_four_tip_samples_by_hand():
    ss = four_tip_mut_samples()
    d = M.derive_sets([s.topology() for s in ss])
    r = S.mutation_support(ss, d.corr, d.exact, d.master)
    assert r.records == [(0, 5, 0, 1), (4, 3, 0, 1), (4, 3, 1, 2), (5, 1, 0, 2), (6, 7, 2, 3)]
    check_four_tip_mutations(r)


def test_a_record_carried_twice_on_one_branch_takes_the_first_time():
    ss = four_tip_mut_samples()
    d = M.derive_sets([s.topology() for s in ss])
    r = S.mutation_support(ss, d.corr, d.exact, d.master)
    assert r.t_min[0] == -0.75 and r.num_with[0] == 3        # sample 1's -0.75, not its later -0.25; counted once
    swapped = [ss[1], ss[0], ss[2]]                          # the master (the first maximum) is now the one that carries it twice: two records of their own
    d = M.derive_sets([s.topology() for s in swapped])
    assert d.master == 0
    r = S.mutation_support(swapped, d.corr, d.exact, d.master)
    assert r.records[:3] == [(0, 5, 0, 1), (0, 5, 1, 0), (0, 5, 0, 1)]
    assert list(r.num_with[:3]) == [3, 1, 3] and list(r.t_min[:3]) == [-0.75, -0.5, -0.75] and r.mean_t[0] == r.mean_t[2] == (-0.75 + -0.5 + -0.3) / 3


def test_the_index_rule_at_one_two_and_three_values():
    assert [S.quantile_of([7.0], q) for q in (0.0, 0.3, 1.0)] == [7.0, 7.0, 7.0]
    assert [S.quantile_of([1.0, 2.0], q) for q in (0.0, 0.5, 0.999, 1.0)] == [1.0, 1.0, 1.0, 2.0]
    assert [S.quantile_of([1.0, 2.0, 3.0], q) for q in (0.0, 0.49, 0.5, 0.975, 1.0)] == [1.0, 1.0, 2.0, 2.0, 3.0]
    for m in (1, 2, 3, 10, 257):                             # NumPy computes the same index
        for q in (0.0, 0.025, 0.5, 0.975, 1.0):
            assert S.quantile_of(list(range(m)), q) == int(np.floor(q * np.float64(m - 1)))
    assert [S.hpd_window(m, 0.95) for m in (1, 2, 3, 20, 21)] == [1, 2, 3, 19, 20]


def test_the_hpd_ties_and_its_two_ends():
    assert S.hpd_of([1.0, 1.0, 1.0, 1.0], 0.5) == (1.0, 1.0, 0)                    # equal values: the first window
    assert S.hpd_of([0.0, 1.0, 2.0, 3.0, 4.0], 0.4) == (0.0, 1.0, 0)               # equal widths: the first window
    assert S.hpd_of([0.0, 2.0, 3.0, 4.0, 6.0], 0.6) == (2.0, 4.0, 1)
    assert S.hpd_of([0.0, 2.0, 2.5, 4.0, 4.5, 9.0], 0.5) == (2.0, 4.0, 1)          # widths 2.5, 2, 2, 5: the first of the two
    assert S.hpd_of([-3.0, 0.5, 9.0], 1.0) == (-3.0, 9.0, 0)                       # mass 1: (min, max)
    assert S.hpd_of([-3.0, 0.5, 9.0], 1e-9) == (-3.0, -3.0, 0)                     # w = 1: lo == hi == s[0]
    assert S.hpd_of([5.0], 0.95) == (5.0, 5.0, 0)
