"""The site-state prober over many samples (emat_tree_samples_probe_site_states, emat_mcc_probe_site_states) restated: a loop of
prober_model.probe_site_states_on_tree per sample and site, mean and order statistics as numpy makes them; and a seeded generator of
sample sets that carry mutations, with the state-chain condition the reference asserts of a tree (every mutation's `from` is the state
above it, `to` differs from `from`).  Pure Python / numpy; needs no GPU.

Bound per (sample, site), test_probe_gpu.py's end-to-end one: the device adds the fractional terms of a cell in fixed point with the
quantum q of the store's node count, each rounded once, and converts once (u = 2^-53); the model adds doubles.  With B fractional terms
and A additions into a cell the two cell sums differ by at most B q / 2 + (A + 1) u |cell| (asserted with SAFETY = 2); eps is that over
the cell total, and Tree_prober's recurrence, a convex combination, adds the cells' errors up: 1e-12 + 3 eps cells."""
import random

import numpy as np

import mcc_model
import prober_model as M
import samples_probe_model as SP

NUM_SITES = 12           # of every generated set; site NUM_SITES - 1 is never mutated


class MutSample:
    """A sample that kept its mutations: the arrays of a mcc_model.Sample, CSR mutation lists per node, and the reference sequence
    its root starts from -- what prober_model asks a tree for."""

    def __init__(self, s, mut_offset, mut_site, mut_from, mut_to, mut_t, ref):
        self.parent, self.child0, self.child1, self.t, self.root = s.parent, s.child0, s.child1, np.asarray(s.t, np.float64), int(s.root)
        self.mut_offset, self.mut_site = np.asarray(mut_offset, np.int32), np.asarray(mut_site, np.int32)
        self.mut_from, self.mut_to, self.mut_t = np.asarray(mut_from, np.uint8), np.asarray(mut_to, np.uint8), np.asarray(mut_t, np.float64)
        self.ref = np.asarray(ref, np.uint8)
        self.num_nodes = self.n = int(self.parent.shape[0])

    def topology(self):
        return mcc_model.Sample(self.parent, self.child0, self.child1, self.t, self.root)

    def push_args(self):
        """The arguments of EmatBackend.tree_sample_push_flat_mutations."""
        return (self.parent, self.child0, self.child1, self.t, self.root, self.mut_offset, self.mut_site, self.mut_from, self.mut_to, self.mut_t, self.ref)


# ---- the batched model ---------------------------------------------------------------------------------------------------------
def model_one(s, pop, site, t_start, t_end, cells):
    """(p [4][cells], cells_to_skip, tolerance) of prober_model on one sample and site."""
    fam, skip, root_state = M.site_states_branch_counts(s, s.ref, site, t_start, t_end, cells)
    want, B, A = fam.array(), fam.touched(), fam.adds()
    bound = B * SP.quantum(s.num_nodes) / 2 + (A + 1) * SP.U * np.abs(want)
    tot = want.sum(axis=0)
    eps = float(np.max(SP.SAFETY * bound.sum(axis=0)[tot > 0] / tot[tot > 0])) if np.any(tot > 0) else 0.0
    p = M.tree_prober(fam, skip, M.OraclePop(pop), [float(k == root_state) for k in range(4)])
    return p, skip, SP.P_TOL + 3.0 * eps * fam.num_cells


def model_batched(samples, pops, sites, t_start, t_end, cells, ranks=()):
    """What the batched call returns for the chosen `samples`: p [M][sites][4][cells], mean (sample-order sum / M), order statistics
    (np.sort over the samples) [ranks][sites][4][cells], cells_to_skip [M], and the tolerance of every p[k][i] [M][sites]."""
    m = len(samples)
    p = np.zeros((m, len(sites), 4, cells)); tol = np.zeros((m, len(sites))); skip = np.zeros(m, np.int32)
    for k, s in enumerate(samples):
        for i, site in enumerate(sites):
            p[k, i], skip[k], tol[k, i] = model_one(s, pops[k] if len(pops) > 1 else pops[0], int(site), t_start, t_end, cells)
    total = np.zeros(p.shape[1:])
    for k in range(m): total = total + p[k]
    srt = np.sort(p, axis=0)
    stats = np.stack([srt[q] for q in ranks]) if len(ranks) else None
    return p, total / m, stats, skip, tol


# ---- the generator ---------------------------------------------------------------------------------------------------------------
def _preorder(s):
    out, stack = [], [int(s.root)]
    while stack:
        v = stack.pop(); out.append(v)
        if s.child0[v] >= 0: stack.append(int(s.child1[v])); stack.append(int(s.child0[v]))
    return out


def add_mutations(rng, s, ref, root_site, tip_site):
    """States simulated down the tree `s` (a mcc_model.Sample) for every site but the last: a branch mutates a site with a probability
    that leaves most branches alone, now and then twice, every mutation from the state above it.  The root's own list changes
    `root_site` (once or twice); the branch of one tip changes `tip_site`.  Lists are in time order."""
    n, L = s.n, len(ref)
    lists = [[] for _ in range(n)]                       # per node: (site, from, to, t)
    state = np.tile(np.asarray(ref, np.uint8), (n, 1))   # per node: the sequence at the node
    other = lambda a: rng.choice([x for x in range(4) if x != a])
    tips = [v for v in range(n) if s.child0[v] < 0 and v != s.root]
    lucky_tip = rng.choice(tips) if tips else -1
    for v in _preorder(s):
        if v == s.root:
            cur = state[v]
            for j in range(rng.choice((1, 2))):
                to = other(int(cur[root_site]))
                lists[v].append((root_site, int(cur[root_site]), to, float(s.t[v]) - 1.0 + 0.25 * j)); cur[root_site] = to
            continue
        p = int(s.parent[v])
        cur = state[v]; cur[:] = state[p]
        lo, hi = float(s.t[p]), float(s.t[v])
        rate = min(0.5, 3.0 / n + 0.05)
        for site in range(L - 1):
            hits = (v == lucky_tip and site == tip_site) + (rng.random() < rate) + (rng.random() < 0.1 * rate)
            for tm in sorted(rng.uniform(lo, hi) for _ in range(hits)):
                to = other(int(cur[site]))
                lists[v].append((site, int(cur[site]), to, tm)); cur[site] = to
        lists[v].sort(key=lambda r: r[3])
    off = np.zeros(n + 1, np.int32)
    flat = []
    for v in range(n):
        flat += lists[v]; off[v + 1] = len(flat)
    col = lambda i, dt: np.array([r[i] for r in flat], dt)
    return MutSample(s, off, col(0, np.int32), col(1, np.uint8), col(2, np.uint8), col(3, np.float64), ref)


def sample_set(seed, num_tips, num_samples):
    """(samples, special): samples_probe_model.sample_set's trees -- random binary trees over fixed tips -- each with mutations of its own
    on one reference sequence per sample; special = {"never", "root", "tip"}: a site no sample mutates, one every sample changes on
    its root's own list, one every sample mutates on a tip branch."""
    rng = random.Random(seed * 7919 + 13)
    special = {"never": NUM_SITES - 1, "root": rng.randrange(NUM_SITES - 1)}
    special["tip"] = rng.choice([x for x in range(NUM_SITES - 1) if x != special["root"]])
    out = []
    for s in SP.sample_set(seed, num_tips, num_samples):
        ref = [rng.randrange(4) for _ in range(NUM_SITES)]
        out.append(add_mutations(rng, s, ref, special["root"], special["tip"]))
    return out, special


def check_state_chain(s, times=True):
    """The condition the reference asserts of a tree's mutations (assert_phylo_tree_integrity, core/phylo_tree.cpp:113-200: CHECK_NE(m.from, m.to), CHECK_EQ(m.from, cur_seq[m.site])): walking down from
    the reference sequence, every mutation leaves the state it finds and arrives at another; sites and states are in range.
    `times`: a list is in time order and lies on its branch (the prober reads no mutation time, and the reference's own fixtures do not keep to it)."""
    state = np.tile(s.ref, (s.n, 1))
    for v in _preorder(s):
        cur = state[v]
        if v != s.root: cur[:] = state[int(s.parent[v])]
        last_t = -np.inf
        for j in range(int(s.mut_offset[v]), int(s.mut_offset[v + 1])):
            site, frm, to = int(s.mut_site[j]), int(s.mut_from[j]), int(s.mut_to[j])
            assert 0 <= site < len(s.ref) and 0 <= frm < 4 and 0 <= to < 4 and frm != to, (v, j)
            assert cur[site] == frm, "node %d, mutation %d: from %d and the state above is %d" % (v, j, frm, cur[site])
            assert not times or s.mut_t[j] >= last_t, (v, j)
            if times and v != s.root: assert s.t[int(s.parent[v])] <= s.mut_t[j] <= s.t[v], (v, j)
            cur[site] = to; last_t = float(s.mut_t[j])
    assert int(s.mut_offset[0]) == 0 and int(s.mut_offset[s.n]) <= len(s.mut_site)


# ---- the seeded cases of the GPU test ---------------------------------------------------------------------------------------------
# (tips, samples pushed, first, stride, cells, which sites, t_start between the roots).  Node counts 3 .. 513 on both sides of 256 (the
# kernels' block) and of 511 (where the fixed-point quantum changes); samples 1 .. 100 with samples x nodes small; cells 1 .. 1000.
# Sites: n = never mutated, r = changed on the root's list, t = mutated on a tip branch, a digit = that site; a repeat is a repeat.
REQUIRED = [(2, 3, 0, 1, 1, "r", True), (4, 2, 0, 1, 63, "nrt", True), (128, 3, 0, 1, 64, "nrt0r", True), (129, 2, 0, 1, 65, "t", True),
            (256, 3, 0, 1, 20, "rn", False), (257, 2, 0, 1, 20, "tt", True), (5, 1, 0, 1, 10, "n", False), (4, 65, 0, 1, 8, "r", True),
            (3, 100, 0, 1, 6, "t", True), (7, 2, 0, 1, 1000, "rt", True), (9, 9, 2, 3, 11, "nrt12", True), (12, 8, 1, 2, 9, "3", True),
            (2, 5, 4, 1, 3, "rr", False), (30, 7, 1, 1, 64, "trn45", True)]


def gpu_cases():
    rng = random.Random(78)
    cases = list(REQUIRED)
    while len(cases) < 40:
        pushed = rng.randint(1, 10)
        first = rng.randrange(pushed) if rng.random() < 0.5 else 0
        sites = "".join(rng.choice("nrt0123456789") for _ in range(rng.randint(1, 5)))
        cases.append((rng.randint(2, 40), pushed, first, rng.choice((1, 1, 2, 3)), rng.choice((1, 7, 33, 63, 64, 65)), sites, rng.random() < 0.7))
    return cases


def sites_of(spec, special):
    return [special[{"n": "never", "r": "root", "t": "tip"}[c]] if c in "nrt" else int(c) for c in spec]


def window(chosen, rng, split):
    """(t_start, t_end): with `split`, t_start between the earliest and the latest root of the chosen samples, so that the grids of one
    call are extended by different numbers of cells."""
    roots = sorted(float(s.t[s.root]) for s in chosen)
    t_end = max(float(s.t.max()) for s in chosen) + 0.25
    if split and roots[0] < roots[-1]:
        return 0.5 * (roots[0] + roots[-1]), t_end
    return (roots[0] - 0.3, t_end) if rng.random() < 0.5 else (roots[-1] + 0.37, t_end)
