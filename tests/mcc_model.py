"""Two independent restatements of the reference's MCC tree (core/mcc_tree.cpp:58-181), held against each other and against the device.

The reference has no unit test of mcc_tree.cpp, so there are no expectations of its own to store.  The yardstick is therefore:

(a) `derive_letter`: derive_mcc_tree to the letter -- random 64-bit tip fingerprints XORed up the tree, a dict of counts over the
    fingerprints of ALL nodes of all samples, log clade credibility summed over the inner nodes in node order, the master by
    max_element (first maximum), corresponding nodes bottom-up through find_MRCA_of's walk by node times (phylo_tree.cpp:204-268, its
    equal-times branch included), derived quantities summed over the samples in sample order.
(b) `derive_sets`: the definitions, with no fingerprints and no tree walk by times: a clade is the frozenset of the tips below a node;
    a clade's count is the number of samples that contain that set; an MCC node's corresponding node in a sample is the node of the
    SMALLEST clade of the sample that contains the MCC node's clade (the clades that contain a given tip are a chain under
    inclusion, so it is looked for among the ancestors of one of the clade's tips, smallest first); exact = the two sets are equal.
    Its log clade credibility is the correctly rounded sum of the terms (math.fsum), which has no order at all.

Two samples with the same topology and different node numbering have the same log clade credibility in (b) and sums that can differ
in the last bits in (a), so the two may name different masters among tied samples; `master=` makes either derive the rest from a
given master, and `expected_master` says which index a third implementation has to name.

A sample is a `Sample` of plain numpy arrays (parent, child0, child1, t, root; -1 = no node), the engine's flat layout.
Pure Python / numpy; needs no GPU and nothing of the product.
"""
import math
import random
from dataclasses import dataclass, field
from typing import List

import numpy as np

NO = -1


@dataclass
class Sample:
    parent: np.ndarray
    child0: np.ndarray
    child1: np.ndarray
    t: np.ndarray
    root: int

    @property
    def n(self):
        return int(self.parent.shape[0])

    def is_tip(self, v):
        return self.child0[v] == NO

    def inner_nodes(self):
        return [v for v in range(self.n) if self.child0[v] != NO]

    def post_order(self):
        out, stack = [], [(self.root, False)]
        while stack:
            v, done = stack.pop()
            if done or self.child0[v] == NO:
                out.append(v)
            else:
                stack.append((v, True)); stack.append((int(self.child1[v]), False)); stack.append((int(self.child0[v]), False))
        return out

    def copy(self):
        return Sample(self.parent.copy(), self.child0.copy(), self.child1.copy(), self.t.copy(), int(self.root))


@dataclass
class Mcc:
    master: int
    log_cc: List[float]
    log_cc_terms_abs: List[float]        # per sample, the sum of |term|: what a bound on the summation error is made of
    num_exact: np.ndarray                # [n] per MCC node
    support: np.ndarray
    t: np.ndarray
    t_mrca: np.ndarray
    corr: np.ndarray                     # [M][n] node in sample k that corresponds to MCC node v
    exact: np.ndarray                    # [M][n] bool
    inner_counts: list = field(default_factory=list)   # per sample: {inner node: in how many samples its clade occurs}


# ---- (a) to the letter -----------------------------------------------------------------------------------------------------
def find_mrca_by_times(s: Sample, p: int, q: int) -> int:
    """find_MRCA_of (phylo_tree.cpp:204-268)."""
    if p == NO: return p
    if q == NO: return q
    while p != q:
        tp, tq = s.t[p], s.t[q]
        if tp > tq:
            p = int(s.parent[p]); assert p != NO
        elif tp < tq:
            q = int(s.parent[q]); assert q != NO
        elif s.is_tip(p):
            p = int(s.parent[p]); assert p != NO
        elif s.is_tip(q):
            q = int(s.parent[q]); assert q != NO
        else:
            anc_p, anc_q = [], []
            cur = p
            while cur != NO: anc_p.append(cur); cur = int(s.parent[cur])
            cur = q
            while cur != NO: anc_q.append(cur); cur = int(s.parent[cur])
            cand = s.root
            while anc_p and anc_q and anc_p[-1] == anc_q[-1]:
                cand = anc_p[-1]; anc_p.pop(); anc_q.pop()
            return cand
    return p


def _fingerprints(s: Sample, fp: list):
    """calc_inner_node_clade_fingerprints (mcc_tree.cpp:30-41); fp holds the tips' on entry."""
    for v in s.post_order():
        if not s.is_tip(v):
            fp[v] = fp[s.child0[v]] ^ fp[s.child1[v]]


def derive_letter(samples: List[Sample], seed: int = 0, master=None) -> Mcc:
    M = len(samples); assert M > 0
    n = samples[0].n
    rng = random.Random(seed)
    fp = [0] * n
    for v in range(n):
        if samples[0].is_tip(v): fp[v] = rng.getrandbits(64)
    log_i_over_m = [-math.inf] + [math.log(i) - math.log(M) for i in range(1, M + 1)]
    counts = {}
    for s in samples:
        _fingerprints(s, fp)
        for f in fp: counts[f] = counts.get(f, 0) + 1
    log_cc, abs_terms, inner_counts = [0.0] * M, [0.0] * M, []
    for i, s in enumerate(samples):
        _fingerprints(s, fp)
        ic = {}
        for v in range(n):
            if not s.is_tip(v):
                term = log_i_over_m[counts[fp[v]]]
                log_cc[i] += term; abs_terms[i] += abs(term); ic[v] = counts[fp[v]]
        inner_counts.append(ic)
    if master is None: master = max(range(M), key=lambda i: (log_cc[i], -i))          # max_element: the first maximum
    mcc = samples[master]
    mcc_fp = list(fp); _fingerprints(mcc, mcc_fp)
    corr = np.full((M, n), NO, np.int64); exact = np.zeros((M, n), bool)
    order = mcc.post_order()
    for i, s in enumerate(samples):
        _fingerprints(s, fp)
        c = [NO] * n
        for v in order:
            c[v] = v if mcc.is_tip(v) else find_mrca_by_times(s, c[mcc.child0[v]], c[mcc.child1[v]])
            corr[i, v] = c[v]; exact[i, v] = fp[c[v]] == mcc_fp[v]
    return _derived(samples, master, log_cc, abs_terms, corr, exact, inner_counts)


def _derived(samples, master, log_cc, abs_terms, corr, exact, inner_counts) -> Mcc:
    """Mcc_tree::calculate_derived_quantities (mcc_tree.cpp:158-179): the sums over the samples in sample order."""
    M, n = len(samples), samples[0].n
    num_exact = np.zeros(n, np.int64); support = np.zeros(n); t = np.zeros(n); t_mrca = np.zeros(n)
    for v in range(n):
        sum_t, sum_t_mrca, hits = 0.0, 0.0, 0
        for i, s in enumerate(samples):
            tc = float(s.t[corr[i, v]])
            sum_t_mrca += tc
            if exact[i, v]: sum_t += tc; hits += 1
        assert hits > 0
        num_exact[v] = hits; support[v] = float(hits) / M; t[v] = sum_t / hits; t_mrca[v] = sum_t_mrca / M
    return Mcc(master, list(log_cc), list(abs_terms), num_exact, support, t, t_mrca, corr, exact, inner_counts)


# ---- (b) the definitions ---------------------------------------------------------------------------------------------------
def clades_of(s: Sample):
    """frozenset of tips below every node."""
    c = [None] * s.n
    for v in s.post_order():
        c[v] = frozenset((v,)) if s.is_tip(v) else c[s.child0[v]] | c[s.child1[v]]
    return c


def derive_sets(samples: List[Sample], master=None) -> Mcc:
    M = len(samples); assert M > 0
    n = samples[0].n
    clades = [clades_of(s) for s in samples]
    in_samples = {}
    for c in clades:
        for cl in set(c): in_samples[cl] = in_samples.get(cl, 0) + 1
    log_cc, abs_terms, inner_counts = [], [], []
    for s, c in zip(samples, clades):
        ic = {v: in_samples[c[v]] for v in s.inner_nodes()}
        terms = [math.log(k) - math.log(M) for k in ic.values()]
        log_cc.append(math.fsum(terms)); abs_terms.append(math.fsum(abs(x) for x in terms)); inner_counts.append(ic)
    if master is None: master = max(range(M), key=lambda i: (log_cc[i], -i))
    mcc_clades = clades[master]
    corr = np.full((M, n), NO, np.int64); exact = np.zeros((M, n), bool)
    for i, (s, c) in enumerate(zip(samples, clades)):
        for v in range(n):
            want = mcc_clades[v]
            u = next(iter(want))                     # any tip of the clade: the clades that contain it are its ancestors', smallest first
            while not want <= c[u]: u = int(s.parent[u])
            corr[i, v] = u; exact[i, v] = c[u] == want
    return _derived(samples, master, log_cc, abs_terms, corr, exact, inner_counts)


def log_cc_bound(num_inner: int, abs_terms: float) -> float:
    """First-order bound on the difference of two floating-point sums of the same num_inner terms in different orders, u = 2^-53: each
    partial sum is at most sum|terms| in magnitude, each of the num_inner - 1 additions rounds once, and the histogram form (hist[c] times the
    term, then added) rounds once more per product; the two orders share their terms, so the bound is taken once, with two roundings to spare:
    (num_inner + 2) u sum|terms|."""
    return (num_inner + 2) * 2.0 ** -53 * abs_terms


def count_histogram(inner_counts: dict):
    """{c: number of inner nodes whose clade is in c samples}, as a sorted tuple: two samples with the same histogram have the same
    log clade credibility as a real number, term for term."""
    h = {}
    for c in inner_counts.values(): h[c] = h.get(c, 0) + 1
    return tuple(sorted(h.items()))


def tie_kind(samples, model: Mcc, num_inner: int) -> str:
    """How the master of a sample set is decided: "gap" (best and second-best distinct log_cc further apart than twice the bound),
    "same topology" (everything within the bound of the best has the best's topology), "same histogram" (... the best's histogram
    of clade counts, with another topology: an exact tie all the same, e.g. ANY two different trees at M = 2), or "rounding" (sums
    that differ as real numbers by less than the bound, or are equal only as real numbers: log 2 + log 2 = log 1 + log 4)."""
    if not expected_master(model, num_inner)[1]: return "gap"
    best = max(model.log_cc)
    bound = max(log_cc_bound(num_inner, a) for a in model.log_cc_terms_abs)
    tied = [i for i, x in enumerate(model.log_cc) if best - x <= bound]
    if all(same_topology(samples[tied[0]], samples[i]) for i in tied): return "same topology"
    if len({count_histogram(model.inner_counts[i]) for i in tied}) == 1: return "same histogram"
    return "rounding"


def same_topology(a: Sample, b: Sample) -> bool:
    return set(clades_of(a)) == set(clades_of(b))


def expected_master(model: Mcc, num_inner: int):
    """(index the device must report, decided_by_bound): where the model's best and second-best DISTINCT log_cc differ by more than twice
    the bound the master is the model's; otherwise the first index among those within the bound of the best."""
    best = max(model.log_cc)
    bound = max(log_cc_bound(num_inner, a) for a in model.log_cc_terms_abs)
    distinct = sorted(set(model.log_cc), reverse=True)
    if len(distinct) == 1 or distinct[0] - distinct[1] > 2 * bound:
        return model.master, False
    return min(i for i, x in enumerate(model.log_cc) if best - x <= bound), True


# ---- sample sets for the sweeps ---------------------------------------------------------------------------------------------
def random_tree(rng: random.Random, num_tips: int, tip_ids, inner_ids, integer_times=False) -> Sample:
    """A random binary tree (random joins) on the given node indices, times decreasing towards the root."""
    n = 2 * num_tips - 1
    parent = np.full(n, NO, np.int32); c0 = np.full(n, NO, np.int32); c1 = np.full(n, NO, np.int32); t = np.zeros(n)
    live = []
    for v in tip_ids:
        t[v] = rng.randint(0, 3) if integer_times else rng.uniform(0.0, 3.0)
        live.append(v)
    for v in inner_ids:
        a = live.pop(rng.randrange(len(live))); b = live.pop(rng.randrange(len(live)))
        c0[v], c1[v] = a, b; parent[a] = parent[b] = v
        lo = min(t[a], t[b])
        t[v] = lo - (rng.randint(0, 2) if integer_times else rng.uniform(0.01, 1.0))
        live.append(v)
    return Sample(parent, c0, c1, t, int(live[0]))


def _below(s: Sample, v: int):
    out, stack = set(), [v]
    while stack:
        u = stack.pop(); out.add(u)
        if s.child0[u] != NO: stack.append(int(s.child0[u])); stack.append(int(s.child1[u]))
    return out


def random_spr(rng: random.Random, s: Sample, integer_times=False) -> bool:
    """One subtree-prune-and-regraft in place, node times kept consistent (a parent is never later than its children)."""
    n = s.n
    if n < 5: return False
    for _ in range(20):
        v = rng.randrange(n)
        p = int(s.parent[v])
        if p == NO: continue
        sib = int(s.child1[p] if s.child0[p] == v else s.child0[p])
        sub = _below(s, v)
        w = rng.randrange(n)
        if w in sub or w == p or w == sib: continue
        gw = int(s.parent[w])                        # (not p: w is neither v nor its sibling; so taking p out leaves it w's parent)
        hi = min(s.t[w], s.t[v])
        if gw != NO and not s.t[gw] <= hi: continue  # no time for p between w's parent and both of its new children
        # take p out: its other child takes its place
        g = int(s.parent[p])
        s.parent[sib] = g
        if g == NO: s.root = sib
        elif s.child0[g] == p: s.child0[g] = sib
        else: s.child1[g] = sib
        # put p in above w
        s.parent[p] = gw
        if gw == NO: s.root = p
        elif s.child0[gw] == w: s.child0[gw] = p
        else: s.child1[gw] = p
        s.child0[p], s.child1[p] = (v, w) if rng.random() < 0.5 else (w, v)
        s.parent[w] = p; s.parent[v] = p
        lo = s.t[gw] if gw != NO else hi - 2.0
        s.t[p] = rng.randint(math.ceil(lo), math.floor(hi)) if integer_times and math.ceil(lo) <= math.floor(hi) else rng.uniform(lo, hi)
        return True
    return False


def relabel_inner(rng: random.Random, s: Sample) -> Sample:
    """The same tree with its inner nodes renumbered at random (tips keep their indices, as the reference assumes)."""
    inner = s.inner_nodes()
    shuffled = list(inner); rng.shuffle(shuffled)
    m = np.arange(s.n); m[inner] = shuffled
    mm = lambda a: np.where(a == NO, NO, m[np.maximum(a, 0)]).astype(np.int32)
    out = Sample(np.full(s.n, NO, np.int32), np.full(s.n, NO, np.int32), np.full(s.n, NO, np.int32), np.zeros(s.n), int(m[s.root]))
    out.parent[m] = mm(s.parent); out.child0[m] = mm(s.child0); out.child1[m] = mm(s.child1); out.t[m] = s.t
    return out


def random_sample_set(rng: random.Random, max_tips: int, max_samples: int) -> List[Sample]:
    """Samples perturbed from one another by random SPRs, so that clades are shared; every few sets with integer node times (equal
    times between distinct nodes, parents and children included), every few with some samples repeated under another numbering."""
    num_tips = rng.randint(2, max_tips); M = rng.randint(1, max_samples)
    n = 2 * num_tips - 1
    ids = list(range(n)); rng.shuffle(ids)
    tips, inner = sorted(ids[:num_tips]), ids[num_tips:]
    integer_times = rng.random() < 0.25
    cur = random_tree(rng, num_tips, tips, inner, integer_times)
    out = []
    for k in range(M):
        if k and rng.random() < 0.15:
            out.append(relabel_inner(rng, out[rng.randrange(len(out))])); continue
        for _ in range(rng.choice((0, 1, 1, 2, 4))): random_spr(rng, cur, integer_times)
        if rng.random() < 0.5:
            for v in cur.post_order():       # new node times, consistent
                if cur.is_tip(v): continue
                lo = min(cur.t[cur.child0[v]], cur.t[cur.child1[v]])
                cur.t[v] = lo - (rng.randint(0, 2) if integer_times else rng.uniform(0.01, 1.0))
        out.append(relabel_inner(rng, cur) if rng.random() < 0.5 else cur.copy())
    return out


def check_times(s: Sample):
    for v in range(s.n):
        if s.parent[v] != NO: assert s.t[s.parent[v]] <= s.t[v]
