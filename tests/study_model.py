"""The exact model of ONE candidate study: what an SPR1 move's two scans and their weights amount to, restated from the
definitions -- a third party for the HIP engine (emat_device_spr.hpp: wave_local_scan, study_seed_fill, wave_make_study,
root_region_log_weight, study_log_alpha_in_region) and the CPU oracle (oracle/orc_spr.hpp), which restate the reference's
depth-first builder in the same order and so can share a mistake.

Nothing here calls the oracle or the engine, nothing here is an interval set and nothing here is a work stack: sets of sites
are boolean arrays, numbers are Fractions or 60-digit mpmath numbers (exact_model's arithmetic), results are `Exact`.

The pruned tree (spr_study.h:48-57: "will generate regions as if the parent node P of X were not in the tree").  Take a
part's tree and the model's graft of X (graft_model.GraftModel.graft).  Every mutation the graft calls hot is read off; X's
subtree and P leave; P's branch and the sibling's become one branch whose mutations are P's that remain followed by the
sibling's.  When P is the run's root, the sibling becomes the root with its own sequence and every mutation of its branch was
hot.  What remains does not depend on where X hangs: `Pruned.same_as` says so of the trees before and after an accepted move.

Regions (spr_study.h:9-15, 90-101; spr_study.cpp:211-224).  A region is a maximal stretch of a branch of the pruned tree
between consecutive mutations (ALL mutations), (t_min, t_max]; t_max is cut at t_X and a stretch with t_min >= t_X is dropped.
A part that holds the run's root has one more region above its root, t_min = -inf; in another part the root's branch holds no
region (spr_study.cpp:150-158).

min_muts (spr_study.h:13, spr_study.cpp:93-101) of a region: the number of sites, not missing at X, where the pruned tree's
sequence in the region -- the reference sequence with the mutations from the root down to the region applied -- differs from
X's.  Sites only X's side has data for (the graft's open infos) count as equal: the deltas a scan starts from are the closed
infos' alone (subrun.cpp:547, 594: summarize_closed_mutations), and no mutation of the pruned tree lies on such a site.

Reach (spr_study.h:59-60, 86-89; spr_study.cpp:63-79).  The start point is the top of the start sibling's branch: on the joined
branch the point between P's mutations and the sibling's, above the root when the sibling became the root.  A region belongs
to a study of limit k when the one path from the start point to it crosses at most k mutations at sites not missing at X;
limit None is every region.  The regions form a tree, so the path and its count are unique: no walk order enters.

Weights (spr_study.cpp:226-385), f = 0.8, lambda_X = lambda_i[X], mu = lambda_X / (L - sites missing at X), a region below
the root with t' = (t_min + t_max) / 2:  log W = log(f lambda_X (t_max - t_min)) + f (-lambda_X (t_X - t') + m log(mu (t_X - t') / 3)).
Above the root, t_S the root's time, s_min = |t_X - t_S|, s_max = s_min + 20 (t_max_tip - min(t_X, t_S)), x = lambda_X f s,
a = f m + 1:  x_max < 0.01:  log W = -log 2 + log(f lambda_X) + f m log(mu / 3) + a log s_max + log1p(-(s_min / s_max)^a) - log a;
otherwise  log W = -log 2 + f m log(mu / (3 lambda_X f)) + lgamma(a) + log(Q(a, x_min) - Q(a, x_max)).
p_i = W_i / sum W.  Densities (spr_study.cpp:486-549): below the root log p_i - log(t_max - t_min); above it, s = (t_X - t) +
(t_S - t), power law: log p_i + log 2 + log a + (a - 1) log s - a log s_max - log1p(-(s_min / s_max)^a); gamma: log p_i + log 2 +
log(lambda_X f) + f m log(lambda_X f s) - lambda_X f s - lgamma(a) - log(Q(a, x_min) - Q(a, x_max)).

S and n (exact_model's rules), term by term:
- log(f lambda_X D), D = t_max - t_min one difference of stored times: |log| + 1;
- -f lambda_X (t_X - t'): t' is a rounded mean and t_X - t' a difference of unlike magnitudes: f lambda_X (|t_X| + |t'|);
- f m log(mu (t_X - t') / 3): f m (|log| + 1 + (|t_X| + |t'|) / (t_X - t'));
- the root's power law: log 2, |log(f lambda_X)| + 1, f m (|log(mu / 3)| + 1), a (|log s_max| + 1), |log1p| + 1 +
  a (1 + |log(s_min / s_max)|) r / (1 - r) with r = (s_min / s_max)^a, |log a| + 1;
- the root's gamma: log 2, f m (|log(mu / (3 lambda_X f))| + 1), |lgamma| + 1, |log(Q_lo - Q_hi)| + 4 (x_min g(x_min) + x_max g(x_max)) /
  (Q_lo - Q_hi) with g the gamma density (the relative roundings of x_min and x_max);
- log p_i = (log W_i - M) - log sum exp(log W_j - M): log W_i's own S, |log W_i - M|; log(sum W) carries the sum over regions of
  W_j times (log W_j's own S + 1 + 2 |log W_j - M|) divided by sum W, plus one u per addition (regions / (n + 8) joins S), and
  |log sum| + 1; |log p_i|;
- a density adds |log D| + 1 below the root; above it the terms' magnitudes as above, with s a sum of two differences:
  (|t_X| + 2 |t| + |t_S|) / s times the exponent;  n = 24.
Named apart, as the prior's k_term is:
- `gamma_term`: the incomplete-gamma difference gets the tolerance the project holds gamma_q to, 1e-12 + 1e-9 Q per value
  (test_oracle_pinning.check_gamma_reference_cases), divided by (Q_lo - Q_hi), once for log W of the root region where it
  enters log p_i (times p_root, and once more when i is the root region) and once for the density above the root;
- `lambda_sensitivity`: |d log alpha / d log lambda_X|.  lambda_X is itself computed (exact_model.Derived.lambda_i: value, S, n),
  so a caller adds (n + 8) u S / lambda_X times this, as check_accepted_slide does for the proposal rate.

Reference lines: core/spr_study.h:17-171, core/spr_study.cpp:9-24, 93-128, 130-224, 226-385, 486-549; core/subrun.cpp:492-675.
"""
from fractions import Fraction as F

import mpmath
import numpy as np

import exact_model as X
from exact_model import Exact

F_ANNEAL = F(0.8)                     # subrun.cpp:511: annealing_factor = 0.8, the double
_mp = X._mp


class Pruned:
    """The part's tree with X's graft read off and X's subtree and P taken out.  kids / parent / t over the nodes that remain,
    muts[b] = [(site, from, to, t)] per branch, root, root_seq; start_branch and start_idx: the start point of a scan from X's
    sibling (region start_idx of branch start_branch; the root's one region when the sibling became the root)."""

    def __init__(self, gm, Xn):
        T = gm.T
        g = gm.graft(Xn)
        P, S = T.parent[Xn], g.S
        L = gm.L
        path = [Xn]
        while path[-1] != T.root:
            path.append(T.parent[path[-1]])
        hot_on = {}
        self.only_X = np.zeros(L, bool)             # sites of the open infos: only X's side has data there
        if g.rooty:
            px, ps, c = g.infos
            hot_on[Xn], hot_on[S] = px.hot | c.hot, ps.hot | c.hot
            self.only_X |= px.hot
        else:
            for j, b in enumerate(g.infos):
                for k in range((len(path) - 2 if b.is_open else j) + 1):
                    hot_on[path[k]] = hot_on.get(path[k], np.zeros(L, bool)) | b.hot
                if b.is_open:
                    self.only_X |= b.hot
        # (what the graft lists as hot is what these masks take: GraftModel._on_branch of the same masks)
        assert sum(len(b.muts) for b in g.infos) == sum(1 for br, m in hot_on.items() for (l, _, _, _) in T.muts[br] if m[l])
        gone, st = set(), [Xn]
        while st:
            v = st.pop(); gone.add(v); st += T.kids[v]
        gone.add(P)
        keep = lambda br: [m for m in T.muts[br] if br not in hot_on or not hot_on[br][m[0]]]
        self.Xn, self.S, self.t_X = Xn, S, T.t[Xn]
        self.nodes = [v for v in T.pre if v not in gone]
        self.parent = {v: T.parent[v] for v in self.nodes}
        self.kids = {v: [k for k in T.kids[v] if k not in gone] for v in self.nodes}
        self.t = {v: T.t[v] for v in self.nodes}
        self.muts = {v: keep(v) for v in self.nodes}
        if g.rooty:
            assert not self.muts[S], "a mutation of the root's other branch is not part of the rooty graft"
            self.root, self.parent[S] = S, -1
            self.root_seq = gm.seq_at(S).copy()
            self.muts[S] = []
            self.start_branch, self.start_idx = S, 0
        else:
            G = T.parent[P]
            self.root = T.root
            self.parent[S] = G
            self.kids[G] = [S if k == P else k for k in T.kids[G]]
            self.start_branch, self.start_idx = S, len(keep(P))
            self.muts[S] = keep(P) + self.muts[S]
            self.root_seq = gm.seq_at(T.root).copy()
            self.muts[self.root] = []               # (the root's own list spells root_seq against the reference sequence)
        self.data = np.zeros(L, bool)               # sites some tip that remains has data for
        for k in range(len(path) - 1):
            self.data |= gm.data(gm.sibling(path[k]))
        self.missing_at_X = gm.missing_at(Xn).copy()
        self.seq_X = gm.seq_at(Xn).copy()
        self.L = L

    def same_as(self, o):
        """Raises AssertionError where the two pruned trees differ: topology, every mutation's site and states, node and mutation
        times bit for bit, the root's sequence where the pruned tree has data.  (The times a rooty graft reflects about the run's root
        never get here: every mutation of the root's other branch is hot and was read off, which __init__ asserts.)"""
        assert self.root == o.root and self.Xn == o.Xn, "roots %d and %d" % (self.root, o.root)
        assert sorted(self.nodes) == sorted(o.nodes), "the pruned trees hold different nodes"
        for v in self.nodes:
            assert self.parent[v] == o.parent[v] and sorted(self.kids[v]) == sorted(o.kids[v]), "node %d: links differ" % v
            assert self.t[v] == o.t[v], "node %d: time %r and %r" % (v, float(self.t[v]), float(o.t[v]))
            a, b = self.muts[v], o.muts[v]
            assert [m[:3] for m in a] == [m[:3] for m in b], "branch %d: mutations %s and %s" % (v, [m[:3] for m in a], [m[:3] for m in b])
            for x, y in zip(a, b):
                assert np.float64(x[3]).tobytes() == np.float64(y[3]).tobytes(), "branch %d: mutation time %r and %r" % (v, x[3], y[3])
        assert np.array_equal(self.data, o.data), "the pruned trees have data at different sites"
        assert np.array_equal(self.root_seq[self.data], o.root_seq[o.data]), "the pruned trees' root sequences differ"
        assert np.array_equal(self.missing_at_X, o.missing_at_X) and np.array_equal(self.seq_X[~self.missing_at_X], o.seq_X[~o.missing_at_X]), "X's own sequence changed"


class Region:
    __slots__ = ("branch", "idx", "t_min", "t_max", "m", "above_root", "crossed", "uncounted")

    def __repr__(self):
        return "Region(branch %d, idx %d, (%s, %r], m %d, crossed %s)" % (self.branch, self.idx, "-inf" if self.t_min is None else repr(float(self.t_min)),
                                                                          float(self.t_max), self.m, self.crossed)


def all_regions(pr: Pruned, includes_run_root):
    """Every stretch of the pruned tree as a Region (the root's one stretch too, whether or not it may hold X), with `m` = min_muts
    and `crossed` / `uncounted` = the mutations at sites not missing / missing at X on the path from the start point."""
    count = ~pr.missing_at_X & ~pr.only_X
    regs, by_branch = [], {}
    st = [(pr.root, pr.root_seq)]
    while st:
        v, seq = st.pop()
        seq = seq.copy()
        m = int(np.count_nonzero((seq != pr.seq_X) & count))
        lst = []
        t_prev = None if v == pr.root else pr.t[pr.parent[v]]
        muts = pr.muts[v]
        for i in range(len(muts) + 1):
            r = Region()
            r.branch, r.idx, r.t_min, r.above_root, r.m = v, i, t_prev, v == pr.root, m
            r.t_max = pr.t[v] if i == len(muts) else F(muts[i][3])
            r.crossed = r.uncounted = None
            lst.append(r)
            if i < len(muts):
                l, a, b, _ = muts[i]
                assert seq[l] == a, "branch %d: mutation of site %d from %d, the pruned tree says %d" % (v, l, a, seq[l])
                if count[l]:
                    m += int(b != pr.seq_X[l]) - int(a != pr.seq_X[l])
                seq[l] = b
                t_prev = r.t_max
        by_branch[v] = lst
        regs += lst
        for k in pr.kids[v]:
            st.append((k, seq))
    # the path counts: neighbours are consecutive stretches of a branch (the mutation between them is crossed) and a branch's last
    # stretch with its children's first (nothing is crossed)
    start = by_branch[pr.start_branch][pr.start_idx]
    start.crossed, start.uncounted = 0, 0
    todo = [start]
    while todo:
        r = todo.pop()
        lst, muts = by_branch[r.branch], pr.muts[r.branch]
        nbrs = []
        if r.idx > 0:
            nbrs.append((lst[r.idx - 1], muts[r.idx - 1][0]))
        elif r.branch != pr.root:
            nbrs.append((by_branch[pr.parent[r.branch]][-1], None))
        if r.idx < len(muts):
            nbrs.append((lst[r.idx + 1], muts[r.idx][0]))
        else:
            nbrs += [(by_branch[k][0], None) for k in pr.kids[r.branch]]
        for q, site in nbrs:
            if q.crossed is None:
                c = site is not None and not pr.missing_at_X[site]
                u = site is not None and bool(pr.missing_at_X[site])
                q.crossed, q.uncounted = r.crossed + int(c), r.uncounted + int(u)
                todo.append(q)
    assert all(r.crossed is not None for r in regs)
    return regs


class Density:
    """log_alpha of one (region, time): `exact` (value, S, n), `gamma_term` and `lambda_sensitivity` (the module's docstring)."""
    __slots__ = ("exact", "gamma_term", "lambda_sensitivity", "region", "branch_kind")


class Study:
    """The study of limit `limit` (None: unlimited) scanned from pr's start point.  lam: Exact lambda_i[X]; t_max_tip: a float."""

    def __init__(self, pr: Pruned, includes_run_root, limit, lam: Exact, t_max_tip, f=F_ANNEAL):
        self.pr, self.limit, self.f, self.lam = pr, limit, f, lam
        t_X = pr.t_X
        self.regions = []
        for r in all_regions(pr, includes_run_root):
            if limit is not None and r.crossed > limit:
                continue
            if r.above_root and not includes_run_root:
                continue
            if r.t_min is not None and r.t_min >= t_X:
                continue
            if r.t_max > t_X:
                r.t_max = t_X
            self.regions.append(r)
        assert self.regions, "a study without regions"
        n_X = pr.L - int(pr.missing_at_X.sum())
        self.mu = lam.value / n_X
        self.t_max_tip = F(float(t_max_tip))
        with mpmath.workdps(X._DPS):
            self._weigh()

    def _root_params(self, r):
        t_X, t_S = self.pr.t_X, self.pr.t[r.branch]
        s_min = abs(t_X - t_S)
        span = self.t_max_tip - min(t_X, t_S)
        assert span >= 0
        s_max = s_min + 20 * span
        lf = self.lam.value * self.f
        x_min, x_max = lf * s_min, lf * s_max
        assert abs(x_max - F(1, 100)) > F(1, 10 ** 12), "x_max too close to the switch between the two densities to say which the code takes"
        return t_S, s_min, s_max, x_min, x_max, self.f * r.m + 1

    def _weigh(self):
        mp = mpmath
        f, lam, mu, t_X = _mp(self.f), _mp(self.lam.value), _mp(self.mu), self.pr.t_X
        n = len(self.regions)
        self.lw, self.lw_S, self.dlam, self.gamma_w = [None] * n, [0.0] * n, [0.0] * n, [0.0] * n
        self.root_kind = None
        for i, r in enumerate(self.regions):
            m = r.m
            if not r.above_root:
                D, tp = r.t_max - r.t_min, (r.t_min + r.t_max) / 2
                tau = t_X - tp
                if D == 0 or (tau == 0 and m > 0):
                    continue                                    # log W = -inf: a stretch between two mutations at the same time
                mag = _mp(abs(t_X) + abs(tp))
                l1 = mp.log(f * lam * _mp(D))
                lw, S = l1 - f * lam * _mp(tau), abs(l1) + 1 + f * lam * mag
                if m:
                    l2 = mp.log(mu * _mp(tau) / 3)
                    lw += f * m * l2
                    S += f * m * (abs(l2) + 1 + mag / _mp(tau))
                self.lw[i], self.lw_S[i], self.dlam[i] = lw, S, float(f * m - f * lam * _mp(tau))
            else:
                t_S, s_min, s_max, x_min, x_max, a = self._root_params(r)
                a = _mp(a)
                if x_max < F(1, 100):
                    self.root_kind = "power"
                    rr = mp.power(_mp(s_min) / _mp(s_max), a)
                    l1, l2, l3, l4 = mp.log(f * lam), mp.log(mu / 3), mp.log(_mp(s_max)), mp.log1p(-rr)
                    lw = -mp.log(2) + l1 + f * m * l2 + a * l3 + l4 - mp.log(a)
                    lrat = abs(mp.log(_mp(s_min) / _mp(s_max))) if s_min else 0
                    S = mp.log(2) + abs(l1) + 1 + f * m * (abs(l2) + 1) + a * (abs(l3) + 1) + abs(l4) + 1 + a * (1 + lrat) * rr / (1 - rr) + abs(mp.log(a)) + 1
                    self.lw[i], self.lw_S[i], self.dlam[i] = lw, S, float(f * m)
                else:
                    self.root_kind = "gamma"
                    q_lo, q_hi = mp.gammainc(a, _mp(x_min), mp.inf, regularized=True), mp.gammainc(a, _mp(x_max), mp.inf, regularized=True)
                    qd = q_lo - q_hi
                    g = lambda x: mp.exp((a - 1) * mp.log(x) - x - mp.loggamma(a)) if x > 0 else (mp.mpf(1) if a == 1 else mp.mpf(0))
                    xg_lo, xg_hi = _mp(x_min) * g(_mp(x_min)), _mp(x_max) * g(_mp(x_max))
                    l1, l2, l3 = mp.log(mu / (3 * lam * f)), mp.loggamma(a), mp.log(qd)
                    lw = -mp.log(2) + f * m * l1 + l2 + l3
                    S = mp.log(2) + f * m * (abs(l1) + 1) + abs(l2) + 1 + abs(l3) + 4 * (xg_lo + xg_hi) / qd
                    self.lw[i], self.lw_S[i] = lw, S
                    self.dlam[i] = float((xg_hi - xg_lo) / qd - 1)
                    self.gamma_w[i] = float(((1e-12 + 1e-9 * q_lo) + (1e-12 + 1e-9 * q_hi)) / qd)
                    self._root_gamma = (l2, l3, (xg_hi - xg_lo) / qd)
        live = [i for i in range(n) if self.lw[i] is not None]
        assert live, "every region of the study has weight 0"
        M = max(self.lw[i] for i in live)
        w = {i: mp.exp(self.lw[i] - M) for i in live}
        tot = sum(w.values())
        self.log_p = [None] * n
        self.log_p_S = [0.0] * n
        self.log_p_gamma = [0.0] * n
        self.log_p_dlam = [0.0] * n
        sum_S = sum(w[i] * (self.lw_S[i] + 1 + 2 * abs(self.lw[i] - M)) for i in live) / tot
        sum_gamma = sum(float(w[i] / tot) * self.gamma_w[i] for i in live)
        mean_dlam = sum(float(w[i] / tot) * abs(self.dlam[i]) for i in live)
        ltot = mp.log(tot)
        for i in live:
            lp = (self.lw[i] - M) - ltot
            self.log_p[i] = lp
            self.log_p_S[i] = self.lw_S[i] + abs(self.lw[i] - M) + sum_S + mp.mpf(len(live)) / 32 + abs(ltot) + 1 + abs(lp)
            self.log_p_gamma[i] = self.gamma_w[i] + sum_gamma
            self.log_p_dlam[i] = abs(self.dlam[i]) + mean_dlam

    def probabilities(self):
        """[p_i] as floats (0 for a region of weight 0)."""
        with mpmath.workdps(X._DPS):
            return [0.0 if lp is None else float(mpmath.exp(lp)) for lp in self.log_p]

    def find(self, branch, t):
        """The index of the region of `branch` that holds time t (spr_study.cpp:474-484), or -1."""
        t = F(float(t))
        hit = [i for i, r in enumerate(self.regions) if r.branch == branch and (r.t_min is None or r.t_min < t) and t <= r.t_max]
        assert len(hit) <= 1
        return hit[0] if hit else -1

    def log_alpha(self, i, t) -> Density:
        with mpmath.workdps(X._DPS):
            return self._log_alpha(i, F(float(t)))

    def _log_alpha(self, i, t):
        mp = mpmath
        r = self.regions[i]
        assert self.log_p[i] is not None, "a time in a region of weight 0"
        f, lam = _mp(self.f), _mp(self.lam.value)
        d = Density()
        d.region, d.gamma_term, d.lambda_sensitivity = r, self.log_p_gamma[i], self.log_p_dlam[i]
        v, S = self.log_p[i], self.log_p_S[i]
        if not r.above_root:
            d.branch_kind = "below"
            lD = mp.log(_mp(r.t_max - r.t_min))
            v, S = v - lD, S + abs(lD) + 1
        else:
            t_X = self.pr.t_X
            t_S, s_min, s_max, x_min, x_max, a = self._root_params(r)
            a, m = _mp(a), r.m
            s = (t_X - t) + (t_S - t)
            assert s >= s_min and s <= s_max + F(1, 10 ** 6), "a time above the root outside the density's support"
            smag = _mp(abs(t_X) + 2 * abs(t) + abs(t_S)) / _mp(s)
            ls = mp.log(_mp(s))
            if self.root_kind == "power":
                d.branch_kind = "power"
                rr = mp.power(_mp(s_min) / _mp(s_max), a)
                l3, l4 = mp.log(_mp(s_max)), mp.log1p(-rr)
                lrat = abs(mp.log(_mp(s_min) / _mp(s_max))) if s_min else 0
                v = v + mp.log(2) + mp.log(a) + (a - 1) * ls - a * l3 - l4
                S = S + mp.log(2) + abs(mp.log(a)) + 1 + (a - 1) * (abs(ls) + 1 + smag) + a * (abs(l3) + 1) + abs(l4) + 1 + a * (1 + lrat) * rr / (1 - rr)
            else:
                d.branch_kind = "gamma"
                lg, lq, dq = self._root_gamma
                x = lam * f * _mp(s)
                l1, l2 = mp.log(lam * f), mp.log(x)
                v = v + mp.log(2) + l1 + f * m * l2 - x - lg - lq
                S = S + mp.log(2) + abs(l1) + 1 + f * m * (abs(l2) + 1 + smag) + x * (1 + smag) + abs(lg) + 1 + abs(lq)
                d.gamma_term += self.gamma_w[i]
                d.lambda_sensitivity += float(abs(1 + f * m - x - dq))
        d.exact = Exact(X._frac(v), F(float(S)), 24)
        return d
