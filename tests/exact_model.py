"""The exact value of every posterior term the engine maintains, restated from the model's definitions -- a third party for
the HIP engine and the CPU oracle, which evaluate the same sums in the same order and so can share a mistake.

Arithmetic: every sum of products of doubles is a `fractions.Fraction` (a float64 converts exactly), `log` / `exp` /
`expm1` are evaluated by mpmath at 60 digits and taken over as Fractions, and nothing is rounded until a test asks for
float(value).  Nothing here calls the oracle or the engine: `FlatTree` and `PopModel` are read as plain containers.

Every quantity comes back as an `Exact`: its value, its condition magnitude S and its term count n.  S is the sum of the
absolute values of every term the reference's formula adds before anything cancels, so a float64 evaluation of the same
terms in ANY order lies within (n + 8) u S of the value (u = 2^-53; the worst case of recursive summation, plus a few
roundings inside each term).  Rules for the terms:
- a difference of two stored times, t_X - t_P, counts as |t_X - t_P| (it rounds once, relative to its result);
- a computed cell bound t_ref -/+ c t_step counts as |t_ref| + |c t_step| (the product rounds before the sum);
- a factor exp(x) counts its result times (1 + |x|) (a relative error e of x is a relative error |x| e of exp(x)), and a
  log(y) counts |log y| + 1 plus the magnitude of whatever exponent y carries;
- a quantity built on another one (lambda inside a branch's log G, k_bar inside a cell's prior term) counts that one's S
  times the factor it is multiplied by, and adds its n;
- a difference of two states (`partial_log_prior_delta`, `part_log_G_delta`: what one accepted move changed) counts only the
  terms that differ between them, each with the S its own rule above gives it in the state before plus in the state after:
  whatever both states hold alike is never formed by a code that computes the difference, so the bound does not carry the
  total's magnitude.  A cell of the grid differs when its exact k_bar_p differs, an inner node's -log N(t) when its time
  does, a branch when its parent, end times, mutations or lambda do, the root prior when the root's state counts do;
- a term that a move adds to a log MH ratio and takes away again (a displacement's delta log G = d_logG_dt (new_t - old_t)
  and its proposal ratio, the same product) counts twice its magnitude: the sum rounds while it holds that term.

Reference lines of the definitions: core/pop_model.cpp:18-145, 181-204, 247-330; core/phylo_tree_calc.cpp:67-93,
120-371, 390-436, 458-635 and phylo_tree_calc.h:185-210; core/subrun.cpp:17-56; core/scalable_coalescent.cpp:23-187;
core/very_scalable_coalescent.cpp:14-79, 355-386.
"""
from __future__ import annotations

import bisect
import math
from fractions import Fraction as F

import mpmath
import numpy as np

U = 2.0 ** -53
_DPS = 60
_ZERO = F(0)


class Exact:
    """value (a Fraction, or -inf), condition magnitude S >= 0 and number of terms n of one quantity."""
    __slots__ = ("value", "S", "n")

    def __init__(self, value, S, n):
        self.value, self.S, self.n = value, S, int(n)

    @property
    def f(self) -> float:
        return float(self.value)

    def bound(self) -> float:
        """(n + 8) u S: what rounding alone may put between the value and a float64 evaluation of it."""
        return (self.n + 8) * U * float(self.S)

    def err(self, x) -> float:
        """`x`: a float64, or a Fraction (the exact difference of two float64 values an engine reported)."""
        if isinstance(x, F):
            return float(abs(x - self.value)) if isinstance(self.value, F) else math.inf
        x = float(x)
        if not isinstance(self.value, F):
            return 0.0 if x == self.value else math.inf
        if not math.isfinite(x):
            return math.inf
        return float(abs(F(x) - self.value))

    def units(self, x) -> float:
        """|x - value| in units of u S (the bound is n + 8 of them)."""
        e = self.err(x)
        return e / (U * float(self.S)) if self.S else (0.0 if e == 0.0 else math.inf)

    def ok(self, x) -> bool:
        return self.err(x) <= self.bound()

    def __repr__(self):
        return "Exact(%r, S=%.3g, n=%d)" % (float(self.value), float(self.S), self.n)


def _mp(x):
    if isinstance(x, F):
        return mpmath.mpf(x.numerator) / x.denominator
    return mpmath.mpf(x)


def _frac(m) -> F:
    """An mpmath number as the Fraction it is exactly."""
    sign, man, exp, _ = mpmath.mpf(m)._mpf_
    man = -int(man) if sign else int(man)
    return F(man * 2 ** exp) if exp >= 0 else F(man, 2 ** -exp)


def _log(x) -> F:
    with mpmath.workdps(_DPS):
        return _frac(mpmath.log(_mp(x)))


def _exp(x) -> F:
    with mpmath.workdps(_DPS):
        return _frac(mpmath.exp(_mp(x)))


def _expm1(x) -> F:
    with mpmath.workdps(_DPS):
        return _frac(mpmath.expm1(_mp(x)))


def _fl(x):
    """A float64 input (or a numpy scalar) as a Fraction."""
    return F(float(x))


# ---- population models (core/pop_model.cpp) -------------------------------------------------------------------------
class Pop:
    """The population model N(t) a PopModel describes: constant, exponential (with a floor min_pop, either growth sign) or
    skygrid (stepwise or log-linear between knots, constant beyond both ends)."""

    def __init__(self, pm):
        self.kind = pm.kind
        self.popsize_bar_cache = {}
        if pm.kind == 0:
            self.N0 = _fl(pm.p[0])
        elif pm.kind == 1:
            self.t0, self.n0, self.g, self.min_pop = (_fl(v) for v in pm.p[:4])
            self.log_n0 = _log(self.n0)
            self.t_c = None
            if self.min_pop > 0 and self.g != 0:      # N(t_c) = min_pop
                self.t_c = self.t0 + (_log(self.min_pop) - self.log_n0) / self.g
        else:
            self.x = [_fl(v) for v in pm.skygrid_x]
            self.gamma = [_fl(v) for v in pm.skygrid_gamma]
            self.log_linear = pm.skygrid_type == 2
            assert len(self.x) >= 2 and len(self.x) == len(self.gamma) and all(a < b for a, b in zip(self.x, self.x[1:]))

    # log N(t) and the magnitude its exponent carries
    def _sky_interval(self, t):
        """k with t in (x[k-1], x[k]]; 0 for t <= x[0], M + 1 for t > x[M]."""
        return bisect.bisect_left(self.x, t)

    def log_N(self, t):
        """(log N(t) exactly, the magnitude of the exponent a float64 evaluation of N carries)."""
        t = _fl(t) if not isinstance(t, F) else t
        if self.kind == 0:
            return _log(self.N0), _ZERO
        if self.kind == 1:
            arg = self.g * (t - self.t0)
            v = self.log_n0 + arg
            if self.min_pop > 0 and self.min_pop >= _exp(v):
                return _log(self.min_pop), _ZERO
            return v, abs(arg) + abs(self.log_n0)
        k, M = self._sky_interval(t), len(self.x) - 1
        if k == 0:
            return self.gamma[0], abs(self.gamma[0])
        if k > M:
            return self.gamma[M], abs(self.gamma[M])
        if not self.log_linear:
            return self.gamma[k], abs(self.gamma[k])
        c = (t - self.x[k - 1]) / (self.x[k] - self.x[k - 1])
        return (1 - c) * self.gamma[k - 1] + c * self.gamma[k], 3 * (abs(self.gamma[k - 1]) + abs(self.gamma[k]))

    def pop_at_time(self, t) -> Exact:
        v, a = self.log_N(t)
        N = self.N0 if self.kind == 0 else _exp(v)
        return Exact(N, N * (1 + a), 4)

    def neg_log_pop(self, t):
        """(-log N(t), its S): the term an inner node adds to a coalescent prior."""
        v, a = self.log_N(t)
        return -v, abs(v) + a + 1

    def pop_integral(self, a, b) -> Exact:
        """The integral of N(t) over [a, b]."""
        a, b = (x if isinstance(x, F) else _fl(x) for x in (a, b))
        assert a <= b
        if self.kind == 0:
            return Exact((b - a) * self.N0, (b - a) * self.N0, 2)
        if self.kind == 1:
            return self._exp_integral(a, b)
        return self._sky_integral(a, b)

    def _exp_piece(self, lo, hi):
        """(integral of n0 exp(g (t - t0)) over [lo, hi], its S)."""
        if hi <= lo:
            return _ZERO, _ZERO
        x0, d = self.g * (lo - self.t0), self.g * (hi - lo)
        v = self.n0 / self.g * _exp(x0) * _expm1(d)
        return v, abs(v) * (2 + abs(x0) + abs(d))

    def _exp_integral(self, a, b):
        if self.g == 0:
            N = max(self.n0, self.min_pop)
            return Exact((b - a) * N, (b - a) * N, 2)
        if self.t_c is None:
            v, S = self._exp_piece(a, b)
            return Exact(v, S, 6)
        tc = self.t_c
        if self.g > 0:           # the floor holds before t_c
            floor_lo, floor_hi, exp_lo, exp_hi = a, min(b, tc), max(a, tc), b
        else:                    # ... after it
            floor_lo, floor_hi, exp_lo, exp_hi = max(a, tc), b, a, min(b, tc)
        fl = max(_ZERO, floor_hi - floor_lo) * self.min_pop
        v, S = self._exp_piece(exp_lo, exp_hi)
        return Exact(fl + v, fl + S, 8)

    def _sky_integral(self, a, b):
        x, gm, M = self.x, self.gamma, len(self.x) - 1
        ka, kb = self._sky_interval(a), self._sky_interval(b)
        total, S, bias = _ZERO, _ZERO, max(gm[max(ka - 1, 0): min(kb, M) + 1])
        for k in range(ka, kb + 1):
            lo = max(a, x[k - 1]) if k > 0 else a
            hi = min(b, x[k]) if k <= M else b
            if hi <= lo:
                continue
            if k == 0 or k == M + 1 or not self.log_linear or gm[k] == gm[k - 1]:
                g = gm[0] if k == 0 else gm[M] if k == M + 1 else gm[k]
                v, cond = _exp(g) * (hi - lo), 2 + abs(g)
            else:
                w = x[k] - x[k - 1]
                G_lo = gm[k - 1] + (gm[k] - gm[k - 1]) * (lo - x[k - 1]) / w
                G_hi = gm[k - 1] + (gm[k] - gm[k - 1]) * (hi - x[k - 1]) / w
                D = G_hi - G_lo
                v = _exp(G_lo) * (hi - lo) * _expm1(D) / D
                cond = 3 + 3 * (abs(gm[k - 1]) + abs(gm[k])) + abs(D)
            total += v
            S += v * (cond + abs(bias))
        # the float64 form scales by exp(-bias), sums, and returns exp(log(sum) + bias)
        if total > 0:
            S += total * (2 + abs(_log(total)) + abs(bias))
        return Exact(total, S, 2 * (kb - ka + 1) + 6)


# ---- the evolution model ---------------------------------------------------------------------------------------------
class Evo:
    """Partitions beta with mu_beta, pi_beta, Q_beta; per site a rate nu_l and a partition.  rate(l, a) = mu nu_l q_l(a) with
    q(a) = -Q_aa the escape rate of state a; rate(l, a, b) = mu nu_l Q_ab."""

    def __init__(self, mu, pi, q, nu_l, partition_for_site):
        self.mu = [float(m) for m in np.asarray(mu, np.float64).reshape(-1)]
        P = len(self.mu)
        self.pi = np.asarray(pi, np.float64).reshape(P, 4)
        self.q = np.asarray(q, np.float64).reshape(P, 4, 4)
        self.nu = np.asarray(nu_l, np.float64).tolist()
        self.pfs = np.asarray(partition_for_site, np.int64).tolist()
        self.L = len(self.nu)
        self._r, self._rab, self._lograb, self._cum = {}, {}, {}, {}
        self._escape = [[F(-float(self.q[p, a, a])) for a in range(4)] for p in range(P)]

    @property
    def num_partitions(self):
        return len(self.mu)

    @staticmethod
    def of(sc, nu_l=None, evo=None):
        """The evolution model a test configures (helpers.configure): the scenario's HKY, or `evo` = (mu, pi, q, pfs)."""
        L = sc.num_sites
        nu = np.ones(L) if nu_l is None else nu_l
        if evo is not None:
            mu, pi, q, pfs = evo
            return Evo(mu, pi, q, nu, pfs)
        from delphy_amd.engine import hky_q_matrix      # the rate matrix both engines are handed (input data, not arithmetic)
        return Evo([sc.mu], [sc.pi], [hky_q_matrix(sc.kappa, sc.pi)], nu, np.zeros(L, np.int32))

    def q_a(self, l, a) -> F:
        return self._escape[self.pfs[l]][a]

    def rate(self, l, a) -> F:
        key = (self.pfs[l], self.nu[l], a)
        r = self._r.get(key)
        if r is None:
            r = self._r[key] = F(self.mu[key[0]]) * F(key[1]) * self._escape[key[0]][a]
        return r

    def log_rate_ab(self, l, a, b) -> F:
        key = (self.pfs[l], self.nu[l], a, b)
        r = self._lograb.get(key)
        if r is None:
            r = self._lograb[key] = _log(F(self.mu[key[0]]) * F(key[1]) * F(float(self.q[key[0], a, b])))
        return r


# ---- the tree as plain lists ----------------------------------------------------------------------------------------
class _Tree:
    def __init__(self, tree):
        n = tree.num_nodes
        self.n, self.root = n, int(tree.root)
        self.parent = tree.parent[:n].tolist()
        self.kids = [[c for c in (a, b) if c >= 0] for a, b in zip(tree.child0[:n].tolist(), tree.child1[:n].tolist())]
        self.t = [F(x) for x in tree.t[:n].tolist()]
        mo, ms, mf, mt, mtt = tree.mut_offset.tolist(), tree.mut_site.tolist(), tree.mut_from.tolist(), tree.mut_to.tolist(), tree.mut_t.tolist()
        self.muts = [[(ms[k], mf[k], mt[k], mtt[k]) for k in range(mo[i], mo[i + 1])] for i in range(n)]
        io, s, e = tree.miss_offset.tolist(), tree.miss_start.tolist(), tree.miss_end.tolist()
        self.miss = [[(s[k], e[k]) for k in range(io[i], io[i + 1])] for i in range(n)]
        fo, fs, fst = tree.mfs_offset.tolist(), tree.mfs_site.tolist(), tree.mfs_state.tolist()
        self.mfs = [{fs[k]: fst[k] for k in range(fo[i], fo[i + 1])} for i in range(n)]
        self.pre = []
        stack = [self.root]
        while stack:
            x = stack.pop()
            self.pre.append(x)
            stack.extend(reversed(self.kids[x]))
        assert len(self.pre) == n, "tree is not connected"

    def length(self, X):
        return self.t[X] - self.t[self.parent[X]]


def _walk(T: _Tree, ref, evo: Evo, visit):
    """Depth-first over the tree keeping `diff` = {site: state} of the sites whose state at the current node differs from
    the ref and that are not missing there.  visit(X, diff, newly_missing_states) is called on entering X, after X's branch
    is applied; newly_missing_states = [(site, state at the parent)] ... given as (intervals, {site: state != ref}).
    Checks the tree's own bookkeeping on the way: mutation from-states, missation from-states."""
    diff = {}
    stack = [(T.root, False)]
    undo = {}
    while stack:
        X, leaving = stack.pop()
        if leaving:
            for l, old in reversed(undo.pop(X)):
                if old is None:
                    diff.pop(l, None)
                else:
                    diff[l] = old
            continue
        log = []
        gone = {}
        if T.miss[X]:
            for l in [l for l in diff if any(s <= l < e for s, e in T.miss[X])]:
                gone[l] = diff[l]
                log.append((l, diff.pop(l)))
            assert gone == T.mfs[X], "node %d: missation from-states %s, the path says %s" % (X, T.mfs[X], gone)
        for (l, a, b, _) in T.muts[X]:
            cur = diff.get(l, ref[l])
            assert cur == a, "node %d: mutation at site %d from %d, the path says %d" % (X, l, a, cur)
            assert not any(s <= l < e for s, e in T.miss[X]), "node %d: mutation on a missing site %d" % (X, l)
            log.append((l, diff.get(l)))
            if b == ref[l]:
                diff.pop(l, None)
            else:
                diff[l] = b
        visit(X, diff, gone)
        undo[X] = log
        stack.append((X, True))
        for c in reversed(T.kids[X]):
            stack.append((c, False))


class Derived:
    """lambda_i, num_sites_missing and the pieces of log G of one tree (a whole tree or a part), computed exactly."""

    def __init__(self, tree, ref, evo: Evo, brute=False):
        self.T = T = tree if isinstance(tree, _Tree) else _Tree(tree)
        self.ref = ref = np.asarray(ref).tolist()
        self.evo = evo
        L = len(ref)
        assert L == evo.L
        key = bytes(np.asarray(ref, np.uint8))
        cum = evo._cum.get(key)
        if cum is None:                     # Fraction prefix sums of the ref's rates serve long missing intervals
            cum = [_ZERO] * (L + 1)
            for l in range(L):
                cum[l + 1] = cum[l] + evo.rate(l, ref[l])
            evo._cum = {key: cum}
        self.cum = cum
        self.lam = [None] * T.n
        self.lam_S = [None] * T.n
        self.lam_n = [0] * T.n
        self.nsm = [0] * T.n
        self.root_state_diff = None

        def visit(X, diff, gone):
            P = T.parent[X]
            if X == T.root:
                lam, S, n, nsm = cum[L], cum[L], L, 0
                self.root_state_diff = dict(diff)
            else:
                lam, S, n, nsm = self.lam[P], self.lam_S[P], self.lam_n[P], self.nsm[P]
            for s, e in T.miss[X]:              # newly missing: every site of [s, e) at the state it had at the parent
                lam -= cum[e] - cum[s]
                S += cum[e] + cum[s]; n += 2; nsm += e - s
            for l, st in gone.items():
                d = evo.rate(l, st) - evo.rate(l, ref[l])
                lam -= d; S += evo.rate(l, st) + evo.rate(l, ref[l]); n += 2
            for (l, a, b, _) in T.muts[X]:
                ra, rb = evo.rate(l, a), evo.rate(l, b)
                lam += rb - ra; S += ra + rb; n += 2
            self.lam[X], self.lam_S[X], self.lam_n[X], self.nsm[X] = lam, S, n, nsm

        _walk(T, ref, evo, visit)
        if brute:
            self.lam = self._brute_lambda()

    def retimed(self, tree):
        """The Derived of a tree that differs from this one's in node and mutation TIMES only: lambda_i and the missing-site
        counts depend on none of them."""
        d = object.__new__(Derived)
        for k, v in self.__dict__.items():
            setattr(d, k, v)
        d.T = _Tree(tree)
        return d

    def _brute_lambda(self):
        """lambda at every node straight from the definition: the node's whole sequence, site by site."""
        T, ref, evo = self.T, self.ref, self.evo
        out = [None] * T.n
        for X in range(T.n):
            path = []
            c = X
            while c >= 0:
                path.append(c); c = T.parent[c]
            seq = list(ref)
            missing = set()
            for c in reversed(path):
                for (l, a, b, _) in T.muts[c]:
                    seq[l] = b
                for s, e in T.miss[c]:
                    missing.update(range(s, e))
            lam = _ZERO
            for l in range(len(seq)):
                if l not in missing:
                    lam += evo.rate(l, seq[l])
            out[X] = lam
        return out

    def lambda_i(self, X) -> Exact:
        return Exact(self.lam[X], self.lam_S[X], self.lam_n[X])

    def branch_log_G(self, X):
        """(value, S, n) of log G of branch X (phylo_tree_calc.h:185-206): -integral of lambda along the branch plus
        log(mu nu Q_ab) per mutation."""
        T, evo = self.T, self.evo
        tP = T.t[T.parent[X]]
        ln = T.t[X] - tP
        v = -self.lam[X] * ln
        S = self.lam_S[X] * abs(ln)
        n = 1
        for (l, a, b, mt) in T.muts[X]:
            ra, rb, dt = evo.rate(l, a), evo.rate(l, b), F(mt) - tP
            v -= (ra - rb) * dt
            lg = evo.log_rate_ab(l, a, b)
            v += lg
            S += (ra + rb) * abs(dt) + abs(lg) + 3
            n += 2
        return v, S, n

    def log_G_below_root(self) -> Exact:
        v, S, n, nl = _ZERO, _ZERO, 0, 0
        for X in range(self.T.n):
            if X != self.T.root:
                a, b, c = self.branch_log_G(X)
                v += a; S += b; n += c; nl = max(nl, self.lam_n[X])
        return Exact(v, S, n + nl)

    def root_state_counts(self):
        """f[beta][a]: sites of partition beta in state a at the root, those missing there left out."""
        T, ref, evo = self.T, self.ref, self.evo
        f = [[0] * 4 for _ in range(evo.num_partitions)]
        for l in range(len(ref)):
            f[evo.pfs[l]][ref[l]] += 1
        for l, st in self.root_state_diff.items():
            f[evo.pfs[l]][ref[l]] -= 1; f[evo.pfs[l]][st] += 1
        for s, e in T.miss[T.root]:
            for l in range(s, e):               # missing at the root: at the state the ref (and the root's deltas) give
                f[evo.pfs[l]][T.mfs[T.root].get(l, ref[l])] -= 1
        return f

    def log_root_prior(self) -> Exact:
        f = self.root_state_counts()
        v, S = _ZERO, _ZERO
        for p in range(self.evo.num_partitions):
            for a in range(4):
                pi = float(self.evo.pi[p, a])
                if pi == 0.0:
                    if f[p][a] != 0:
                        return Exact(-math.inf, _ZERO, 0)
                    continue
                lg = _log(F(pi)) * f[p][a]
                v += lg; S += abs(lg) + abs(f[p][a])
        return Exact(v, S, 4 * self.evo.num_partitions)

    def part_log_G(self, includes_run_root) -> Exact:
        """Subrun::calc_cur_log_G (subrun.cpp:58-68): the root prior only in the part that holds the run's root."""
        below = self.log_G_below_root()
        if not includes_run_root:
            return below
        rp = self.log_root_prior()
        if not isinstance(rp.value, F):
            return rp
        return Exact(below.value + rp.value, below.S + rp.S, below.n + rp.n)


# ---- sufficient statistics of the global moves ----------------------------------------------------------------------
def stats(tree, ref, evo: Evo):
    """Below the tree's root: T (total branch length), Ttwiddle_l per site (time in each state weighted by its escape rate,
    missing branches left out), Ttwiddle_beta_a (time each partition spends in each state, weighted by nu_l),
    num_muts_l, num_muts_beta_ab, num_muts.  Definitions: phylo_tree_calc.cpp:120-371, 577-635."""
    T = tree if isinstance(tree, _Tree) else _Tree(tree)
    ref = np.asarray(ref).tolist()
    L, P = len(ref), evo.num_partitions
    nu = [F(x) for x in evo.nu]
    length = [T.length(X) if X != T.root else _ZERO for X in range(T.n)]
    below = [_ZERO] * T.n                     # branch length of the subtree below each node, its own branch excluded
    for X in reversed(T.pre):
        for c in T.kids[X]:
            below[X] += below[c] + length[c]
    total = below[T.root]
    # time every site is NOT missing: the whole tree minus, for each missation at Y, Y's branch and everything below
    miss_time = [_ZERO] * (L + 1)
    muts_l = [0] * L
    M = np.zeros((P, 4, 4), np.int64)
    num_muts = 0
    # per site: q(state) x time, beyond the ref-state default; per (beta, a): nu x time
    tw_extra = {}
    tw_extra_S = {}
    beta_a = [[_ZERO] * 4 for _ in range(P)]
    beta_a_S = [[_ZERO] * 4 for _ in range(P)]
    for X in T.pre:
        w = below[X] + length[X]
        for s, e in T.miss[X]:
            miss_time[s] += w; miss_time[e] -= w

    def visit(X, diff, gone):
        nonlocal num_muts
        if X == T.root:
            return
        ln, tP = length[X], T.t[T.parent[X]]
        for l, st in diff.items():              # a site in another state than the ref's along this branch (its bottom end)
            tw_extra[l] = tw_extra.get(l, _ZERO) + (evo.q_a(l, st) - evo.q_a(l, ref[l])) * ln
            tw_extra_S[l] = tw_extra_S.get(l, _ZERO) + (evo.q_a(l, st) + evo.q_a(l, ref[l])) * ln
        for (l, a, b, mt) in T.muts[X]:         # before the mutation the site was in `a`, not `b`
            dt = F(mt) - tP
            tw_extra[l] = tw_extra.get(l, _ZERO) + (evo.q_a(l, a) - evo.q_a(l, b)) * dt
            tw_extra_S[l] = tw_extra_S.get(l, _ZERO) + (evo.q_a(l, a) + evo.q_a(l, b)) * abs(dt)
            p = evo.pfs[l]
            beta_a[p][a] += nu[l] * dt; beta_a[p][b] -= nu[l] * dt
            beta_a_S[p][a] += nu[l] * abs(dt); beta_a_S[p][b] += nu[l] * abs(dt)
            muts_l[l] += 1; M[p, a, b] += 1; num_muts += 1
        for l, st in diff.items():
            p = evo.pfs[l]
            beta_a[p][st] += nu[l] * ln; beta_a[p][ref[l]] -= nu[l] * ln
            beta_a_S[p][st] += nu[l] * ln; beta_a_S[p][ref[l]] += nu[l] * ln

    _walk(T, ref, evo, visit)
    Tt, Tt_S, acc = [], [], _ZERO
    nmax_nodes = T.n
    for l in range(L):
        acc += miss_time[l]
        present = total - acc                   # time site l is not missing
        qa = evo.q_a(l, ref[l])
        v = qa * present + tw_extra.get(l, _ZERO)
        S = qa * (total + abs(acc)) + tw_extra_S.get(l, _ZERO)
        Tt.append(Exact(v, S, nmax_nodes + 4))
    # the ref-state default of Ttwiddle_beta_a: every not-missing site of beta, at its ref state, along every branch
    acc = _ZERO
    for l in range(L):
        acc += miss_time[l]
        p = evo.pfs[l]
        beta_a[p][ref[l]] += nu[l] * (total - acc)
        beta_a_S[p][ref[l]] += nu[l] * (total + abs(acc))
    Tba = [[Exact(beta_a[p][a], beta_a_S[p][a], L + 2 * T.n + 8) for a in range(4)] for p in range(P)]
    return dict(T=Exact(total, total, T.n), Ttwiddle_l=Tt, Ttwiddle_beta_a=Tba, num_muts_l=np.array(muts_l, np.int64),
                num_muts_beta_ab=M, num_muts=num_muts)


def add_stats(a, b):
    """Statistics of two disjoint sets of branches together (the parts of one tree)."""
    def add(x, y):
        return Exact(x.value + y.value, x.S + y.S, max(x.n, y.n) + 1)
    P = len(a["Ttwiddle_beta_a"])
    return dict(T=add(a["T"], b["T"]), Ttwiddle_l=[add(x, y) for x, y in zip(a["Ttwiddle_l"], b["Ttwiddle_l"])],
                Ttwiddle_beta_a=[[add(a["Ttwiddle_beta_a"][p][s], b["Ttwiddle_beta_a"][p][s]) for s in range(4)] for p in range(P)],
                num_muts_l=a["num_muts_l"] + b["num_muts_l"], num_muts_beta_ab=a["num_muts_beta_ab"] + b["num_muts_beta_ab"], num_muts=a["num_muts"] + b["num_muts"])


# ---- coalescent grids -----------------------------------------------------------------------------------------------
def _floor(x: F) -> int:
    return x.numerator // x.denominator


def _lineage_intervals(T: _Tree):
    return [(T.t[T.parent[X]], T.t[X]) for X in range(T.n) if X != T.root]


def _grid(intervals, cell_of, lb_of, ub_of, c0, c1, t_step, bound_mag):
    """k_bar over the cells c0..c1: (1/t_step) x the time-integral of the number of lineages in each cell, with per cell
    the S of the float64 accumulation and its number of additions."""
    ncell = c1 - c0 + 1
    part = [_ZERO] * ncell
    S = [_ZERO] * ncell
    cnt = [0] * ncell
    full = [0] * (ncell + 1)
    for lo, hi in intervals:
        if hi <= lo:
            continue
        a, b = cell_of(lo), cell_of(hi)          # cell index grows with time when the grid runs forward, and the other way
        ca, cb = min(a, b), max(a, b)
        for c in sorted({ca, ca + 1, cb - 1, cb}):
            if not ca <= c <= cb or not c0 <= c <= c1:
                continue
            i = c - c0
            # an end of the interval on or next to this cell: a float64 evaluation takes its share from a computed bound
            S[i] += bound_mag(c) / t_step
            cnt[i] += 1
            if ca < c < cb:
                continue
            clo, chi = max(lo, lb_of(c)), min(hi, ub_of(c))
            if chi <= clo:
                continue
            part[i] += (chi - clo) / t_step
            S[i] += (chi - clo) / t_step
        flo, fhi = max(ca + 1, c0), min(cb, c1 + 1)      # the cells it crosses whole, within c0..c1
        if flo < fhi:
            full[flo - c0] += 1; full[fhi - c0] -= 1
    run = 0
    kb = []
    for i in range(ncell):
        run += full[i]
        kb.append(part[i] + run)
        S[i] += run
        cnt[i] += run
    return kb, S, cnt


def k_bar_p(tree, includes_tree_root, t_ref, t_step, num_cells):
    """The part's lineage count per cell of the very-scalable grid (cell i = [t_ref - (i+1) t_step, t_ref - i t_step]),
    time-averaged; the part holding the tree's root also has the lineage above its root, down to the end of the grid
    (very_scalable_coalescent.cpp:14-79, 123-127)."""
    T = tree if isinstance(tree, _Tree) else _Tree(tree)
    tr, ts = _fl(t_ref), _fl(t_step)
    iv = _lineage_intervals(T)
    if includes_tree_root:
        iv.append((tr - num_cells * ts, T.t[T.root]))
    return _grid(iv, lambda t: _floor((tr - t) / ts), lambda c: tr - (c + 1) * ts, lambda c: tr - c * ts, 0, num_cells - 1, ts,
                 lambda c: abs(tr) + abs((c + 1) * ts))


def popsize_bar_vsc(pop: Pop, t_ref, t_step, cell) -> Exact:
    """pop_integral over cell `cell` of the very-scalable grid / t_step, on the exact cell bounds (kept per model: the parts of
    one grid share their cells)."""
    key = (float(t_ref), float(t_step), int(cell))
    if key not in pop.popsize_bar_cache:
        pop.popsize_bar_cache[key] = _popsize_bar_vsc(pop, t_ref, t_step, cell)
    return pop.popsize_bar_cache[key]


def _popsize_bar_vsc(pop: Pop, t_ref, t_step, cell) -> Exact:
    tr, ts = _fl(t_ref), _fl(t_step)
    lo, hi = tr - (cell + 1) * ts, tr - cell * ts
    I = pop.pop_integral(lo, hi)
    # a bound off by d moves the integral by N(bound) d
    Nmax = max(pop.pop_at_time(lo).value, pop.pop_at_time(hi).value)
    return Exact(I.value / ts, (I.S + Nmax * 2 * (abs(tr) + abs((cell + 1) * ts))) / ts, I.n + 4)


def partial_log_prior(tree, pop: Pop, includes_tree_root, tables) -> Exact:
    """Very_scalable_coalescent_prior_part::calc_partial_log_prior (very_scalable_coalescent.cpp:355-386) of a part, on the
    shared tables it holds (k_twiddle_bar_p, k_twiddle_bar, popsize_bar, num_active_parts as given) and its own k_bar_p
    computed exactly from its tree."""
    T = tree if isinstance(tree, _Tree) else _Tree(tree)
    n = len(tables["k_bar_p"])
    kb, kS, kn = k_bar_p(T, includes_tree_root, tables["t_ref"], tables["t_step"], n)
    ts = _fl(tables["t_step"])
    v, S, nmax = _ZERO, _ZERO, 0
    for i in range(n):
        k = kb[i]
        if k == 0:
            continue
        A = int(tables["num_active_parts"][i])
        assert A > 0, "cell %d: the part has lineages there but the table says %d active parts" % (i, A)
        pb, ktp, kt = _fl(tables["popsize_bar"][i]), _fl(tables["k_twiddle_bar_p"][i]), _fl(tables["k_twiddle_bar"][i])
        c = ktp * A - kt + F(1, 2)
        w = ts / pb
        v -= w * (F(1, 2) * k * k * A - c * k)
        S += w * (F(1, 2) * k * k * A + (abs(ktp * A) + abs(kt) + F(1, 2)) * abs(k)) + abs(w * (k * A - c)) * kS[i]
        nmax = max(nmax, kn[i])
    ninner = 0
    for X in range(T.n):
        if T.kids[X]:
            a, b = pop.neg_log_pop(T.t[X])
            v += a; S += b; ninner += 1
    return Exact(v, S, 4 * n + ninner + nmax)


class ExactDelta(Exact):
    """An Exact difference between two states.  `cells` = {cell: (k_bar_p before, after)} of the grid cells that differ and
    `k_sensitivity` = the sum over them of |d term / d k_bar_p| = |w (k A - c)| at the larger of the two (what an error of the
    engine's MAINTAINED k_bar_p, on which it evaluates the prior, is multiplied by); `branches` = the branches that differ."""
    __slots__ = ("cells", "k_sensitivity", "branches", "root_prior_differs")

    def __init__(self, value, S, n):
        Exact.__init__(self, value, S, n)
        self.cells, self.k_sensitivity, self.branches, self.root_prior_differs = {}, _ZERO, [], False


def _part_intervals(T: _Tree, includes_tree_root, tr, ts, num_cells):
    iv = _lineage_intervals(T)
    if includes_tree_root:
        iv.append((tr - num_cells * ts, T.t[T.root]))
    return iv


def partial_log_prior_delta(before, after, pop: Pop, includes_tree_root, tables) -> ExactDelta:
    """partial_log_prior(after) - partial_log_prior(before), both on `tables` (those read AFTER the move: cells the root part's
    grid appended during it hold the same lineage above the root in both trees, or differ and are counted), over the cells
    whose exact k_bar_p differs and the inner nodes whose time differs.  Per cell and node the S of partial_log_prior's rule,
    before plus after."""
    from collections import Counter
    B = before if isinstance(before, _Tree) else _Tree(before)
    A = after if isinstance(after, _Tree) else _Tree(after)
    assert A.n == B.n
    n = len(tables["k_bar_p"])
    tr, ts = _fl(tables["t_ref"]), _fl(tables["t_step"])
    ivB, ivA = _part_intervals(B, includes_tree_root, tr, ts, n), _part_intervals(A, includes_tree_root, tr, ts, n)
    cB, cA = Counter(ivB), Counter(ivA)
    changed = list((cB - cA).keys()) + list((cA - cB).keys())
    out = ExactDelta(_ZERO, _ZERO, 0)
    v, S, nterms, nmax = _ZERO, _ZERO, 0, 0
    if changed:
        cell_of = lambda t: _floor((tr - t) / ts)
        lb_of, ub_of = (lambda c: tr - (c + 1) * ts), (lambda c: tr - c * ts)
        ends = [cell_of(t) for iv in changed for t in iv]
        c0, c1 = max(0, min(ends)), min(n - 1, max(ends))
        tlo, thi = lb_of(c1), ub_of(c0)
        mag = lambda c: abs(tr) + abs((c + 1) * ts)
        near = lambda ivs: [(lo, hi) for lo, hi in ivs if hi >= tlo and lo <= thi]
        kB, SB, nB = _grid(near(ivB), cell_of, lb_of, ub_of, c0, c1, ts, mag)
        kA, SA, nA = _grid(near(ivA), cell_of, lb_of, ub_of, c0, c1, ts, mag)
        for j, i in enumerate(range(c0, c1 + 1)):
            if kB[j] == kA[j]:
                continue
            out.cells[i] = (kB[j], kA[j])
            Ap = int(tables["num_active_parts"][i])
            assert Ap > 0, "cell %d: the part has lineages there but the table says %d active parts" % (i, Ap)
            pb, ktp, kt = _fl(tables["popsize_bar"][i]), _fl(tables["k_twiddle_bar_p"][i]), _fl(tables["k_twiddle_bar"][i])
            c = ktp * Ap - kt + F(1, 2)
            w = ts / pb
            sens = _ZERO
            for sign, k, kS in ((-1, kB[j], SB[j]), (1, kA[j], SA[j])):
                v -= sign * w * (F(1, 2) * k * k * Ap - c * k)
                s1 = abs(w * (k * Ap - c))
                S += w * (F(1, 2) * k * k * Ap + (abs(ktp * Ap) + abs(kt) + F(1, 2)) * abs(k)) + s1 * kS
                sens = max(sens, s1)
            out.k_sensitivity += sens
            nterms += 8
            nmax = max(nmax, nB[j], nA[j])
    for X in range(A.n):
        if A.kids[X] and A.t[X] != B.t[X]:
            a, sa = pop.neg_log_pop(A.t[X])
            b, sb = pop.neg_log_pop(B.t[X])
            v += a - b; S += sa + sb; nterms += 2
    out.value, out.S, out.n = v, S, nterms + nmax
    return out


def part_log_G_delta(before, after, ref, evo: Evo, includes_run_root) -> ExactDelta:
    """part_log_G(after) - part_log_G(before) over the branches whose parent, end times, mutations or lambda differ, and the
    root prior when the root's state counts do.  `before` / `after`: trees, or the `Derived` of them."""
    DB = before if isinstance(before, Derived) else Derived(before, ref, evo)
    DA = after if isinstance(after, Derived) else Derived(after, ref, evo)
    B, A = DB.T, DA.T
    assert A.n == B.n
    out = ExactDelta(_ZERO, _ZERO, 0)
    v, S, n, nl = _ZERO, _ZERO, 0, 0
    for X in range(A.n):
        inB, inA = X != B.root, X != A.root
        if inB and inA and B.parent[X] == A.parent[X] and B.t[X] == A.t[X] and B.t[B.parent[X]] == A.t[A.parent[X]] \
                and DB.lam[X] == DA.lam[X] and B.muts[X] == A.muts[X]:
            continue
        if not inB and not inA:
            continue
        out.branches.append(X)
        if inA:
            a, b, c = DA.branch_log_G(X); v += a; S += b; n += c; nl = max(nl, DA.lam_n[X])
        if inB:
            a, b, c = DB.branch_log_G(X); v -= a; S += b; n += c; nl = max(nl, DB.lam_n[X])
    if includes_run_root and (DB.root_state_counts() != DA.root_state_counts()):
        rB, rA = DB.log_root_prior(), DA.log_root_prior()
        assert isinstance(rB.value, F) and isinstance(rA.value, F), "a root state of prior probability 0"
        v += rA.value - rB.value; S += rA.S + rB.S; n += rA.n + rB.n
        out.root_prior_differs = True
    out.value, out.S, out.n = v, S, n + nl
    return out


def displacement_slope(dv: "Derived", node) -> F:
    """d log G / d t of one node's time inside the window its neighbouring mutations leave it, from the definitions: the branch
    above it lengthens at -lambda(node); each child's branch shortens at the rate just below the node, which is the node's
    rate less what the child's missing intervals take away (every newly missing site at the state it had at the node)."""
    T, evo, ref, cum = dv.T, dv.evo, dv.ref, dv.cum
    d = _ZERO if node == T.root else -dv.lam[node]
    for c in T.kids[node]:
        below = dv.lam[node]
        for s, e in T.miss[c]:
            below -= cum[e] - cum[s]
        for l, st in T.mfs[c].items():
            below -= evo.rate(l, st) - evo.rate(l, ref[l])
        d += below
    return d


def scalable_log_prior(tree, pop: Pop, t_ref, t_step) -> Exact:
    """Scalable_coalescent_prior::calc_log_prior (scalable_coalescent.cpp:163-187) of a whole tree: cells
    [t_ref + c t_step, t_ref + (c+1) t_step], k_bar the time-averaged lineage count (1 before the root), popsize_bar the
    cell's pop_integral / t_step; -sum t_step k_bar (k_bar - 1) / (2 popsize_bar) - sum over inner nodes of log N(t)."""
    T = tree if isinstance(tree, _Tree) else _Tree(tree)
    tr, ts = _fl(t_ref), _fl(t_step)
    cell = lambda t: _floor((t - tr) / ts)
    c0, c1 = cell(T.t[T.root]), cell(max(T.t))
    iv = _lineage_intervals(T) + [(tr + c0 * ts, T.t[T.root])]
    kb, kS, kn = _grid(iv, cell, lambda c: tr + c * ts, lambda c: tr + (c + 1) * ts, c0, c1, ts, lambda c: abs(tr) + abs((c + 1) * ts))
    v, S, nmax = _ZERO, _ZERO, 0
    for i, c in enumerate(range(c0, c1 + 1)):
        k = kb[i]
        if k == 0 or k == 1:
            continue
        lo, hi = tr + c * ts, tr + (c + 1) * ts
        I = pop.pop_integral(lo, hi)
        Nmax = max(pop.pop_at_time(lo).value, pop.pop_at_time(hi).value)
        pS = I.S + Nmax * 2 * (abs(tr) + abs((c + 1) * ts))
        term = ts * ts * k * (k - 1) / (2 * I.value)
        v -= term
        S += abs(term) * (1 + pS / I.value) + abs(ts * ts * (2 * k - 1) / (2 * I.value)) * kS[i]
        nmax = max(nmax, kn[i] + I.n)
    ninner = 0
    for X in range(T.n):
        if T.kids[X]:
            a, b = pop.neg_log_pop(T.t[X])
            v += a; S += b; ninner += 1
    return Exact(v, S, 4 * (c1 - c0 + 1) + ninner + nmax)


def adversarial_pop_cases():
    """(name, PopModel, a[], b[]) on the edges where population code goes wrong: g dt from 0 (zero-length intervals) through
    1e-12 to 50 with both signs of g; intervals straddling, starting on and ending on the minimum-population crossover t_c, and
    on either side of it; uneven skygrid knots with points on, beside and beyond them, adjacent gammas equal and 1e-12 apart,
    stepwise and log-linear."""
    from delphy_amd.engine import PopModel
    out = []
    t0 = 100.0
    dts = np.concatenate([[0.0], 10.0 ** np.linspace(-12, math.log10(50.0), 40)])
    for g in (0.37, -0.37, 1e-3, -2.5):
        dt = dts / abs(g)
        a = np.concatenate([t0 - 0.5 * dt, np.full(dt.shape, t0 + 3.0)])
        out.append(("exp g=%g" % g, PopModel.exp(t0, 50.0, g, 0.0), a, np.concatenate([t0 + 0.5 * dt, t0 + 3.0 + dt])))
    for g in (0.37, -0.37):
        pm = PopModel.exp(t0, 50.0, g, 7.0)
        tc = float(Pop(pm).t_c)
        w = np.concatenate([[0.0], 10.0 ** np.linspace(-12, 1.5, 25)])
        a = np.concatenate([tc - w, np.full(w.shape, tc), tc - w, tc - 2 * w - 1.0, tc + w + 0.5])
        b = np.concatenate([tc + w, tc + w, np.full(w.shape, tc), tc - w - 1.0, tc + 2 * w + 0.5])
        out.append(("exp g=%g min_pop" % g, pm, a, b))
    x = np.array([0.0, 0.5, 3.0, 3.1, 10.0, 40.0, 41.0])
    gam = np.array([2.0, 2.0, 5.5, 5.5 + 1e-12, 1.0, 1.0 - 1e-12, 3.0])
    pts = np.concatenate([x, x - 1e-9, x + 1e-9, [-50.0, -1.0, 45.0, 400.0], np.linspace(-2.0, 43.0, 37)])
    lo, hi = np.meshgrid(pts, pts)
    keep = lo <= hi
    for log_linear in (False, True):
        out.append(("skygrid %s" % ("log-linear" if log_linear else "stepwise"), PopModel.skygrid(x, gam, log_linear), lo[keep], hi[keep]))
    return out
