"""The exact model of ONE graft: what analyze_graft / propose_new_graft hand a topology move, restated per site from the
definitions -- a third party for the HIP engine (emat_device_spr.hpp) and the CPU oracle (oracle/orc_spr.hpp), which restate
the reference's interval-set algebra in the same order and so can share a mistake.

Nothing here calls the oracle or the engine and nothing here is an interval set: every set of sites is a boolean array over
the sites, every number a Fraction (exact_model's arithmetic), every quantity an `Exact` (value, S, n).

Base quantities of a part's tree:
- missing_at[Y][l]: site l lies in a missing interval of a node on the path from the part's root to Y;
- informative[tip][l] = not missing_at[tip][l];  data[Y][l]: some tip below Y is informative at l.

Inner graft of X (its parent P is not the part's root).  phi_0 = X, phi_{i+1} = parent(phi_i), sib_i the other child of
phi_{i+1}.  warm_0 = every site; warm_{i+1} = warm_i & ~data[sib_i] & data[X]; hot_i = warm_i & ~warm_{i+1}.  Info i runs from
A = phi_{i+1} down to X, B = phi_i.  The path stops where nothing is warm any more; when it reaches the part's root it ends
closed there in a part that does not hold the run's root (everything still warm is hot), and otherwise whatever is still warm
above the root is the open info (A = none, B = root, as long as X is below the root).
Rooty graft of X (P is the run's root, S its other child): info 0, open, P -> X on the sites only X's side has data for; info
1, open, P -> S on the sites only S's side has; info 2, closed, S -> P -> X on the sites both have, T = (t_X - t_P) + (t_S - t_P),
its mutations on P -> S reversed and reflected about t_P.

Per info: hot_muts_to_X = the mutations on the branches from A down to X at hot sites, top branch first, each branch in stored
order; hot_deltas_to_X their net change per site (closed infos); partial_lambda_at_X / _at_A = the sum over the hot sites
informative at X (for P -> S: at S) of mu nu_l q_l(state there).  delta_log_G = the sum over the infos of the branch log G
(exact_model.Derived.branch_log_G's definition: -lambda_end T - sum (r_from - r_to)(t_m - t_A) + sum log(mu nu Q_from,to)) plus
log(pi_from / pi_to) for every mutation that changes the run's root state (open infos; for the rooty graft also the P -> S part of
the closed path, whose start S is held fixed).  log_alpha_mut(mu) = sum_i [-mu L_i T_i + M_i log(mu / 3)] - for every closed info
[(L_i - d_i) log P_AA + d_i log P_AC], P_AC = -expm1(-4/3 mu T_i) / 4, P_AA = 1 - 3 P_AC, L_i = hot sites informative at X,
M_i = hot mutations, d_i = hot deltas.

S and n (exact_model's rules; one graft's numbers are formed whole, so S is the full sum of the terms):
- T_to_X = t_X - t_A is one difference of stored times: S = |T|, n = 1; the rooty closed path's is a sum of two: S = both, n = 3;
- a partial lambda is formed from prefix sums of the reference sequence's rates, one difference per interval of sites (S: both
  prefix sums, per maximal run of the set), one correction per site whose state is not the reference's (S: both rates) and one
  per mutation walked (S: both rates); where the code takes it from a node's whole lambda less another partial lambda (the inner
  graft's info 0, and level i's as the set that slid in less the set that slides on; the rooty closed path) it carries those S;
- a branch log G carries lambda's S times |T|; a mutation's (r_from + r_to) times the magnitude of its time offset -- the code
  re-derives the branch's start as t_X - T_to_X, so |t_X| + |T| + |t_m - t_A|; a reflected time 2 |t_P| more -- and
  |log rate| + 3;
- log(pi_from / pi_to) counts |log| + 1;
- -mu L T counts its magnitude; M log(mu/3) counts M (|log(mu/3)| + 1); P_AC counts P_AC (1 + |x|), x = -4/3 mu T;
  d log P_AC counts d (|log P_AC| + 1 + (1 + |x|)); (L - d) log P_AA counts (L - d)(|log P_AA| + 1 + 3 P_AC (1 + |x|) / P_AA).

Reference lines of the definitions: core/spr_move.h:28-150 (the header's words), core/spr_move.cpp:91-316, 582-836;
SURVEY.md a13.
"""
from fractions import Fraction as F

import numpy as np

import exact_model as X
from exact_model import Exact

_Z = F(0)


def _runs(mask):
    """[(s, e)] of the maximal runs of a boolean array."""
    m = np.concatenate([[False], mask, [False]])
    d = np.flatnonzero(m[1:] != m[:-1])
    return list(zip(d[0::2].tolist(), d[1::2].tolist()))


class Info:
    __slots__ = ("A", "B", "is_open", "warm", "hot", "muts", "reflected", "deltas", "T", "lam_A", "lam_X", "L", "M", "d")


class Graft:
    """One graft of the model: X, S, t_P, infos, delta_log_G (Exact) and log_alpha_mut(mu) (Exact)."""

    def __init__(self, X_, S_, t_P, infos, dlg, rooty):
        self.X, self.S, self.t_P, self.infos, self.delta_log_G, self.rooty = X_, S_, t_P, infos, dlg, rooty
        self._lam = {}

    def log_alpha_mut(self, mu) -> Exact:
        """`mu`: a float64 handed to the engine, or an exact rate (a Fraction) the engine computes itself; then `mu_sensitivity`
        says what that computation's own error may add."""
        return self._log_alpha_mut(mu)[0]

    def mu_sensitivity(self, mu):
        """The sum over log_alpha_mut's terms of |d term / d mu|: an error e of mu moves log_alpha_mut by at most this times e, to
        first order.  A caller that takes mu from another computed quantity (value, S, n) adds (n + 8) u S times this to the bound
        instead of widening every term of log_alpha_mut by that quantity's n."""
        return self._log_alpha_mut(mu)[1]

    def _log_alpha_mut(self, mu):
        key = mu
        if key in self._lam:
            return self._lam[key]
        m = mu if isinstance(mu, F) else F(float(mu))
        lg3 = X._log(m / 3)
        v, S, n, sens = _Z, _Z, 0, _Z
        for b in self.infos:
            T = b.T.value
            v += -m * b.L * T + b.M * lg3
            S += m * b.L * abs(T) + b.M * (abs(lg3) + 1)
            sens += b.L * abs(T) + b.M / m
            n += 4
            if not b.is_open:
                x = -F(4, 3) * m * T
                pac = -X._expm1(x) / 4
                paa = 1 - 3 * pac
                dpac = abs(T) / 3 * (1 - 4 * pac)           # d P_AC / d mu = (T / 3) exp(x)
                if b.L - b.d:
                    l1 = X._log(paa)
                    v -= (b.L - b.d) * l1
                    S += (b.L - b.d) * (abs(l1) + 1 + 3 * pac * (1 + abs(x)) / paa)
                    sens += (b.L - b.d) * 3 * dpac / paa
                if b.d:
                    l2 = X._log(pac)
                    v -= b.d * l2
                    S += b.d * (abs(l2) + 1 + (1 + abs(x)))
                    sens += b.d * dpac / pac
                n += 8
        self._lam[key] = (Exact(v, S, n), sens)
        return self._lam[key]


class GraftModel:
    """The grafts of one part's tree.  `tree`: a FlatTree; `ref`: the reference sequence; `evo`: exact_model.Evo;
    `includes_run_root`: the part holds the run's root (its root may change, paths may end in the open branch above it)."""

    def __init__(self, tree, ref, evo: X.Evo, includes_run_root):
        self.dv = tree if isinstance(tree, X.Derived) else X.Derived(tree, ref, evo)       # (a tree, or the Derived of it)
        self.T = self.dv.T
        self.ref = np.asarray(ref, np.int64)
        self.evo, self.incl = evo, bool(includes_run_root)
        self.L = len(self.ref)
        self.cum = self.dv.cum
        self._missing, self._data, self._seq, self._grafts = {}, {}, {}, {}

    # ---- the base quantities, for the nodes a graft asks about -------------------------------------------------------------
    def missing_at(self, Y):
        T, todo = self.T, []
        while Y >= 0 and Y not in self._missing:
            todo.append(Y); Y = T.parent[Y]
        for Y in reversed(todo):
            m = np.zeros(self.L, bool) if Y == T.root else self._missing[T.parent[Y]].copy()
            for s, e in T.miss[Y]:
                m[s:e] = True
            self._missing[Y] = m
        return self._missing[todo[0]] if todo else self._missing[Y]

    def data(self, Y):
        T = self.T
        if Y not in self._data:
            post, st = [], [Y]
            while st:
                v = st.pop()
                if v not in self._data:
                    post.append(v); st += T.kids[v]
            for v in reversed(post):
                self._data[v] = ~self.missing_at(v) if not T.kids[v] else self._data[T.kids[v][0]] | self._data[T.kids[v][1]]
                # the tree holds a missing interval at the highest node below which no tip has data (the builder's and the moves'
                # own factoring): "missing at v" and "no data below v" are the same set
                assert np.array_equal(self._data[v], ~self.missing_at(v)), "node %d: missing intervals not factored up to it" % v
        return self._data[Y]

    # ---- states and rates ------------------------------------------------------------------------------------------------
    def seq_at(self, Y):
        """The state of every site at node Y as the path's mutations give it (meaningful where Y is not missing)."""
        s = self._seq.get(Y)
        if s is None:
            T = self.T
            s = self.ref.copy() if Y == T.root else self.seq_at(T.parent[Y]).copy()
            for (l, a, b, _) in T.muts[Y]:
                s[l] = b
            self._seq[Y] = s
        return s

    def sibling(self, Y):
        a, b = self.T.kids[self.T.parent[Y]]
        return b if a == Y else a

    def _pl(self, mask, seq):
        """(sum over the sites of `mask` of rate(l, seq[l]), S, n) by the partial-lambda rule of the docstring."""
        cum, evo, ref = self.cum, self.evo, self.ref
        v, S, n = _Z, _Z, 0
        for s, e in _runs(mask):
            v += cum[e] - cum[s]; S += cum[e] + cum[s]; n += 2
        for l in np.flatnonzero(mask & (seq != ref)).tolist():
            ra, rb = evo.rate(l, int(seq[l])), evo.rate(l, int(ref[l]))
            v += ra - rb; S += ra + rb; n += 2
        return v, S, n

    def _mut_S(self, muts):
        return sum((self.evo.rate(l, a) + self.evo.rate(l, b) for (a, l, b, _) in muts), _Z)

    def _branch(self, lam: Exact, t_A, t_X, T: Exact, muts, reflected=()):
        """(value, S, n) of one info's branch log G: rate lam at the end, start t_A (a Fraction), mutations [from, site, to, t]."""
        evo = self.evo
        v = -lam.value * T.value
        S = lam.S * abs(T.value)
        n = 1 + lam.n
        for k, (a, l, b, mt) in enumerate(muts):
            ra, rb = evo.rate(l, a), evo.rate(l, b)
            dt = (mt if isinstance(mt, F) else F(mt)) - t_A
            lg = evo.log_rate_ab(l, a, b)
            v += -(ra - rb) * dt + lg
            S += (ra + rb) * (abs(t_X) + abs(T.value) + abs(dt) + (2 * abs(t_A) if k in reflected else 0)) + abs(lg) + 3
            n += 2
        return v, S, n

    def _pi_ratio(self, muts):
        v, S, n = _Z, _Z, 0
        for (a, l, b, _) in muts:
            p = self.evo.pfs[l]
            lg = X._log(F(float(self.evo.pi[p, a])) / F(float(self.evo.pi[p, b])))
            v += lg; S += abs(lg) + 1; n += 2
        return v, S, n

    @staticmethod
    def _deltas(muts):
        first, last = {}, {}
        for (a, l, b, _) in muts:
            first.setdefault(l, a); last[l] = b
        return [[l, first[l], last[l]] for l in sorted(first) if first[l] != last[l]]

    # ---- the graft -------------------------------------------------------------------------------------------------------
    def can_analyse(self, Xn):
        """What the move code analyses: not the root, and not a child of the root of a part that is not the run's
        (spr_move_core returns before the analysis there)."""
        T = self.T
        return Xn != T.root and (self.incl or T.parent[Xn] != T.root)

    def graft(self, Xn) -> Graft:
        T = self.T
        assert self.can_analyse(Xn)
        g = self._grafts.get(Xn)
        if g is None:
            g = self._grafts[Xn] = self._rooty(Xn) if T.parent[Xn] == T.root else self._inner(Xn)
        return g

    def _on_branch(self, Y, mask):
        return [(a, l, b, t) for (l, a, b, t) in self.T.muts[Y] if mask[l]]

    def _inner(self, Xn) -> Graft:
        T, dv = self.T, self.dv
        inf_X = ~self.missing_at(Xn)
        path = [Xn]
        while path[-1] != T.root:
            path.append(T.parent[path[-1]])
        tX = T.t[Xn]
        warm = np.ones(self.L, bool)
        infos, i = [], 0
        while True:
            b = Info()
            b.A, b.B, b.is_open, b.warm = path[i + 1], path[i], False, warm
            nxt = warm & ~self.data(self.sibling(path[i])) & self.data(Xn)
            at_root = path[i + 1] == T.root
            if at_root and not self.incl:
                nxt = np.zeros(self.L, bool)                # ends closed at the part's root: everything still warm is hot
            b.hot = warm & ~nxt
            infos.append(b)
            warm = nxt
            if not warm.any():
                break
            if at_root:
                o = Info()
                o.A, o.B, o.is_open, o.warm, o.hot = -1, T.root, True, warm, warm
                infos.append(o)
                break
            i += 1
        v, S, n = _Z, _Z, 0
        for j, b in enumerate(infos):
            top = len(path) - 2 if b.is_open else j         # the highest branch of the path whose mutations it owns
            b.muts = [m for k in range(top, -1, -1) for m in self._on_branch(path[k], b.hot)]
            b.reflected = ()
            b.deltas = [] if b.is_open else self._deltas(b.muts)
            A = T.root if b.is_open else b.A
            b.T = Exact(tX - T.t[A], abs(tX - T.t[A]), 1)
            own = b.hot & inf_X
            la, sa, na = self._pl(own, self.seq_at(A))
            lx, sx, nx = self._pl(own, self.seq_at(Xn))
            # how the code comes by it: what slid in less what slides on, each a set of intervals at the states at A, plus the walk
            # over the mutations of B; level 0 from X's whole lambda
            if j == 0:
                extra_S, extra_n = dv.lam_S[Xn] + self._mut_S(self._on_branch(Xn, np.ones(self.L, bool))), dv.lam_n[Xn] + 2 * len(T.muts[Xn])
            else:
                _, s_in, n_in = self._pl(b.warm, self.seq_at(A))
                extra_S, extra_n = s_in + self._mut_S(self._on_branch(b.B, b.warm)), n_in + 2 * len(T.muts[b.B])
            if j + 1 < len(infos) and not b.is_open:
                _, s_on, n_on = self._pl(infos[j + 1].warm, self.seq_at(A))
                extra_S += s_on; extra_n += n_on
            b.lam_A = Exact(la, sa + extra_S, na + extra_n)
            b.lam_X = Exact(lx, sx + b.lam_A.S + self._mut_S(b.muts), nx + b.lam_A.n + 2 * len(b.muts))
            b.L, b.M, b.d = int(own.sum()), len(b.muts), len(b.deltas)
            bv, bS, bn = self._branch(b.lam_X, T.t[A], tX, b.T, b.muts)
            v += bv; S += bS; n += bn
            if b.is_open:
                pv, pS, pn = self._pi_ratio(b.muts)
                v += pv; S += pS; n += pn
        return Graft(Xn, self.sibling(Xn), float(T.t[T.parent[Xn]]), infos, Exact(v, S, n), False)

    def _rooty(self, Xn) -> Graft:
        T, dv = self.T, self.dv
        P, Sn = T.root, self.sibling(Xn)
        tP, tX, tS = T.t[P], T.t[Xn], T.t[Sn]
        dX, dS = self.data(Xn), self.data(Sn)
        every = np.ones(self.L, bool)
        rseq, xseq, sseq = self.seq_at(P), self.seq_at(Xn), self.seq_at(Sn)

        px = Info()
        px.A, px.B, px.is_open = P, Xn, True
        px.warm = px.hot = dX & ~dS
        px.muts, px.reflected, px.deltas = self._on_branch(Xn, px.hot), (), []
        px.T = Exact(tX - tP, abs(tX - tP), 1)
        la, sa, na = self._pl(px.hot, rseq)
        lx, _, _ = self._pl(px.hot, xseq)
        px.lam_A = Exact(la, sa, na)
        px.lam_X = Exact(lx, sa + self._mut_S(px.muts), na + 2 * len(px.muts))

        ps = Info()
        ps.A, ps.B, ps.is_open = P, Sn, True
        ps.warm = ps.hot = dS & ~dX
        ps.muts, ps.reflected, ps.deltas = self._on_branch(Sn, ps.hot), (), []
        ps.T = Exact(tS - tP, abs(tS - tP), 1)
        la, sa, na = self._pl(ps.hot, rseq)
        lx, _, _ = self._pl(ps.hot, sseq)
        ps.lam_A = Exact(la, sa, na)
        ps.lam_X = Exact(lx, sa + self._mut_S(ps.muts), na + 2 * len(ps.muts))

        c = Info()
        c.A, c.B, c.is_open = Sn, P, False
        c.warm = c.hot = dS & dX
        on_PS = self._on_branch(Sn, c.hot)                                      # as the tree holds them: root -> S
        on_PX = self._on_branch(Xn, c.hot)
        back = [(b, l, a, tP - (F(t) - tP)) for (a, l, b, t) in reversed(on_PS)]     # S -> root, times reflected about t_P
        c.muts = back + on_PX
        c.reflected = tuple(range(len(back)))
        c.deltas = self._deltas(c.muts)
        c.T = Exact((tS - tP) + (tX - tP), abs(tS - tP) + abs(tX - tP), 3)
        lx, sx, nx = self._pl(c.hot, xseq)
        la, sa, na = self._pl(c.hot, sseq)
        c.lam_X = Exact(lx, sx + dv.lam_S[Xn] + px.lam_X.S, nx + dv.lam_n[Xn] + px.lam_X.n)
        c.lam_A = Exact(la, sa + dv.lam_S[Sn] + ps.lam_X.S, na + dv.lam_n[Sn] + ps.lam_X.n)

        v, S, n = _Z, _Z, 0
        for lam, t_end, T_, muts in ((px.lam_X, tX, px.T, px.muts), (ps.lam_X, tS, ps.T, ps.muts),
                                     (c.lam_X, tX, px.T, on_PX), (c.lam_A, tS, ps.T, on_PS)):
            refl = range(len(muts)) if muts is on_PS else ()
            bv, bS, bn = self._branch(lam, tP, t_end, T_, muts, refl)
            v += bv; S += bS; n += bn
        for muts in (px.muts, ps.muts, on_PS):
            pv, pS, pn = self._pi_ratio(muts)
            v += pv; S += pS; n += pn
        for b in (px, ps, c):
            b.L, b.M, b.d = int(b.hot.sum()), len(b.muts), len(b.deltas)
        return Graft(Xn, Sn, float(tP), [px, ps, c], Exact(v, S, n), True)


# ---- an engine's graft against the model's ---------------------------------------------------------------------------------
def _mask(intervals, L):
    m = np.zeros(L, bool)
    prev = 0
    for s, e in intervals:
        assert prev <= s < e <= L, "interval list %s is not sorted and disjoint" % (intervals,)
        m[s:e] = True
        prev = e
    return m


def compare(tally, g, m: Graft, mu, L, where):
    """An engine's graft `g` (engine.decode_graft_output's dict) against the model's.  Sets and lists are asserted equal
    (failures into tally.fail), numbers go through tally.check.  Returns False when the structure differs (nothing further is
    compared then)."""
    fails = tally.fail
    n0 = len(fails)
    if (g["X"], g["S"]) != (m.X, m.S) or np.float64(g["t_P"]).tobytes() != np.float64(m.t_P).tobytes():
        fails.append("%s: X, S, t_P %s, the model says %s" % (where, (g["X"], g["S"], g["t_P"]), (m.X, m.S, m.t_P)))
    if len(g["branch_infos"]) != len(m.infos):
        fails.append("%s: %d branch infos, the model says %d" % (where, len(g["branch_infos"]), len(m.infos)))
        return False
    for i, (gb, b) in enumerate(zip(g["branch_infos"], m.infos)):
        w = "%s info %d" % (where, i)
        if (gb["A"], gb["B"], bool(gb["is_open"])) != (b.A, b.B, b.is_open):
            fails.append("%s: A, B, is_open %s, the model says %s" % (w, (gb["A"], gb["B"], gb["is_open"]), (b.A, b.B, b.is_open)))
        for f, want in (("warm_sites", b.warm), ("hot_sites", b.hot)):
            try:
                got = _mask(gb[f], L)
            except AssertionError as e:
                fails.append("%s: %s: %s" % (w, f, e)); continue
            if not np.array_equal(got, want):
                fails.append("%s: %s differs from the model's at sites %s" % (w, f, np.flatnonzero(got != want)[:12].tolist()))
        gm = gb["hot_muts_to_X"]
        if [x[:3] for x in gm] != [list(x[:3]) for x in b.muts]:
            fails.append("%s: hot_muts_to_X %s, the model says %s" % (w, [x[:3] for x in gm], [list(x[:3]) for x in b.muts]))
        else:
            tP = abs(m.t_P)
            for k, (x, y) in enumerate(zip(gm, b.muts)):
                if k in b.reflected:        # a time the code reflects about t_P (and the tree may hold reflected back): roundings of t_P -/+ (t - t_P)
                    if not abs(F(x[3]) - y[3]) <= 4 * X.U * (tP + abs(float(y[3]) - m.t_P)):
                        fails.append("%s: reflected time of hot mutation %d %r, the model says %r" % (w, k, x[3], float(y[3])))
                elif np.float64(x[3]).tobytes() != np.float64(y[3]).tobytes():
                    fails.append("%s: time of hot mutation %d %r, the model says %r" % (w, k, x[3], y[3]))
        if gb["hot_deltas_to_X"] != b.deltas:
            fails.append("%s: hot_deltas_to_X %s, the model says %s" % (w, gb["hot_deltas_to_X"], b.deltas))
        tally.check("T_to_X", b.T, gb["T_to_X"], w)
        tally.check("partial_lambda_at_A", b.lam_A, gb["partial_lambda_at_A"], w)
        tally.check("partial_lambda_at_X", b.lam_X, gb["partial_lambda_at_X"], w)
    tally.check("delta_log_G", m.delta_log_G, g["delta_log_G"], where)
    tally.check("log_alpha_mut", m.log_alpha_mut(mu), g["log_alpha_mut"], where)
    return len(fails) == n0
