"""What every local move DREW, held to the distribution its log MH assumes -- a third party for the HIP engine
(emat_device_moves.hpp; emat_device_core.hpp: uniform_pick, gaussian, uniform_oc; emat_device_spr.hpp: study_pick_time_in_region)
and the CPU oracle, which restate the reference's samplers by the same reading and so can share a mistake.

No statistics.  move_steps.step_chain hands check_step the part before and after every single move, the move's trace row and the
position of the part's random stream before and after it; the next word's index is 2 * counter - has_spare, and Philox and the
conversions of a word to a uniform are integer arithmetic (tests/skygrid_streams.py; test_rng_cursor_gpu.py pins the words).  So every
uniform a move consumed is known bit for bit, and a draw is held to the DEFINITION of its distribution by the probability integral
transform: the value written into the tree is the exact inverse CDF, of the exact distribution, at that uniform.  Nothing here calls
either engine; numbers are Fractions or 60-digit mpmath numbers.

The identities (u = 2^-53 below; to_co = (w >> 11) / 2^53, to_oo = (2 (w >> 12) + 1) / 2^53, to_oc = ((w >> 11) + 1) / 2^53):

Every move (subrun.cpp:98-121).  Word 0 through mix_total * to_co (32, or 30 with topology moves off) gives the kind, cuts at 7.5 / 15 /
30 / 31.  A node pick is floor(word n_nodes / 2^64), repeated while the pick is not acceptable (an inner node for the inner-node
displacement, subrun.cpp:150-153; a tip for the tip displacement, subrun.cpp:236-239; not the root for SPR1, after its chooser word,
subrun.cpp:497-503); the row's node is the first acceptable pick.  A branch reform picks once, and not at all when n_nodes < 3
(subrun.cpp:289-291); a slide picks once (subrun.cpp:354-358).

Words consumed.  position after - position before is what the model predicts, for every move that is not a topology move or a
`compound` reform; for those the history sampler inside propose_new_graft takes words the model does not state, and the leading words
and the last word are held.  Moves that end early, un-noted (row "not accepted", NaN), after exactly their leading words: an inner pick
of the part's root in a part without the run's root; an exact-date tip; a reform of the root; n_nodes < 3; a drawn time that landed on
a bound (no acceptance word); the root displacement outside [t_min, t_max]; the slide of the root, the slide with new_t_P > t_X, the
slide down without a straddling branch, a slide or SPR1 of a child of the part's root in a part without the run's root.  A reform of a
branch without mutations draws nothing and is accepted with log_mh 0.0.  An SPR1 whose drawn time equals t_X or an end of the new
branch (subrun.cpp:560-566) ends un-noted two words after its picks (the region's word and the time's).  A displacement of the run's
root that takes the coalescent grid past its last cell draws one Gaussian per appended cell (very_scalable_coalescent.cpp:259-299: two
words each, k_twiddle_bar_p = sqrt(popsize_bar / t_step) z, held like the step below) between the step's words and the verdict's.
No valid part has fewer than three nodes (the inner-node displacement's pick would never end), so that rule is stated and not
exercised.  A bounded exponential lands on a bound only where the window is a few doubles wide (|log v| <= 36.8 keeps the draw off b by
more than a rounding otherwise): test_move_steps.on_a_bound_scenario is such a window, and every tip displacement of its case ends that
way.  No SPR1 of any case draws a time that equals an end of its region; that early end has a counter of its own.

Acceptance (mh_accept).  A noted move with log_mh >= 0 is accepted and takes no word; with log_mh < 0 its LAST word through to_co is v
and the verdict is v < exp(log_mh), log_mh the row's own double, the exponential mpmath's.  Borderline only when |v - exp(log_mh)| <=
4 u exp(log_mh).

Bounded exponential (distributions.h:38-69; accepted tip displacement, accepted displacement of an inner node other than the run's
root).  v = to_oo(word), a = t_min, b = t_max as the move forms them from the tree before, lambda the exact slope
(exact_model.displacement_slope; minus the exact lambda_i for a tip), F(x) = expm1(lambda (x - a)) / expm1(lambda (b - a)), uniform when
lambda is 0, the result clamped to [a, b].  The new time is F^-1(v) for ltr = lambda (b - a) >= -100.  For ltr < -100 the reference
(distributions.h:56-57) returns a + log(v) / lambda, and log(v) / lambda is log(1 - v') / lambda at v' = 1 - v: the new time is F^-1(1 - v)
there.  to_oo's grid is symmetric about 1/2 (1 - (2k + 1) / 2^53 = (2 (2^52 - 1 - k) + 1) / 2^53), so 1 - v is the uniform of another word
of the same probability and the draw has the distribution all the same; the model states which of the two the move evaluates, and a
step whose exact ltr lies within 100 d' / |lambda| of -100, where the statement changes, is borderline.  (At +100 both spellings agree to the
dropped term, below.)  The engine's lambda differs from the exact one by at most d = (n + 8) u S of the slope (slope_exact: the node's
lambda three times, each child's missing intervals once); the product lambda (b - a) rounds twice more, so d' = d + 3 u |lambda|.  F^-1
is increasing in lambda, so the admissible interval is [F^-1(v; lambda - d'), F^-1(v; lambda + d')] widened by
- `ops`: u (2 max(|a|, |b|) + 6 |x - anchor|), anchor = b in the ltr > 100 spelling and a otherwise: the logarithm, the division and the
  final sum, at their magnitudes;
- `cancel` (|ltr| <= 100): the reference forms exp(ltr) - 1, relative error u (2 exp(ltr) / |expm1(ltr)| + 2) on y = v expm1(ltr), which
  moves log1p(y) / lambda by |y| / ((1 + y) |lambda|) times that;
- `drop` (|ltr| > 100): exp(-|ltr|) / (v |lambda|), what the short spellings leave out.
Where [lambda - d', lambda + d'] contains 0 the step passes if the time is the uniform draw a + v (b - a) to u (|a| + 2 |b - a| + |x|);
otherwise it is counted slope_sign_undetermined and only its words and verdict are held.

Gaussian step (gaussian: Box-Muller).  z = sqrt(-2 log u1) cos(2 pi u2), u1 = to_oc(word), u2 = to_co(next word).  Accepted root
displacement (subrun.cpp:196-207): new_t - old_t = sigma z, sigma = min(1 / (2 lambda_root), t_max_tip - t_max).  Accepted slide
(subrun.cpp:360-380): t_P after - t_P before = sigma z, sigma = min(1 / (2 lambda_X), t_max_tip - t_early), t_early = min(t_X, t_S)
under the part's root and the root's time otherwise.  sigma is decreasing in lambda, so it lies between its values at lambda -/+ its
Exact.bound(); the step is held to |sigma z| (3 u + the relative width of that interval) + 26 u sigma r + u |new time|, r = sqrt(-2 log
u1): the engine's 2 pi is a double (2 u of the angle, at most 2 pi), log, sqrt, cos and the two products round, the sum rounds at the
new time's magnitude.  The early ends above are decided by the same number: a step within that bound of the comparison is borderline.

Slide down past the sibling (subrun.cpp:325-350, 425-440).  The new sibling is element floor(word n / 2^64) of the branches below P
that straddle the new time, X's subtree left out, depth first, child0 first, on the tree before (straddling_branches: the one
derivation move_steps.slide_alpha_ratio's n comes from too).

Branch reform (phylo_tree.cpp:579-644; accepted, not compound).  Every mutation's new time is t_P + (t_X - t_P) to_oc(word_i) to
2 u (|t_P| + |t_X - t_P|) (the device may contract the multiply-add).  Sites all different: word i goes to the mutation that was i-th
before.  A site twice on the branch: sites in ascending order, each site's draws, sorted, to that site's mutations in their old order.
n words, plus one if log_mh < 0.

SPR1 (spr_study.cpp:424-471; accepted).  Words: the kind, the chooser (`Words` is the one reader of the stream: move_steps.scan_limit_from_stream reads the limit through it),
the picks, the region pick, then the time: below the root (t - t_min) / (t_max - t_min) = to_oc(word) to 2 u (|t_min| + |t_max - t_min|);
above it, s = t_X + t_S - 2 t, a = f m + 1: power law (s^a - s_min^a) / (s_max^a - s_min^a) = to_oo(word), s held to s u (16 + 4 (a |log
s_max| + a |log s_min| + |log v| / a)), v the bracket (the two powers, the sum at the larger one's magnitude, the rounded exponents a and
1 / a); gamma Q(a, beta s) = Q_lo + (Q_hi - Q_lo) to_oc(word), beta = f lambda_X, held in Q: three values of the project's own tolerance
for gamma_q / gamma_q_inv (1e-12 + 1e-9 Q, test_oracle_pinning.check_gamma_reference_cases) plus the density beta g(beta s) times the
error of s, plus lambda_X's bound through beta.  s and t are clamped to [s_min, s_max] and the region's times; both are then read
through t's rounding, 4 u (|t_X| + |t_S| + s) on s.  Region, a, beta, s_min, s_max are study_model.Study's.

Out of scope: which region the cumulative walk picks (it depends on the scan's order; the region's probability is held through
log_alpha); the draws of the mutational-history sampler (the reference's frequency test runs on 25 000 device histories, and
check_accepted_slide holds the density of the history written); the compound reform's inner spr_move_core.

A step is left out of an identity only as `borderline` (asserted 0), `slope_sign_undetermined` or `position_half_known`
(stream_position could not say whether half a block was pending: both readings are tried and exactly one must satisfy every identity).
"""
from fractions import Fraction as F

import mpmath
import numpy as np

import exact_model as X
import skygrid_streams as RS

U = F(1, 2 ** 53)
_mp = X._mp
mp = mpmath
CUTS = (7.5, 15.0, 30.0, 31.0)
BEXP_CLASSES = ("ltr > 100", "ltr < -100", "|ltr| < 1e-6", "in between", "exactly zero")
EARLY = ("inner pick of the part's root outside the root part", "exact-date tip", "reform of the root", "reform of a branch without mutations",
         "n_nodes < 3", "drawn time on a bound", "root displacement outside its window", "slide above X", "slide of the root",
         "slide without a straddling branch", "topology move under the part's root outside the root part",
         "SPR1 time on an end of its region")
REFORM_SIZES = ("1", "2", "3", "4", "more than 4", "a site twice", "more than 32")
SPR1_TIMES = ("below the root", "power law", "gamma")


class Borderline(Exception):
    pass


class Mismatch(Exception):
    pass


# ---- the stream -------------------------------------------------------------------------------------------------------
class Words:
    """The words of a part's stream from a position (a part_rng() dict with has_spare known)."""

    def __init__(self, rng):
        self.key, self.at = np.uint64(rng["key"]), 2 * int(rng["counter"]) - int(bool(rng["has_spare"]))
        self._blocks = {}
        if rng["has_spare"] and rng.get("spare") is not None:
            if self[0] != int(rng["spare"]):
                raise Mismatch("the stream's pending half block is not the second half of block %d" % (int(rng["counter"]) - 1))

    def __getitem__(self, i):
        idx = self.at + i
        blk = self._blocks.get(idx >> 1)
        if blk is None:
            w = RS.philox4x32_10(np.uint64(idx >> 1), self.key)
            blk = self._blocks[idx >> 1] = (int(w[0]) | (int(w[1]) << 32), int(w[2]) | (int(w[3]) << 32))
        return blk[idx & 1]


def index_of(rng):
    return 2 * int(rng["counter"]) - int(bool(rng["has_spare"]))


def to_co(w):
    return F(w >> 11, 2 ** 53)


def to_oo(w):
    return F(2 * (w >> 12) + 1, 2 ** 53)


def to_oc(w):
    return F((w >> 11) + 1, 2 ** 53)


def pick(w, n):
    return (w * n) >> 64


def kind_of(word, mix_total=32.0, topology=True):
    r = 0.0 + (mix_total - 0.0) * float(to_co(word))        # mix_draw: the double, as the cuts are doubles
    k = sum(r >= c for c in CUTS)
    return k if (k < 3 or topology) else -1


# ---- the distributions ------------------------------------------------------------------------------------------------
def bexp_offset(v, lam, D):
    """F^-1(v) - a of the bounded exponential of slope lam on a window of length D, as an mpmath number (call inside workdps)."""
    if lam == 0:
        return _mp(v) * _mp(D)
    L = _mp(lam) * _mp(D)
    off = mp.log1p(_mp(v) * mp.expm1(L)) / _mp(lam)
    return min(max(off, mp.mpf(0)), _mp(D))


def bexp_class(lam, D):
    L = lam * D
    if L == 0:
        return 4
    return 0 if L > 100 else 1 if L < -100 else 2 if abs(L) < F(1, 10 ** 6) else 3


def bexp_interval(v, lam, d, a, b):
    """(lo, hi, class) of the admissible new time, Fractions; raises Borderline at the -100 switch.  None, None when lambda's sign is not
    determined.  v = to_oo(word)."""
    D = b - a
    dd = d + 3 * U * abs(lam)
    if lam - dd <= 0 <= lam + dd and lam != 0 or (lam == 0 and dd > 0):
        return None, None, bexp_class(lam, D)
    with mp.workdps(X._DPS):
        L = lam * D
        cls = bexp_class(lam, D)
        if lam != 0 and abs(L + 100) <= 100 * dd / abs(lam):
            raise Borderline("ltr %r within its bound of -100" % float(L))
        vv = 1 - v if L < -100 else v
        offs = [bexp_offset(vv, l, D) for l in (lam - dd, lam, lam + dd)]
        off = offs[1]
        mags = 2 * max(abs(a), abs(b))
        anchor = _mp(D) - off if L > 100 else off
        R = _mp(U) * (_mp(mags) + 6 * abs(anchor))
        if lam != 0 and abs(L) <= 100:
            E = mp.expm1(_mp(L))
            y = _mp(v) * E
            R += abs(y) / ((1 + y) * abs(_mp(lam))) * _mp(U) * (2 * mp.exp(_mp(L)) / abs(E) + 2)
        elif lam != 0:
            R += mp.exp(-abs(_mp(L))) / (_mp(v) * abs(_mp(lam)))
        lo = max(_mp(a) + offs[0] - R, _mp(a))
        hi = min(_mp(a) + offs[2] + R, _mp(b))
        return X._frac(lo), X._frac(hi), cls


def gauss_z(w1, w2):
    """(z, r) as mpmath numbers (call inside workdps)."""
    r = mp.sqrt(-2 * mp.log(_mp(to_oc(w1))))
    return r * mp.cos(2 * mp.pi * _mp(to_co(w2))), r


def gaussian_step(w1, w2, lam: X.Exact, span, at):
    """(delta, bound) of sigma z, sigma = min(1 / (2 lambda), span), as Fractions; `at`: the magnitude the new time has."""
    with mp.workdps(X._DPS):
        z, r = gauss_z(w1, w2)
        d = F(lam.bound())
        assert lam.value - d > 0, "lambda's sign is not determined"
        sig = [min(1 / (2 * l), span) for l in (lam.value + d, lam.value, lam.value - d)]
        delta = _mp(sig[1]) * z
        width = _mp(sig[2] - sig[0]) / _mp(sig[1]) if sig[1] else mp.mpf(0)
        bound = abs(delta) * (3 * _mp(U) + width) + 26 * _mp(U) * _mp(sig[1]) * r + _mp(U) * (_mp(abs(at)) + abs(delta))
        return X._frac(delta), X._frac(bound)


def power_quantile(v, a, s_min, s_max):
    """(s, bracket) with (s^a - s_min^a) / (s_max^a - s_min^a) = v, mpmath numbers (call inside workdps)."""
    am = _mp(a)
    lo_a, hi_a = (mp.power(_mp(s_min), am) if s_min else mp.mpf(0)), mp.power(_mp(s_max), am)
    br = lo_a + _mp(v) * (hi_a - lo_a)
    return mp.power(br, 1 / am), br


def gamma_Q(a, x):
    return mp.gammainc(_mp(a), x, mp.inf, regularized=True)


def slope_exact(dv, node) -> X.Exact:
    """exact_model.displacement_slope with the S and n of its terms: the node's lambda once per branch it bounds, each child's missing
    intervals and missation from-states once."""
    T = dv.T
    k = (0 if node == T.root else 1) + len(T.kids[node])
    S, n = k * dv.lam_S[node], k * dv.lam_n[node]
    for c in T.kids[node]:
        for s, e in T.miss[c]:
            S += dv.cum[e] + dv.cum[s]; n += 2
        for l, st in T.mfs[c].items():
            S += dv.evo.rate(l, st) + dv.evo.rate(l, dv.ref[l]); n += 2
    return X.Exact(X.displacement_slope(dv, node), S, n)


# ---- windows as the moves form them -----------------------------------------------------------------------------------
def inner_window(T, node):
    """(t_min, t_max) of inner_node_displace_body on exact_model._Tree T; t_min None for the root."""
    lo = None
    if node != T.root:
        lo = max([T.t[T.parent[node]]] + [F(m[3]) for m in T.muts[node]])
    hi = min([T.t[c] for c in T.kids[node]] + [F(m[3]) for c in T.kids[node] for m in T.muts[c]])
    return lo, hi


def tip_window(T, tree, node):
    lo = max([F(float(tree.t_min[node])), T.t[T.parent[node]]] + [F(m[3]) for m in T.muts[node]])
    return lo, F(float(tree.t_max[node]))


def reform_times(old_sites, words, t_P, t_X):
    """The new (site, old index, time) of every mutation of the branch, times as Fractions."""
    us = [to_oc(w) for w in words]
    n = len(old_sites)
    out = [None] * n
    if len(set(old_sites)) == n:
        for i in range(n):
            out[i] = t_P + (t_X - t_P) * us[i]
        return out
    k = 0
    for l in sorted(set(old_sites)):
        idx = [i for i in range(n) if old_sites[i] == l]
        ts = sorted(t_P + (t_X - t_P) * us[k + j] for j in range(len(idx)))
        for i, t in zip(idx, ts):
            out[i] = t
        k += len(idx)
    return out


# ---- one move ---------------------------------------------------------------------------------------------------------
class Step:
    """What check_step knows of one move."""

    def __init__(self, w, b, a, kind, node, noted, acc, log_mh, compound, mix_total=32.0, topology=True):
        self.w, self.b, self.a, self.kind, self.node, self.noted, self.acc, self.log_mh, self.compound = w, b, a, kind, node, noted, acc, log_mh, compound
        self.mix_total, self.topology = mix_total, topology


def _near(got, want, bound, what, share):
    """got, want, bound Fractions.  Records the share of the bound used."""
    e = abs(got - want)
    share[what] = max(share.get(what, 0.0), float(e / bound) if bound else (0.0 if e == 0 else float("inf")))
    if e > bound:
        raise Mismatch("%s: %r, the draw says %r: %.3g of its bound %.3g" % (what, float(got), float(want), float(e / bound) if bound else float("inf"), float(bound)))


def check_reading(s: Step, rb, ra, cov, share):
    """Every identity of the step under one reading (rb, ra) of the stream's position before and after.  Raises Mismatch or
    Borderline; counts into cov (a fresh Coverage-like object the caller merges) and `share`."""
    w, tb, ta = s.w, s.b["tree"], s.a["tree"]
    dv = w.dv
    T = dv.T
    n_nodes, root = T.n, T.root
    W = Words(rb)
    used = index_of(ra) - index_of(rb)
    if used < 1:
        raise Mismatch("the move consumed %d words" % used)
    k = kind_of(W[0], s.mix_total, s.topology)
    if k != s.kind:
        raise Mismatch("word 0 says %s, the row %s" % (k, s.kind))
    is_tip = lambda x: not T.kids[x]
    at = 1                      # words stated so far
    exact_words = True          # whether the model states every word of the move

    def picks(ok):
        nonlocal at
        while True:
            x = pick(W[at], n_nodes); at += 1
            if ok(x):
                return x
            if at > 4096:
                raise Mismatch("no acceptable pick in 4096 words")

    def ends_here(why):
        if s.noted:
            raise Mismatch("the move must end un-noted (%s), the row is noted" % EARLY[why])
        if used != at:
            raise Mismatch("the move ends after %d words (%s), it consumed %d" % (at, EARLY[why], used))
        cov.draws_early_end[why] += 1
        if why in (1, 2):
            cov.draws_ends_at_once[(0 if w.includes_root else 3) + why - 1] += 1

    def verdict(last):
        """The acceptance of a noted move whose last word (if it takes one) is word `last` - 1."""
        nonlocal at
        if not s.noted:
            raise Mismatch("the move must be noted, the row is not")
        if s.log_mh >= 0.0:
            if not s.acc:
                raise Mismatch("log_mh >= 0 and not accepted")
            return
        with mp.workdps(X._DPS):
            v, e = to_co(W[last - 1]), mp.exp(mp.mpf(s.log_mh))
            if abs(_mp(v) - e) <= 4 * _mp(U) * e:
                raise Borderline("the acceptance draw %r within 4 u of exp(log_mh)" % float(v))
            want = _mp(v) < e
        if want != s.acc:
            raise Mismatch("the acceptance draw %r against exp(log_mh) %r says %s" % (float(v), float(e), "accepted" if want else "rejected"))
        cov.draws_verdicts_drawn += 1

    def bexp(lam: X.Exact, lo, hi):
        """The bounded exponential's word is W[at]."""
        nonlocal at
        v = to_oo(W[at]); at += 1
        l_lo, l_hi, cls = bexp_interval(v, lam.value, F(lam.bound()), lo, hi)
        new_t = F(float(ta.t[s.node]))
        if l_lo is None:
            D = hi - lo
            if s.acc and abs(new_t - (lo + v * D)) <= U * (abs(lo) + 2 * D + abs(new_t)):
                cov.draws_bexp[4] += 1
                share["bounded exponential, uniform"] = max(share.get("bounded exponential, uniform", 0.0), float(abs(new_t - (lo + v * D)) / (U * (abs(lo) + 2 * D + abs(new_t)))))
            else:
                cov.slope_sign_undetermined += 1
            if s.noted:
                verdict(used); at = used
            return
        if not s.noted:
            if not (l_lo <= lo or l_hi >= hi):
                raise Mismatch("un-noted, but the drawn time lies in [%r, %r], inside (%r, %r)" % (float(l_lo), float(l_hi), float(lo), float(hi)))
            ends_here(5)
            return
        if s.acc:
            mid, half = (l_lo + l_hi) / 2, (l_hi - l_lo) / 2
            _near(new_t, mid, half, "bounded exponential, " + BEXP_CLASSES[cls], share)
            cov.draws_bexp[cls] += 1
            cov.draws_bexp_outside_root_part[cls] += int(not w.includes_root)
        at += int(s.log_mh < 0.0)
        verdict(at)

    if s.kind == 0:
        node = picks(lambda x: not is_tip(x))
        if node != s.node:
            raise Mismatch("the first inner pick is node %d" % node)
        if node == root and not w.includes_root:
            ends_here(0)
        elif node == root:
            lo, hi = inner_window(T, node)
            span = F(float(w.t_max_tip)) - hi
            old_t = T.t[node]
            delta, bound = gaussian_step(W[at], W[at + 1], dv.lambda_i(node), span, abs(old_t) + abs(hi))
            at += 2
            new_t = old_t + delta
            if abs(new_t - hi) <= bound:
                raise Borderline("the root's new time within its bound of t_max")
            if new_t > hi:
                ends_here(6)
            else:
                if s.acc:
                    _near(F(float(ta.t[node])) - old_t, delta, bound, "gaussian, root displacement", share)
                    cov.draws_gaussian_root += 1
                # cells the grid appended for the proposed time (very_scalable_coalescent.cpp:259-299): one Gaussian each, before the verdict
                tabb, taba = s.b["tab"], s.a["tab"]
                for i in range(len(tabb["k_bar_p"]), len(taba["k_bar_p"])):
                    with mp.workdps(X._DPS):
                        z, r = gauss_z(W[at], W[at + 1])
                        sig = mp.sqrt(_mp(F(float(taba["popsize_bar"][i]))) / _mp(F(float(taba["t_step"]))))
                        _near(F(float(taba["k_twiddle_bar_p"][i])), X._frac(sig * z), X._frac(_mp(U) * sig * (5 * abs(z) + 26 * r)), "gaussian, appended grid cell", share)
                    at += 2
                    cov.draws_grid_cells += 1
                at += int(s.noted and s.log_mh < 0.0)
                verdict(at)
        else:
            lo, hi = inner_window(T, node)
            bexp(slope_exact(dv, node), lo, hi)
    elif s.kind == 1:
        node = picks(is_tip)
        if node != s.node:
            raise Mismatch("the first tip pick is node %d" % node)
        if tb.t_min[node] == tb.t_max[node]:
            ends_here(1)
        else:
            lo, hi = tip_window(T, tb, node)
            lam = dv.lambda_i(node)
            bexp(X.Exact(-lam.value, lam.S, lam.n), lo, hi)
    elif s.kind == 2:
        if n_nodes < 3:
            if s.node != -1:
                raise Mismatch("n_nodes < 3 and a node in the row")
            ends_here(4)
        else:
            node = pick(W[at], n_nodes); at += 1
            if node != s.node:
                raise Mismatch("the pick is node %d" % node)
            if node == root:
                ends_here(2)
            elif s.compound:
                exact_words = False
                if used < at:
                    raise Mismatch("fewer words than the leading ones")
                verdict(used)
            else:
                sites = [m[0] for m in T.muts[node]]
                n = len(sites)
                if n == 0:
                    if not (s.noted and s.acc and s.log_mh == 0.0):
                        raise Mismatch("a reform of a branch without mutations must be accepted with log_mh 0.0")
                    cov.draws_early_end[3] += 1
                    cov.draws_ends_at_once[(0 if w.includes_root else 3) + 2] += 1
                else:
                    words = [W[at + i] for i in range(n)]
                    at += n
                    if s.acc:
                        t_P, t_X = T.t[T.parent[node]], T.t[node]
                        want = reform_times(sites, words, t_P, t_X)
                        new = X._Tree(ta).muts[node]
                        bound = 2 * U * (abs(t_P) + abs(t_X - t_P))
                        for l in set(sites):
                            wi = [want[i] for i in range(n) if sites[i] == l]
                            got = [F(m[3]) for m in new if m[0] == l]
                            if len(got) != len(wi):
                                raise Mismatch("site %d has %d mutations after, %d before" % (l, len(got), len(wi)))
                            for g, x in zip(got, wi):
                                _near(g, x, bound, "branch reform time", share)
                        for i, hit in enumerate((n == 1, n == 2, n == 3, n == 4, n > 4, len(set(sites)) < n, n > 32)):
                            cov.draws_reforms[i] += int(hit)
                    at += int(s.noted and s.log_mh < 0.0)
                verdict(at)
    elif s.kind == 3:
        exact_words = False
        if n_nodes < 2:
            ends_here(4)
        else:
            Xn = pick(W[at], n_nodes); at += 1
            if Xn != s.node:
                raise Mismatch("the pick is node %d" % Xn)
            if Xn == root:
                ends_here(8)
            else:
                P = T.parent[Xn]
                S = [c for c in T.kids[P] if c != Xn][0]
                t_early = min(T.t[Xn], T.t[S]) if P == root else T.t[root]
                span = F(float(w.t_max_tip)) - t_early
                old = T.t[P]
                delta, bound = gaussian_step(W[at], W[at + 1], dv.lambda_i(Xn), span, abs(old) + abs(T.t[Xn]))
                at += 2
                new = old + delta
                cmp = [old, T.t[Xn], T.t[S]] + ([T.t[T.parent[P]]] if P != root else [])
                if any(abs(new - c) <= bound for c in cmp):
                    raise Borderline("the slide's new time within its bound of a comparison")
                under_root = not w.includes_root and P == root
                SS = None
                if delta > 0 and new > T.t[Xn]:
                    ends_here(7)
                elif delta > 0 and new > T.t[S]:
                    # (the order of a node's two children is the snapshot's: a rejected topology move may have swapped them, and the watch's
                    # exact tree, carried from move to move, does not follow that)
                    br = straddling_branches(X._Tree(tb), P, new, Xn)
                    if any(abs(new - T.t[v]) <= bound for v in _below(T, P, Xn)):
                        raise Borderline("the slide's new time within its bound of a node below P")
                    if not br:
                        ends_here(9)
                    else:
                        SS = br[pick(W[at], len(br))]; at += 1
                        if under_root:
                            ends_here(10)
                        else:
                            _slide_rest(s, cov, share, used, at, verdict, T, ta, P, Xn, SS, delta, bound, len(br))
                else:
                    if delta < 0 and P != root and new < T.t[T.parent[P]]:
                        GG, SS = T.parent[P], P
                        anc = []
                        while GG >= 0:
                            anc.append(GG); GG = T.parent[GG]
                        if any(abs(new - T.t[v]) <= bound for v in anc):
                            raise Borderline("the slide's new time within its bound of an ancestor")
                        GG = T.parent[P]
                        while new < T.t[GG]:
                            SS, GG = GG, T.parent[GG]
                            if GG < 0:
                                break
                    else:
                        SS = S
                    if under_root or (not w.includes_root and SS == root):
                        ends_here(10)
                    else:
                        _slide_rest(s, cov, share, used, at, verdict, T, ta, P, Xn, SS, delta, bound, None)
    elif s.kind == 4:
        exact_words = False
        if n_nodes < 2:
            ends_here(4)
        else:
            at += 1                     # the chooser (check_spr1_time reads it)
            Xn = picks(lambda x: x != root)
            if Xn != s.node:
                raise Mismatch("the first pick that is not the root is node %d" % Xn)
            if dv.lam[Xn] == 0 or (T.parent[Xn] == root and not w.includes_root):
                ends_here(10)
            elif not s.noted:
                # the time drawn in the region equals t_X or an end of the new branch (subrun.cpp:560-566): after the region's word and the
                # time's; which region the walk picked is out of scope, so only the words are held
                at += 2
                ends_here(11)
            else:
                if used < at + 2:
                    raise Mismatch("fewer words than the leading ones")
                verdict(used)
    else:
        raise Mismatch("kind %d" % s.kind)
    if exact_words and used != at:
        raise Mismatch("the model states %d words, the move consumed %d" % (at, used))
    cov.draws_held += 1


def straddling_branches(B, top, t, Xn):
    """The branches below `top` that hold time t on tree B (exact_model._Tree), X's subtree pruned, depth first with child0 first
    (enumerate_descendant_branches_straddling; subrun.cpp:325-350): alpha_ratio's n is its length (move_steps.slide_alpha_ratio), and a
    slide down past the sibling picks its new sibling from it by index."""
    out, st = [], [top]
    while st:
        v = st.pop()
        if v == Xn:
            continue
        if t <= B.t[v]:
            out.append(v)
        else:
            st += reversed(B.kids[v])
    return out


def _below(T, top, Xn):
    out, st = [], [top]
    while st:
        v = st.pop()
        if v != Xn:
            out.append(v); st += T.kids[v]
    return out


def _slide_rest(s, cov, share, used, at, verdict, T, ta, P, Xn, SS, delta, bound, n_down):
    """A slide that reached spr_move_core: noted; accepted -> the Gaussian and the new sibling."""
    if used < at:
        raise Mismatch("fewer words than the leading ones")
    verdict(used)
    if not s.acc:
        return
    got = F(float(ta.t[P])) - T.t[P]
    _near(got, delta, bound, "gaussian, subtree slide", share)
    new_S = [c for c in (int(ta.child0[P]), int(ta.child1[P])) if c != Xn][0]
    if new_S != SS:
        raise Mismatch("the new sibling is %d, the draw says %d" % (new_S, SS))
    cov.draws_gaussian_slide += 1
    if n_down is not None and n_down >= 2:
        cov.draws_slide_down_picks += 1


def spr1_time(cov, share, word, d):
    """The time an accepted SPR1 drew inside its new region.  d: move_steps.spr1_identity's dict, with `limit`."""
    pre, ri = d["pre"], d["new_region"]
    r = pre.regions[ri]
    t = F(float(d["ga"].t_P))
    with mp.workdps(X._DPS):
        if not r.above_root:
            want = r.t_min + (r.t_max - r.t_min) * to_oc(word)
            _near(t, want, 2 * U * (abs(r.t_min) + abs(r.t_max - r.t_min)), "spr1 time below the root", share)
            cov.draws_spr1_times[0] += 1
            return
        t_X = pre.pr.t_X
        t_S, s_min, s_max, x_min, x_max, a = pre._root_params(r)
        s_obs = (t_X - t) + (t_S - t)
        t_round = 4 * U * (abs(t_X) + abs(t_S) + abs(s_obs))
        if pre.root_kind == "power":
            v = to_oo(word)
            am = _mp(a)
            want, br = power_quantile(v, a, s_min, s_max)
            nu = 16 + 4 * (am * abs(mp.log(_mp(s_max))) + (am * abs(mp.log(_mp(s_min))) if s_min else 0) + abs(mp.log(br)) / am)
            bound = X._frac(want * _mp(U) * nu) + t_round
            want = min(max(X._frac(want), s_min), s_max)
            _near(s_obs, want, bound, "spr1 time above the root, power law", share)
            cov.draws_spr1_times[1] += 1
        else:
            lam = d["lam"]
            beta = _mp(lam.value * pre.f)
            Q = lambda x: gamma_Q(a, x)
            q_hi, q_lo = Q(beta * _mp(s_min)), Q(beta * _mp(s_max))
            want = q_lo + (q_hi - q_lo) * _mp(to_oc(word))
            y = beta * _mp(s_obs)
            got = Q(y)
            g = mp.exp((_mp(a) - 1) * mp.log(y) - y - mp.loggamma(_mp(a))) if y > 0 else mp.mpf(0)
            tol = lambda q: mp.mpf("1e-12") + mp.mpf("1e-9") * q
            rel_lam = (lam.n + 8) * _mp(U) * _mp(lam.S / lam.value) + 4 * _mp(U)
            bound = tol(q_hi) + tol(q_lo) + tol(want) + g * (beta * _mp(t_round) + y * rel_lam)
            if s_obs in (s_min, s_max) or abs(s_obs - s_min) <= t_round or abs(s_obs - s_max) <= t_round:     # clamped: the draw lies at or beyond the edge
                if (s_obs <= s_min + t_round and want >= got - bound) or (s_obs >= s_max - t_round and want <= got + bound):
                    cov.draws_spr1_times[2] += 1
                    return
            _near(X._frac(got), X._frac(want), X._frac(bound), "spr1 time above the root, gamma (in Q)", share)
            cov.draws_spr1_times[2] += 1


# ---- the two entries move_steps calls -----------------------------------------------------------------------------------
def _readings(rng):
    return [rng] if rng["has_spare"] is not None else [dict(rng, has_spare=hs, spare=None) for hs in (False, True)]


def _one_reading_of(cov, fresh, run, readings, what):
    """run(reading, cov, share) under every reading; exactly one may satisfy every identity.  -> (share, failure text or None)."""
    good, bad, border = [], [], []
    for r in readings:
        c, share = fresh(), {}
        try:
            run(r, c, share)
            good.append((c, share))
        except Borderline as e:
            border.append(str(e))
        except Mismatch as e:
            bad.append(str(e))
    if len(readings) > 1:
        cov.position_half_known += 1
    if border and not good:
        cov.borderline += 1
        return {}, None
    if len(good) != 1:
        return {}, "%s: %s" % (what, "; ".join(bad) if not good else "the stream's position is half known and %d readings satisfy every identity" % len(good))
    cov.add(good[0][0])
    return good[0][1], None


def check_draws(tally, cov, step: Step, where):
    """Every identity of one move; failures to tally.fail and cov.unchecked."""
    readings = [(rb, ra) for rb in _readings(step.b["rng"]) for ra in _readings(step.a["rng"])]
    share, fail = _one_reading_of(cov, type(cov), lambda r, c, sh: check_reading(step, r[0], r[1], c, sh), readings, "draws")
    for k, v in share.items():
        k = "draw: %s (share of its bound)" % k
        tally.worst[k] = max(tally.worst.get(k, 0.0), v)
    if fail:
        tally.fail.append("%s: %s" % (where, fail)); cov.unchecked += 1


def check_spr1_time(tally, cov, w, Xn, d, limit, rng_before, where, mix_total=32.0):
    """The time an accepted SPR1 of X drew in its new region, from the stream's position before the move (check_accepted_spr1 calls
    this with spr1_identity's dict)."""
    T = w.dv.T

    def run(rb, c, share):
        W = Words(rb)
        if kind_of(W[0], mix_total) != 4:
            raise Mismatch("word 0 does not say SPR1")
        if (None if to_co(W[1]) < F(0.01) else 1) != limit:
            raise Mismatch("the chooser does not give the limit the study was made at")
        at = 2
        while pick(W[at], T.n) == T.root:
            at += 1
        if pick(W[at], T.n) != Xn:
            raise Mismatch("the first pick that is not the root is node %d" % pick(W[at], T.n))
        spr1_time(c, share, W[at + 2], d)
    share, fail = _one_reading_of(cov, type(cov), run, _readings(rng_before), "spr1 time")
    for k, v in share.items():
        k = "draw: %s (share of its bound)" % k
        tally.worst[k] = max(tally.worst.get(k, 0.0), v)
    if fail:
        tally.fail.append("%s: %s" % (where, fail)); cov.unchecked += 1
