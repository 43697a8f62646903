"""One move at a time: the engine's DECISIONS against the exact posterior of tests/exact_model.py.

`step_chain` advances every part's chain by one move per pass on an OracleEngine or an EmatBackend and hands `on_step` the
part's state before and after each move; `check_step` holds the move's trace row and the increments of the maintained totals
to the identities the move code implies (emat_device_moves.hpp; the reference's core/subrun.cpp:148-320, 683-742):

- a tip displacement, or the displacement of an inner node other than the run's root, proposes the new time from a bounded
  exponential with exactly the slope of log G, so delta log G and the proposal ratio are the same product and
  log_mh = partial prior(after) - partial prior(before); and log G is linear in that time: log G(after) - log G(before) =
  d_logG_dt (new_t - old_t) EXACTLY, with d_logG_dt rebuilt from exact lambda_i and the exact rate change across the children's
  missing intervals (exact_model.displacement_slope), as Fractions;
- the displacement of the run's root is a symmetric step: log_mh = delta log G + delta partial prior;
- a branch reform re-times one branch's mutations uniformly: log_mh = delta log G, the prior and k_bar_p untouched;
- an accepted subtree slide of X (spr_move_core, subrun.cpp:683-742; the slide's own Hastings factor, subrun.cpp:352-448): log_mh =
  [delta_log_G - log_alpha_mut](the model's graft of X on the tree after) - [the same on the tree before] + log(alpha_ratio) +
  partial prior(after) - partial prior(before).  The grafts are tests/graft_model.py's, at mu_proposal = lambda(root) / (L - sites
  missing at the root) of the tree BEFORE, taken exactly (its own bound, times log_alpha_mut's sensitivity to mu, joins the bound).  alpha_ratio from the tree before, X and
  the new time: 1 along the same branch; 1/n up past an ancestor, n the branches that straddle the OLD time below the new sibling
  with X's subtree pruned; n down past the sibling, n the branches that straddle the NEW time below P with X's subtree pruned.  The new
  graft's history is read from the tree after, so this also says that log_alpha_mut is the density of the history written;
- for all five kinds the increment of the maintained log_G and log_aug_prior over the one move is the exact difference.
- an accepted SPR1 move of X (subrun.cpp:492-675): log_mh = [delta_log_G - log_alpha_mut](new graft) - [the same](old graft) +
  log_alpha_n2o - log_alpha_o2n + partial prior(after) - partial prior(before).  The graft terms are the slide's; log_alpha_o2n is the
  density of (new sibling's region, new t_P) in the study of tests/study_model.py scanned from the old sibling, log_alpha_n2o that of
  (old sibling, old t_P) in the study scanned from the new one, both on the tree with X's graft read off (asserted to be the same tree
  before and after), at the scan limit the move's second draw gave.  The limit is read from the part's random stream before the move:
  its first word through mix_draw must say SPR1 (asserted), its second through to_co is below 0.01 for an unlimited scan.  The model is
  evaluated at that limit only;
- what every move DREW -- the kind, the node picks, the number of words it consumed, its acceptance, the bounded exponential, the
  Gaussian step, the slide's pick among straddling branches, a reform's new mutation times, the time inside an SPR1 region -- is held, by
  the probability integral transform, to the exact inverse CDF at the very uniforms of the part's random stream: tests/draws_model.py has
  the identities and their bounds, check_step calls it for every move.  Which region an SPR1's cumulative walk picks is not held (it
  depends on the depth-first order, which only the algorithm defines; its probability is held through log_alpha), nor are the draws of
  the mutational-history sampler (the density of the history written is) or a compound reform's inner move.

Bounds.  A log_mh or an increment is held to the `Exact.bound()` of the difference, whose S holds only the terms that differ
(exact_model's docstring).  Added to it, each named:
- the engine evaluates the prior on its MAINTAINED k_bar_p, so a prior difference (log_mh and the log_aug_prior increment, the
  same number) gets the sum over the cells that differ of |w (k A - c)| times check_part's k_bar_p allowance at that move count;
- the increment of a total gets 2 u max(|total before|, |total after|): the one addition at the total's magnitude;
- a simple displacement's log_mh adds delta log G and takes the proposal ratio, the same product, away again: twice that
  product's magnitude joins S (exact_model's docstring, last rule);
- an accepted slide's log_mh gets the sum of its four graft numbers' own Exact.bound() (each formed whole), the prior difference's
  with its k_bar_p allowance, 8 u |log alpha_ratio|, and for the computed proposal rate (n_lambda + 9) u S_mu times the sum over both
  log_alpha_mut's terms of |d term / d mu| (the rate's error reaches log_mh only through that derivative, so the rate's term count
  does not multiply the whole of log_alpha_mut's S);
- an accepted SPR1's log_mh gets the same four graft bounds, the rate's term and the prior's with k_bar_p's allowance, the two densities'
  own Exact.bound(), their gamma_term where a region above the root is involved, and for the computed lambda_X
  (n_lambda + 8) u S_lambda / lambda_X times the two densities' lambda_sensitivity (study_model's docstring names each).

One row, two decisions.  In the part that holds the run's root, a branch reform of a child of the root first runs
spr_move_core in place (subrun.cpp:298-303: the mutations of both root branches "dance"), which accepts or rejects on its own
and leaves no trace row; the row holds the reform's log_mh alone.  Between the two no state can be read, so for these steps
(`compound`) log_mh has no identity over the states before and after; the increments of both totals, which cover both
decisions together, and the validity of the new state are checked, and the steps are counted apart.

A move that is not accepted (rejected, or an early return with a NaN log_mh) leaves log_G, log_aug_prior, k_bar_p (cells the
root part's grid appended while it evaluated the proposal aside: they hold 1), the topology (after a rejected topology move a
node's two children may have changed slots: the pruned subtree goes back under its old parent as its other child), every node
time and every mutation's site and states bit for bit as they were.  Mutation times and lambda_i after a rejected TOPOLOGY move,
as established on the CPU oracle over every rejected subtree slide and SPR1 move of test_move_steps.py's cases:
- mutation times come back bit for bit (peel_graft followed by apply_graft of the old graft puts back the very doubles it took
  out), and so they are asserted of the device -- but for a subtree pruned from under the RUN'S ROOT: the rooty graft reflects
  the sibling branch's mutations about the root's time and back (t -> t_P - (t - t_P) -> t_P + (t_P - t'), four roundings),
  and those times are held to 4 u (|t_P| + |t - t_P|), all others bit for bit;
- lambda_i is NOT always bit-identical: hopping the pruned subtree up and down the tree recomputes the lambda of the nodes it
  passes, and the rooty graft recomputes the root's from its child's.  Where it differs it is held to its Exact bound; where
  it does not (most rejected moves, and every simple move) the bits are asserted.
"""
from fractions import Fraction as F

import numpy as np

import draws_model as DM
import exact_model as X
import graft_model as GM
import study_model as SM

KINDS = ("inner_node_displace", "tip_displace", "branch_reform", "subtree_slide", "spr1")
_TOPO = ("root", "parent", "child0", "child1", "t_min", "t_max", "mut_offset", "miss_offset", "miss_start", "miss_end", "mfs_offset", "mfs_site", "mfs_state")
_MUT = ("mut_site", "mut_from", "mut_to")


# ---- the stepper ----------------------------------------------------------------------------------------------------
def snapshot(engine, p):
    """What one part holds now.  (A device engine is synchronised by step_chain before this reads it.)"""
    st = engine.part_stats(p)
    tree = engine.part_download(p)
    lam, nsm, G, A = engine.part_derived(p, tree.num_nodes)
    tr = engine.part_trace(p, max(int(st["moves_done"]), 1))
    return dict(tree=tree, lam=lam, nsm=nsm, G=float(G), A=float(A), tab=engine.part_coalescent(p), stats=st, rng=stream_position(engine, p, st),
                row=tr[-1].copy() if tr.shape[0] else None, trace_len=tr.shape[0])


def stream_position(engine, p, stats=None):
    """Where part p's random stream stands: engine.part_rng(p).  The device reports it only while the parts lie on it -- not before the
    first pass, nor between a pass that stopped for room and the next.  Then the position is put together from what the host keeps: the
    key (the part's seed, helpers.configure notes it; or the key read earlier) and the blocks opened (part_stats), with has_spare = None:
    whether half a block is pending is not known, unless no block has been opened."""
    keys = engine.__dict__.setdefault("_stream_keys", {})
    try:
        r = engine.part_rng(p)
        keys[p] = r["key"]
        return r
    except Exception as e:
        if "not on a device" not in str(e):
            raise
    key = keys.get(p)
    if key is None:
        key = int(getattr(engine, "_part_seeds")[p])
    ctr = int((stats or engine.part_stats(p))["rng_draws"])
    return dict(key=key, counter=ctr, spare=None, has_spare=False if ctr == 0 else None)


def advance_one_move(engine):
    if hasattr(engine, "synchronize"):
        engine.run_moves_per_part(1); engine.synchronize()
    else:
        engine.run_moves_per_part(1, threads=1)


def step_chain(engine, part_ids, steps, on_step, advance=advance_one_move):
    """`steps` passes of one move per part; on_step(p, step, before, after) for every watched part after every pass."""
    if hasattr(engine, "synchronize"):
        engine.synchronize()
    import time
    prev = {p: snapshot(engine, p) for p in part_ids}
    cost = step_chain.cost = dict(passes=0, advance_s=0.0, read_s=0.0)      # what the engine's side of a pass takes
    for s in range(steps):
        t0 = time.perf_counter()
        advance(engine)
        t1 = time.perf_counter()
        curs = {p: snapshot(engine, p) for p in part_ids}
        cost["passes"] += 1; cost["advance_s"] += t1 - t0; cost["read_s"] += time.perf_counter() - t1
        for p in part_ids:
            on_step(p, s, prev[p], curs[p])
            prev[p] = curs[p]
    return prev


def trees_identical(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f)) for f in _TOPO[1:] + _MUT + ("t", "mut_t")) and a.root == b.root


def assert_stepped_chain_is_the_chain(make_engine, num_parts, moves):
    """`make_engine()` -> a configured engine with a trace of at least `moves` rows.  `moves` passes of one move against one
    pass of `moves` moves: traces and final trees bit for bit, the random streams at the same position."""
    one, many = make_engine(), make_engine()
    try:
        dev = hasattr(one, "synchronize")
        for _ in range(moves):
            advance_one_move(one)
        if dev:
            many.run_moves_per_part(moves); many.synchronize()
        else:
            many.run_moves_per_part(moves, threads=1)
        for p in range(num_parts):
            s1, s2 = one.part_stats(p), many.part_stats(p)
            assert s1["status"] == 0 and s2["status"] == 0
            assert s1["moves_done"] == s2["moves_done"] == moves, (p, s1, s2)
            assert s1["rng_draws"] == s2["rng_draws"], "part %d: rng draws %d stepped, %d in one pass" % (p, s1["rng_draws"], s2["rng_draws"])
            assert s1["proposed"] == s2["proposed"] and s1["accepted"] == s2["accepted"], (p, s1, s2)
            t1, t2 = one.part_trace(p, moves), many.part_trace(p, moves)
            assert t1.shape == t2.shape == (moves, 4)
            assert t1.tobytes() == t2.tobytes(), "part %d: the stepped trace differs from the pass's" % p
            assert trees_identical(one.part_download(p), many.part_download(p)), "part %d: the stepped tree differs from the pass's" % p
            n = s1["num_nodes"]
            d1, d2 = one.part_derived(p, n), many.part_derived(p, n)
            assert d1[0].tobytes() == d2[0].tobytes() and d1[2:] == d2[2:], "part %d: maintained totals differ" % p
    finally:
        one.close(); many.close()


# ---- validity of a part's tree, in plain Python -----------------------------------------------------------------------
def assert_valid_part(tree, ref):
    """Links mutual; t_parent < t_mut <= t_child along every branch; every branch's mutations sorted by (t, site); every
    mutation's `from` the state its site has just above it and no mutation on a site missing there; a tip inside
    [t_min, t_max]; missing intervals sorted, disjoint and non-adjacent.  Raises AssertionError with the place."""
    n, root = tree.num_nodes, int(tree.root)
    par, c0, c1 = tree.parent.tolist(), tree.child0.tolist(), tree.child1.tolist()
    t, tmin, tmax = tree.t.tolist(), tree.t_min.tolist(), tree.t_max.tolist()
    mo, ms, mf, mt, mtt = tree.mut_offset.tolist(), tree.mut_site.tolist(), tree.mut_from.tolist(), tree.mut_to.tolist(), tree.mut_t.tolist()
    io, s_, e_ = tree.miss_offset.tolist(), tree.miss_start.tolist(), tree.miss_end.tolist()
    ref = np.asarray(ref).tolist()
    assert 0 <= root < n and par[root] == -1, "root %d has parent %d" % (root, par[root])
    seen = 0
    for x in range(n):
        assert (c0[x] < 0) == (c1[x] < 0), "node %d has one child" % x
        for c in (c0[x], c1[x]):
            if c >= 0:
                assert 0 <= c < n and par[c] == x, "node %d lists child %d whose parent is %d" % (x, c, par[c])
        if c0[x] >= 0:
            assert c0[x] != c1[x], "node %d lists child %d twice" % (x, c0[x])
        else:
            # (t_min and t_max are stored in single precision; a tip without uncertainty keeps its date in double)
            assert float(tmin[x]) <= t[x] <= float(tmax[x]) or (tmin[x] == tmax[x] and float(np.float32(t[x])) == tmin[x]), \
                "tip %d at %r outside [%r, %r]" % (x, t[x], tmin[x], tmax[x])
        if x != root:
            P = par[x]
            assert 0 <= P < n and x in (c0[P], c1[P]), "node %d names parent %d, which does not list it" % (x, P)
            assert t[P] < t[x], "branch %d: t_parent %r >= t_child %r" % (x, t[P], t[x])
            prev = None
            for k in range(mo[x], mo[x + 1]):
                assert t[P] < mtt[k] <= t[x], "branch %d: mutation at %r outside (%r, %r]" % (x, mtt[k], t[P], t[x])
                assert prev is None or prev <= (mtt[k], ms[k]), "branch %d: mutations not sorted by (t, site)" % x
                prev = (mtt[k], ms[k])
        iv = [(s_[k], e_[k]) for k in range(io[x], io[x + 1])]
        for k, (s, e) in enumerate(iv):
            assert 0 <= s < e <= len(ref), "node %d: missing interval [%d, %d)" % (x, s, e)
            assert k == 0 or iv[k - 1][1] < s, "node %d: missing intervals %s not sorted, disjoint and non-adjacent" % (x, iv)
    # from-states and missing sites along every path: depth first with the states that differ from the ref's and the intervals
    state, stack = {}, [(root, None)]
    missing = []
    while stack:
        x, undo = stack.pop()
        if undo is not None:
            for l, old in reversed(undo[0]):
                if old is None:
                    state.pop(l, None)
                else:
                    state[l] = old
            del missing[undo[1]:]
            continue
        seen += 1
        log, nmiss = [], len(missing)
        missing.extend((s_[k], e_[k]) for k in range(io[x], io[x + 1]))
        for k in range(mo[x], mo[x + 1]):
            l = ms[k]
            cur = state.get(l, ref[l])
            assert cur == mf[k], "node %d: mutation of site %d from %d, the path says %d" % (x, l, mf[k], cur)
            assert mf[k] != mt[k], "node %d: mutation of site %d from %d to itself" % (x, l, mf[k])
            assert not any(s <= l < e for s, e in missing), "node %d: mutation on the missing site %d" % (x, l)
            log.append((l, state.get(l)))
            state[l] = mt[k]
        stack.append((x, (log, nmiss)))
        for c in (c1[x], c0[x]):
            if c >= 0:
                stack.append((c, None))
    assert seen == n, "%d of %d nodes hang on the root" % (seen, n)


# ---- the per-move checks ----------------------------------------------------------------------------------------------
class Coverage:
    """What the checked steps of a test file amount to (the conditions of the issue are asserted on the sum over its cases)."""
    FIELDS = ("steps", "accepted", "accepted_root_displacements", "accepted_negative_log_mh", "accepted_while_grid_grew",
              "accepted_reform_same_site_twice", "accepted_reform_more_than_32", "accepted_outside_root_part", "compound", "compound_accepted",
              "rejected_topology", "rejected_rooty_not_bit_identical", "rejected_topology_lambda_not_bit_identical", "unchecked",
              "accepted_slides_log_mh_exact", "accepted_slide_kinds", "accepted_spr1_log_mh_exact", "accepted_spr1_classes",
              "draws_held", "borderline", "slope_sign_undetermined", "position_half_known", "draws_verdicts_drawn", "draws_bexp", "draws_bexp_outside_root_part", "draws_gaussian_root",
              "draws_gaussian_slide", "draws_slide_down_picks", "draws_grid_cells", "draws_reforms", "draws_spr1_times", "draws_early_end", "draws_ends_at_once")
    SLIDE_KINDS = ("same branch", "up with n >= 2", "down with n >= 2", "X under the run's root", "X in a part without the run's root")
    SPR1_CLASSES = ("unlimited scan", "new region above the root, gamma", "new region above the root, power law", "old region above the root",
                    "part without the run's root", "min_muts >= 1 in the new region", "uncounted mutation on the path", "more than 64 regions",
                    "more than 640 regions")

    def __init__(self):
        self.steps = 0
        self.accepted = [0] * 5
        self.accepted_negative_log_mh = [0] * 3
        self.accepted_root_displacements = self.accepted_while_grid_grew = self.accepted_reform_same_site_twice = 0
        self.accepted_reform_more_than_32 = self.accepted_outside_root_part = self.compound = self.compound_accepted = 0
        self.rejected_topology = self.rejected_rooty_not_bit_identical = self.rejected_topology_lambda_not_bit_identical = self.unchecked = 0
        self.accepted_slides_log_mh_exact = 0
        self.accepted_slide_kinds = [0] * len(self.SLIDE_KINDS)       # accepted slides held to the identity, per SLIDE_KINDS
        self.accepted_spr1_log_mh_exact = 0
        self.accepted_spr1_classes = [0] * len(self.SPR1_CLASSES)     # accepted SPR1 moves held to the identity, per SPR1_CLASSES
        # tests/draws_model.py: moves whose every identity held; the three ways a step may be left out of one; per class
        self.draws_held = self.borderline = self.slope_sign_undetermined = self.position_half_known = self.draws_verdicts_drawn = 0
        self.draws_bexp = [0] * len(DM.BEXP_CLASSES)                  # accepted bounded-exponential draws held, per exact ltr class
        self.draws_bexp_outside_root_part = [0] * len(DM.BEXP_CLASSES)    # ... of them in parts without the run's root (the simple moves are compiled once for each kind of part)
        self.draws_gaussian_root = self.draws_gaussian_slide = self.draws_slide_down_picks = self.draws_grid_cells = 0
        self.draws_reforms = [0] * len(DM.REFORM_SIZES)               # accepted reforms whose new times were held
        self.draws_spr1_times = [0] * len(DM.SPR1_TIMES)
        self.draws_early_end = [0] * len(DM.EARLY)
        self.draws_ends_at_once = [0] * 6     # exact tip, reform of the root, reform of an empty branch: in the root part (the move is called), outside it (settled in the frame)

    def add(self, o):
        for f in self.FIELDS:
            a, b = getattr(self, f), getattr(o, f)
            setattr(self, f, [x + y for x, y in zip(a, b)] if isinstance(a, list) else a + b)

    def as_dict(self):
        return {f: getattr(self, f) for f in self.FIELDS}

    def assert_conditions(self):
        d = self.as_dict()
        assert self.unchecked == 0, d
        assert min(self.accepted) >= 50, d
        assert self.accepted_root_displacements >= 20, d
        assert min(self.accepted_negative_log_mh) >= 20, d
        assert self.accepted_while_grid_grew >= 1, d
        assert self.accepted_reform_same_site_twice >= 1, d
        assert self.accepted_reform_more_than_32 >= 1, d
        assert self.accepted_outside_root_part >= 100, d
        assert self.accepted_slides_log_mh_exact == self.accepted[3], d      # every accepted slide was held to the identity
        assert self.accepted_slides_log_mh_exact >= 1 and min(self.accepted_slide_kinds) >= 1, (dict(zip(self.SLIDE_KINDS, self.accepted_slide_kinds)), d)
        assert self.accepted_spr1_log_mh_exact == self.accepted[4], d        # every accepted SPR1 move was held to the identity
        # what the moves drew (tests/draws_model.py).  The minimums are what the CPU oracle does on test_move_steps.py's cases; a class the
        # oracle reaches a few times asks for one step.  (The bounded exponential's other classes of ltr are test_draws_model.py's.)
        named = lambda names, counts: (dict(zip(names, counts)), d)
        assert self.borderline == 0 and self.slope_sign_undetermined == 0 and self.draws_held == self.steps, d
        assert self.position_half_known == 0, d      # no step was held under the weaker two-readings rule: none of these runs stops a pass for room
        assert self.draws_verdicts_drawn >= 3274, d
        assert self.draws_bexp[2] >= 1582 and self.draws_bexp[3] >= 2282, named(DM.BEXP_CLASSES, self.draws_bexp)
        assert self.draws_gaussian_root == self.accepted_root_displacements and self.draws_gaussian_slide == self.accepted[3], d
        assert self.draws_slide_down_picks >= 1 and self.draws_grid_cells >= 817, d
        assert min(self.draws_reforms) >= 1 and self.draws_reforms[0] >= 576 and self.draws_reforms[4] >= 216, named(DM.REFORM_SIZES, self.draws_reforms)
        assert sum(self.draws_spr1_times) == self.accepted[4] and self.draws_spr1_times[0] >= 173 and self.draws_spr1_times[2] >= 1, named(DM.SPR1_TIMES, self.draws_spr1_times)
        # (no valid part has fewer than 3 nodes; a bounded exponential that lands on a bound is test_draws_model.py's case `on-a-bound`; no
        # SPR1 of any case drew a time that equals an end of its region)
        reached = [c for i, c in enumerate(self.draws_early_end) if i not in (4, 5, 11)]
        assert min(reached) >= 1 and self.draws_early_end[3] >= 3301, named(DM.EARLY, self.draws_early_end)
        assert min(self.draws_ends_at_once) >= 1, d                          # in the root part (a move is called) and outside it (settled in the frame)


class PartWatch:
    """The exact side of one part's chain: the model, the Derived of the tree it holds and its exact k_bar_p, carried from move
    to move (a move's `before` is the last move's `after`)."""

    def __init__(self, p, first, ref, ev, pop, includes_root, tag=""):
        self.p, self.ref, self.ev, self.pop, self.includes_root, self.tag = p, np.asarray(ref), ev, pop, bool(includes_root), tag
        self.dv = X.Derived(first["tree"], ref, ev)
        tab = first["tab"]
        self.kb = X.k_bar_p(self.dv.T, self.includes_root, tab["t_ref"], tab["t_step"], len(tab["k_bar_p"]))[0]
        self.kbf = np.array([abs(float(k)) for k in self.kb])      # |k_bar_p| as floats, for the allowance's kmax
        self.moves = 0          # since k_bar_p was built from scratch
        self.t_max_tip = None   # the run's latest tip time (the studies above the root need it); run_stepped sets it
        self.topology = True    # whether the engine was configured with topology moves (the draw that picks the move spans 32, else 30)
        assert_valid_part(first["tree"], ref)

    def k_allowance(self, tab):
        """check_part's allowance for a maintained k_bar_p after `moves` moves (test_exact_model.py)."""
        kmax = max(1.0, float(self.kbf.max()))
        bmax = (abs(tab["t_ref"]) + len(self.kb) * tab["t_step"]) / tab["t_step"]
        return min(4 * self.moves * X.U * (kmax + bmax), 1e-9 * kmax)


def _slices(tree, x):
    a, b = int(tree.mut_offset[x]), int(tree.mut_offset[x + 1])
    return tree.mut_site[a:b].tolist(), tree.mut_from[a:b].tolist(), tree.mut_to[a:b].tolist(), tree.mut_t[a:b].tolist()


def _same_except(a, b, fields, what, fails, where):
    for f in fields:
        x, y = getattr(a, f), getattr(b, f)
        if not (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y):
            fails.append("%s: %s changed %s" % (where, what, f))


def _bits(x):
    return np.asarray(x, np.float64).tobytes()


def check_step(tally, cov, w: PartWatch, step, b, a):
    """One move of part w.p: `b` and `a` are snapshots before and after it.  Failures go to tally.fail; a step that could not be
    checked counts in cov.unchecked (and is a failure)."""
    where = "%s part %d step %d" % (w.tag, w.p, step)
    fails = tally.fail
    n0 = len(fails)
    cov.steps += 1
    w.moves += 1
    tb, ta, tabb, taba = b["tree"], a["tree"], b["tab"], a["tab"]
    try:
        if a["stats"]["status"] != 0 or a["stats"]["moves_done"] != b["stats"]["moves_done"] + 1 or a["trace_len"] != b["trace_len"] + 1:
            fails.append("%s: status %d, moves_done %d -> %d, trace %d -> %d rows" % (where, a["stats"]["status"], b["stats"]["moves_done"], a["stats"]["moves_done"], b["trace_len"], a["trace_len"]))
            cov.unchecked += 1
            return
        kind, node, acc, log_mh = int(a["row"][0]), int(a["row"][1]), a["row"][2] == 1.0, float(a["row"][3])
        if not (0 <= kind < 5 and a["row"][2] in (0.0, 1.0)):
            fails.append("%s: trace row %s" % (where, a["row"])); cov.unchecked += 1
            return
        where += " (%s of node %d, %s, log_mh %r)" % (KINDS[kind], node, "accepted" if acc else "not accepted", log_mh)
        compound = kind == 2 and w.includes_root and node >= 0 and node != tb.root and int(tb.parent[node]) == tb.root
        DM.check_draws(tally, cov, DM.Step(w, b, a, kind, node, log_mh == log_mh, acc, log_mh, compound, 32.0 if w.topology else 30.0, w.topology), where)
        dp = [y - x for x, y in zip(b["stats"]["proposed"], a["stats"]["proposed"])]
        da = [y - x for x, y in zip(b["stats"]["accepted"], a["stats"]["accepted"])]
        if dp != [int(k == kind) for k in range(5)] or da != [int(k == kind and acc) for k in range(5)]:
            fails.append("%s: proposed rose by %s, accepted by %s" % (where, dp, da))
        if acc and not (log_mh == log_mh):
            fails.append("%s: accepted with a NaN log_mh" % where)
        grew = len(taba["k_bar_p"]) - len(tabb["k_bar_p"])
        if grew < 0 or (grew and not w.includes_root):
            fails.append("%s: the grid went from %d to %d cells" % (where, len(tabb["k_bar_p"]), len(taba["k_bar_p"])))
        if grew > 0:
            w.kb.extend([F(1)] * grew)          # appended cells hold the lineage above the root and nothing else
            w.kbf = np.concatenate([w.kbf, np.ones(grew)])
        nb = len(tabb["k_bar_p"])

        if not acc and not compound:
            if kind >= 3:
                cov.rejected_topology += 1
            if _bits(a["G"]) != _bits(b["G"]) or _bits(a["A"]) != _bits(b["A"]):
                fails.append("%s: totals changed: log_G %r -> %r, log_aug_prior %r -> %r" % (where, b["G"], a["G"], b["A"], a["A"]))
            if _bits(taba["k_bar_p"][:nb]) != _bits(tabb["k_bar_p"]) or not np.all(taba["k_bar_p"][nb:] == 1.0):
                fails.append("%s: k_bar_p changed" % where)
            if kind >= 3:       # a pruned subtree goes back under its old parent, in either of its two slots
                _same_except(tb, ta, tuple(f for f in _TOPO if f not in ("child0", "child1")) + _MUT, "a move that was not accepted", fails, where)
                if not (np.array_equal(np.minimum(ta.child0, ta.child1), np.minimum(tb.child0, tb.child1)) and np.array_equal(np.maximum(ta.child0, ta.child1), np.maximum(tb.child0, tb.child1))):
                    fails.append("%s: a move that was not accepted changed a node's children" % where)
            else:
                _same_except(tb, ta, _TOPO + _MUT, "a move that was not accepted", fails, where)
            if _bits(ta.t) != _bits(tb.t):
                fails.append("%s: node times changed" % where)
            rooty = kind >= 3 and w.includes_root and node >= 0 and node != tb.root and int(tb.parent[node]) == tb.root
            if rooty and (_bits(ta.mut_t) != _bits(tb.mut_t) or _bits(a["lam"]) != _bits(b["lam"])):
                # pruned from under the run's root: the sibling's mutations were reflected about the root's time and back,
                # t -> t_P - (t - t_P) -> t_P + (t_P - t'), four roundings; and the root's lambda was recomputed from its child's
                root = tb.root
                S = int(tb.child1[root]) if int(tb.child0[root]) == node else int(tb.child0[root])
                lo, hi = int(tb.mut_offset[S]), int(tb.mut_offset[S + 1])
                keep = np.ones(tb.mut_t.shape[0], bool); keep[lo:hi] = False
                tP = float(tb.t[root])
                if ta.mut_t[keep].tobytes() != tb.mut_t[keep].tobytes() or \
                        not np.all(np.abs(ta.mut_t[lo:hi] - tb.mut_t[lo:hi]) <= 4 * X.U * (abs(tP) + np.abs(tb.mut_t[lo:hi] - tP))):
                    fails.append("%s: mutation times changed beyond the sibling's reflection about the root" % where)
                other = np.ones(tb.num_nodes, bool); other[root] = False
                if a["lam"][other].tobytes() != b["lam"][other].tobytes() or not np.array_equal(a["nsm"], b["nsm"]):
                    fails.append("%s: lambda_i changed below the root" % where)
                tally.check("lambda_root_after_rejected_move", w.dv.lambda_i(root), a["lam"][root], where)
                w.dv = w.dv.retimed(ta)
                cov.rejected_rooty_not_bit_identical += 1
                return
            if _bits(ta.mut_t) != _bits(tb.mut_t):
                fails.append("%s: mutation times changed" % where)
            if not np.array_equal(a["nsm"], b["nsm"]):
                fails.append("%s: num_sites_missing changed" % where)
            if _bits(a["lam"]) != _bits(b["lam"]):
                if kind < 3:
                    fails.append("%s: lambda_i changed" % where)
                else:       # hopping the pruned subtree up and down the tree recomputes the lambda of the nodes it passes
                    cov.rejected_topology_lambda_not_bit_identical += 1
                    for x in np.flatnonzero(a["lam"] != b["lam"]).tolist():
                        tally.check("lambda_i_after_rejected_move", w.dv.lambda_i(x), a["lam"][x], "%s node %d" % (where, x))
            if len(fails) > n0:
                w.dv = X.Derived(ta, w.ref, w.ev)
            return

        # ---- the state changed (or may have: an accepted branch reform of a branch without mutations changes nothing) --------
        simple = kind <= 2 and not compound
        if simple:
            # locality first: the exact side then re-reads only the times
            _same_except(tb, ta, _TOPO, "a %s" % KINDS[kind], fails, where)
            if _bits(a["lam"]) != _bits(b["lam"]) or not np.array_equal(a["nsm"], b["nsm"]):
                fails.append("%s: lambda_i or num_sites_missing changed" % where)
            if kind <= 1:
                _same_except(tb, ta, _MUT, "a displacement", fails, where)
                if _bits(ta.mut_t) != _bits(tb.mut_t):
                    fails.append("%s: a displacement changed mutation times" % where)
                diff = np.flatnonzero(ta.t != tb.t).tolist()
                if diff != [node]:
                    fails.append("%s: node times changed at %s" % (where, diff))
                if (ta.child0[node] < 0) != (kind == 1):
                    fails.append("%s: node %d is %s" % (where, node, "a tip" if ta.child0[node] < 0 else "an inner node"))
            else:
                if _bits(ta.t) != _bits(tb.t):
                    fails.append("%s: a branch reform changed node times" % where)
                lo, hi = int(tb.mut_offset[node]), int(tb.mut_offset[node + 1])
                keep = np.ones(tb.mut_t.shape[0], bool); keep[lo:hi] = False
                for f in _MUT + ("mut_t",):
                    if getattr(ta, f)[keep].tobytes() != getattr(tb, f)[keep].tobytes():
                        fails.append("%s: a branch reform changed %s of another branch" % (where, f))
                sb_, fb_, ob_, _ = _slices(tb, node)
                sa_, fa_, oa_, _ = _slices(ta, node)
                if sorted(zip(sb_, fb_, ob_)) != sorted(zip(sa_, fa_, oa_)):
                    fails.append("%s: the branch's mutations changed as a multiset of (site, from, to)" % where)
                for l in set(sb_):
                    if [(f, o) for s, f, o in zip(sb_, fb_, ob_) if s == l] != [(f, o) for s, f, o in zip(sa_, fa_, oa_) if s == l]:
                        fails.append("%s: the mutations of site %d changed their order" % (where, l))
                if len(set(sb_)) < len(sb_):
                    cov.accepted_reform_same_site_twice += 1
                if len(sb_) > 32:
                    cov.accepted_reform_more_than_32 += 1
            if len(fails) > n0:
                cov.unchecked += 1          # the exact side below relies on the locality just refuted
                w.dv = X.Derived(ta, w.ref, w.ev)
                w.kb = X.k_bar_p(w.dv.T, w.includes_root, taba["t_ref"], taba["t_step"], len(taba["k_bar_p"]))[0]
                w.kbf = np.array([abs(float(k)) for k in w.kb])
                return
            dvA = w.dv.retimed(ta)
        else:
            dvA = X.Derived(ta, w.ref, w.ev)
            tally.equal("num_sites_missing", a["nsm"], dvA.nsm, where)
        assert_valid_part(ta, w.ref)

        dG = X.part_log_G_delta(w.dv, dvA, w.ref, w.ev, w.includes_root)
        dP = X.partial_log_prior_delta(w.dv.T, dvA.T, w.pop, w.includes_root, taba)
        for i, (kB, kA) in dP.cells.items():
            if w.kb[i] != kB:
                fails.append("%s: the exact k_bar_p carried from move to move is off at cell %d" % (where, i)); cov.unchecked += 1
            w.kb[i] = kA; w.kbf[i] = abs(float(kA))
        k_term = float(dP.k_sensitivity) * w.k_allowance(taba)

        # the increments of the maintained totals, all five kinds
        tally.check("increment_log_G", dG, F(a["G"]) - F(b["G"]), where, 2 * X.U * max(abs(b["G"]), abs(a["G"])))
        tally.check("increment_log_aug_prior", dP, F(a["A"]) - F(b["A"]), where, 2 * X.U * max(abs(b["A"]), abs(a["A"])) + k_term)

        if compound:
            cov.compound += 1
            cov.compound_accepted += int(acc)
        elif kind <= 1:
            root_move = node == tb.root
            if root_move:
                cov.accepted_root_displacements += 1
                ex = X.Exact(dG.value + dP.value, dG.S + dP.S, dG.n + dP.n)
                tally.check("log_mh_root_displace", ex, log_mh, where, k_term)
            else:
                slope = X.displacement_slope(w.dv, node)
                lin = slope * (F(float(ta.t[node])) - F(float(tb.t[node])))
                if dG.value != lin:
                    fails.append("%s: log G is not linear in the node's time: exact difference %r, slope x step %r" % (where, float(dG.value), float(lin)))
                ex = X.Exact(dP.value, dP.S + 2 * abs(lin), dP.n + 2)
                tally.check("log_mh_%s" % KINDS[kind], ex, log_mh, where, k_term)
        elif kind == 2:
            tally.check("log_mh_branch_reform", dG, log_mh, where)
            if dP.cells or dP.value != 0 or _bits(a["A"]) != _bits(b["A"]) or _bits(taba["k_bar_p"]) != _bits(tabb["k_bar_p"]):
                fails.append("%s: a branch reform touched the prior or k_bar_p" % where)
        elif kind == 3 and acc:
            check_accepted_slide(tally, cov, w, node, dvA, dP, k_term, log_mh, where)
        elif kind == 4 and acc:
            check_accepted_spr1(tally, cov, w, node, dvA, dP, k_term, log_mh, b["rng"], where)
        # (a topology move that was not accepted leaves no second state to read its proposed history from: the increments are checked above)

        if acc:
            cov.accepted[kind] += 1
            if simple and log_mh < 0.0:
                cov.accepted_negative_log_mh[kind] += 1
            if grew > 0:
                cov.accepted_while_grid_grew += 1
            if not w.includes_root:
                cov.accepted_outside_root_part += 1
        w.dv = dvA
    except AssertionError as e:
        fails.append("%s: %s" % (where, e))
        cov.unchecked += 1


straddling_branches = DM.straddling_branches     # (the one derivation: a slide's alpha_ratio here, its pick of the new sibling there)


def slide_alpha_ratio(B, A, Xn):
    """(alpha_ratio, kind, n) of the subtree slide that took tree B to tree A (exact_model._Tree) by moving X: from the tree before,
    X and the new time of X's parent.  kind: "same", "up" or "down"; n: the branches the slide chose among on its way back (up) or
    there (down)."""
    P = B.parent[Xn]
    assert P >= 0 and A.parent[Xn] == P, "X's parent is another node"
    S = [k for k in B.kids[P] if k != Xn][0]
    SS = [k for k in A.kids[P] if k != Xn][0]
    old_t, new_t = B.t[P], A.t[P]

    straddling = lambda top, t: straddling_branches(B, top, t, Xn)
    if SS == S:
        G = B.parent[P]
        assert new_t < min(B.t[Xn], B.t[S]) and (G < 0 or B.t[G] <= new_t), "the new time is not on the branch above X's sibling"
        return F(1), "same", 1
    anc, v = [], B.parent[P]
    while v >= 0:
        anc.append(v); v = B.parent[v]
    if SS in anc:
        G = B.parent[SS]
        assert new_t < B.t[SS] and (G < 0 or B.t[G] <= new_t), "the new time is not on the branch above the ancestor"
        n = len(straddling(SS, old_t))
        assert P in straddling(SS, old_t)
        return F(1, n), "up", n
    br = straddling(P, new_t)
    assert SS in br and new_t > B.t[S], "the new sibling does not straddle the new time below P"
    return F(len(br)), "down", len(br)


def check_accepted_slide(tally, cov, w, Xn, dvA, dP, k_term, log_mh, where):
    """The identity of an accepted subtree slide (the module's docstring)."""
    B, A = w.dv.T, dvA.T
    ratio, kind, n = slide_alpha_ratio(B, A, Xn)
    lam = w.dv.lambda_i(B.root)
    sites = len(w.ref) - w.dv.nsm[B.root]
    mu, mu_S, mu_n = lam.value / sites, lam.S / sites, lam.n + 1
    gb = GM.GraftModel(w.dv, w.ref, w.ev, w.includes_root).graft(Xn)
    ga = GM.GraftModel(dvA, w.ref, w.ev, w.includes_root).graft(Xn)
    terms = [ga.delta_log_G, ga.log_alpha_mut(mu), gb.delta_log_G, gb.log_alpha_mut(mu)]
    # mu is itself computed: its own bound (mu_n + 8) u mu_S, times what an error of mu moves the two log_alpha_mut by
    mu_term = (mu_n + 8) * X.U * float(mu_S * (ga.mu_sensitivity(mu) + gb.mu_sensitivity(mu)))
    lr = X._log(ratio)
    v = (terms[0].value - terms[1].value) - (terms[2].value - terms[3].value) + lr + dP.value
    S = sum((t.S for t in terms), dP.S + abs(lr))
    bound = sum(t.bound() for t in terms) + mu_term + dP.bound() + k_term + 8 * X.U * abs(float(lr))
    ex = X.Exact(v, S, 0)
    tally.check("log_mh_subtree_slide", ex, log_mh, "%s [%s, n %d]" % (where, kind, n), bound - ex.bound())
    cov.accepted_slides_log_mh_exact += 1
    rooty = w.includes_root and (B.parent[Xn] == B.root or A.parent[Xn] == A.root)
    for i, hit in enumerate((kind == "same", kind == "up" and n >= 2, kind == "down" and n >= 2, rooty, not w.includes_root)):
        cov.accepted_slide_kinds[i] += int(hit)


def scan_limit_from_stream(rng, mix_total=32.0):
    """The scan limit of the SPR1 move that starts at stream position `rng` (a part_rng() dict read BEFORE the move): None for an unlimited
    scan, 1 otherwise.  The move's first word through mix_draw (emat_device_moves.hpp: 0.0 + (mix_total - 0.0) * to_co(word)) must say SPR1,
    r >= 31 of 32 with topology moves on; its second through to_co is the chooser (subrun.cpp:497-498: < 0.01 scans without a limit)."""
    if rng["has_spare"] is None:            # (stream_position could not say: the two readings must agree, and one of them must say SPR1)
        out = set()
        for hs in (False, True):
            try:
                out.add(scan_limit_from_stream(dict(rng, has_spare=hs, spare=None), mix_total))
            except AssertionError:
                pass
        assert len(out) == 1, "the stream's position is known to a half block only, and the two readings give %s" % sorted(map(str, out))
        return out.pop()
    try:
        W = DM.Words(rng)           # (the one reader of the stream: draws_model holds the rest of the move's words to their identities)
    except DM.Mismatch as e:
        raise AssertionError(str(e))
    assert DM.kind_of(W[0], mix_total) == 4, "the move's first draw does not pick SPR1"
    return None if DM.to_co(W[1]) < F(0.01) else 1


def spr1_identity(w, Xn, dvA, limit):
    """The pieces of an accepted SPR1's identity from the trees before (w.dv) and after (dvA): dict(grafts, mu, mu_term, o2n, n2o, lam,
    pre, post, new_region, old_region)."""
    B, A = w.dv.T, dvA.T
    lam = w.dv.lambda_i(B.root)
    sites = len(w.ref) - w.dv.nsm[B.root]
    mu, mu_S, mu_n = lam.value / sites, lam.S / sites, lam.n + 1
    gmb, gma = GM.GraftModel(w.dv, w.ref, w.ev, w.includes_root), GM.GraftModel(dvA, w.ref, w.ev, w.includes_root)
    gb, ga = gmb.graft(Xn), gma.graft(Xn)
    prb, pra = SM.Pruned(gmb, Xn), SM.Pruned(gma, Xn)
    prb.same_as(pra)
    lamX = w.dv.lambda_i(Xn)
    assert lamX.value == dvA.lambda_i(Xn).value, "lambda of X changed"
    pre = SM.Study(prb, w.includes_root, limit, lamX, w.t_max_tip)          # scanned from the old sibling
    post = SM.Study(pra, w.includes_root, limit, lamX, w.t_max_tip)         # scanned from the new sibling
    new_region = pre.find(ga.S, ga.t_P)
    old_region = post.find(gb.S, gb.t_P)
    assert new_region >= 0, "the new nexus (sibling %d, t_P %r) lies in no region of the study scanned from the old sibling" % (ga.S, ga.t_P)
    assert old_region >= 0, "the old nexus (sibling %d, t_P %r) lies in no region of the study scanned from the new sibling" % (gb.S, gb.t_P)
    o2n, n2o = pre.log_alpha(new_region, ga.t_P), post.log_alpha(old_region, gb.t_P)
    # emat_device_moves.hpp:555-556, restated
    assert pre.regions[new_region].m == sum(bi.d for bi in ga.infos if not bi.is_open), "min_muts of the new region is not the new graft's"
    assert post.regions[old_region].m == sum(bi.d for bi in gb.infos if not bi.is_open), "min_muts of the old region is not the old graft's"
    mu_term = (mu_n + 8) * X.U * float(mu_S * (ga.mu_sensitivity(mu) + gb.mu_sensitivity(mu)))
    return dict(gb=gb, ga=ga, mu=mu, mu_term=mu_term, o2n=o2n, n2o=n2o, lam=lamX, pre=pre, post=post, new_region=new_region, old_region=old_region)


def check_accepted_spr1(tally, cov, w, Xn, dvA, dP, k_term, log_mh, rng_before, where):
    """The identity of an accepted SPR1 move (the module's docstring)."""
    assert w.t_max_tip is not None, "the watch does not know the run's latest tip time"
    limit = scan_limit_from_stream(rng_before)
    d = spr1_identity(w, Xn, dvA, limit)
    ga, gb, mu, o2n, n2o, lam = d["ga"], d["gb"], d["mu"], d["o2n"], d["n2o"], d["lam"]
    terms = [ga.delta_log_G, ga.log_alpha_mut(mu), gb.delta_log_G, gb.log_alpha_mut(mu)]
    lam_term = (lam.n + 8) * X.U * float(lam.S / lam.value) * (o2n.lambda_sensitivity + n2o.lambda_sensitivity)
    gamma_term = o2n.gamma_term + n2o.gamma_term
    tag = "%s [%s scan, %d and %d regions, new region %s]" % (where, "unlimited" if limit is None else "limit 1", len(d["pre"].regions), len(d["post"].regions), o2n.branch_kind)
    # the study's half on its own ...
    sv = n2o.exact.value - o2n.exact.value
    # ... and the whole
    v = (terms[0].value - terms[1].value) - (terms[2].value - terms[3].value) + sv + dP.value
    S = sum((t.S for t in terms), dP.S + n2o.exact.S + o2n.exact.S)
    bound = sum(t.bound() for t in terms) + d["mu_term"] + dP.bound() + k_term + n2o.exact.bound() + o2n.exact.bound() + gamma_term + lam_term
    ex = X.Exact(v, S, 0)
    tally.check("log_mh_spr1", ex, log_mh, tag, bound - ex.bound())
    # what is left of log_mh when the exact graft and prior terms are taken away is the engine's log_alpha_n2o - log_alpha_o2n
    rest = F(log_mh) - ((terms[0].value - terms[1].value) - (terms[2].value - terms[3].value) + dP.value)
    exs = X.Exact(sv, n2o.exact.S + o2n.exact.S, 0)
    tally.check("spr1_log_alpha_n2o_less_o2n", exs, rest, tag, bound - exs.bound())
    for what, e, val in (("log_mh_spr1", ex, log_mh), ("spr1_log_alpha_n2o_less_o2n", exs, rest)):     # how close the worst comes to its bound
        k = what + " (share of its bound)"
        tally.worst[k] = max(tally.worst.get(k, 0.0), e.err(val) / bound)
    cov.accepted_spr1_log_mh_exact += 1
    DM.check_spr1_time(tally, cov, w, Xn, d, limit, rng_before, tag)
    B = w.dv.T
    new_r, old_r = d["pre"].regions[d["new_region"]], d["post"].regions[d["old_region"]]
    nreg = max(len(d["pre"].regions), len(d["post"].regions))
    hits = (limit is None, new_r.above_root and o2n.branch_kind == "gamma", new_r.above_root and o2n.branch_kind == "power", old_r.above_root,
            not w.includes_root, new_r.m >= 1, new_r.uncounted >= 1, nreg > 64, nreg > 640)
    for i, hit in enumerate(hits):
        cov.accepted_spr1_classes[i] += int(bool(hit))
    return d


def run_stepped(tally, cov, engine, sc, parts, incl, ref, ev, pop, steps, tag="", watch=None, advance=advance_one_move, topology=True):
    """Step a configured engine `steps` times and check every move of the watched parts (default: all)."""
    ids = list(range(len(parts))) if watch is None else list(watch)
    if hasattr(engine, "synchronize"):
        engine.synchronize()
    watches = {}

    def on_step(p, s, before, after):
        if p not in watches:
            watches[p] = PartWatch(p, before, ref, ev, pop, incl[p], tag)
            watches[p].t_max_tip, watches[p].topology = sc.t_max_tip, topology
        check_step(tally, cov, watches[p], s, before, after)
    step_chain(engine, ids, steps, on_step, advance)
    return watches
