"""Hand-built inputs for the initial-tree builder (delphy_amd/csrc/emat_build.hpp) and the host-side account of which
size class of the graft step an input selects.  No scenario generator: tip descriptors are written from explicit site lists, and a
seeded numpy generator only fills in what does not matter (the reference sequence, private sites).

Blocks (lists of tips; a tip is dict(t=date, deltas={site: state}, miss=[(start, end), ...])):
  ladder   tip k carries rungs 0 .. k and is dated later than tip k - 1; its cheapest place is the lowest region of tip k - 1's branch (every
           other region lacks at least one more of its sites), so the tree grows one node deeper per tip and tip X is grafted with
           np = X, T = the sites of rungs 0 .. X - 1, nsd = its last rung + its private deltas
  stem     tips equal to the reference sequence: dxn = 0 = the distance at the root, and the reference picks above the root whenever it ties,
           so every such tip becomes the new root's child and tip 0 sinks one node per tip WITHOUT a mutation on the way: a deep path
           with T as small as wanted
  veiled   a tip that misses the sites a path mutates: the distance does not count them, the composition of its deltas does
  bush     tips with one and the same sequence, dated later and later: every region below the shared mutation ties
  fat tip  many private deltas and many missing intervals, on top of some other tip's sequence

`graft_facts` reads (np, T, dxn, mxn, nsd, above the root) of the LAST graft off the oracle's tree of a prefix of the descriptors."""
import dataclasses

import numpy as np

import delphy_amd as d
from oracle_ffi import OracleBuild

FIELDS = ("parent", "child0", "child1", "t", "t_min", "t_max", "mut_offset", "mut_site", "mut_from", "mut_to", "mut_t",
          "miss_offset", "miss_start", "miss_end", "mfs_offset", "mfs_site", "mfs_state")


def compare_builds(ref, tips, seed, want=None):
    """The device's tree for (descriptors, seed) against the oracle's (`want`: the oracle's tree when the caller already has it): the root
    and every field bit for bit, then the reference's closing checks of the builder.  Returns (device tree, oracle tree)."""
    ob = OracleBuild(ref)
    b = d.EmatBackend(int(len(ref)))
    try:
        b.set_ref_sequence(ref)
        got = b.build_usher_like(tips, seed)
        if want is None:
            want = ob.build_usher_like(tips, seed)
        assert got.root == want.root
        for f in FIELDS:
            x, y = getattr(got, f), getattr(want, f)
            assert x.shape == y.shape and np.array_equal(x, y), "%s differs (seed %d)" % (f, seed)
        rc, msg = ob.check(got, tips)
        assert rc == 0, msg
        return got, want
    finally:
        b.close(); ob.close()


def build_both(sc, seed):
    """A scenario's tips through both builders (compare_builds).  Returns (device tree, descriptors)."""
    ob = OracleBuild(sc.ref)
    try:
        tips = ob.tip_descs_of(sc.tree)
    finally:
        ob.close()
    got, _ = compare_builds(sc.ref, tips, seed)
    return got, tips


# ---- descriptors from numpy arrays ------------------------------------------------------------------------------------------

def make_ref(L, seed=20261019):
    return np.random.default_rng(seed).integers(0, 4, size=L, dtype=np.uint8)


def alt(ref, sites, k=1):
    """{site: a state that differs from the reference sequence's} (k = 1, 2, 3 picks which)."""
    return {int(s): int((int(ref[s]) + k) % 4) for s in sites}


def tip(t, deltas=None, miss=()):
    return dict(t=float(t), deltas=dict(deltas or {}), miss=[(int(s), int(e)) for s, e in miss])


def write_descs(ref, tips):
    """delphy_amd.TipDescs of a list of tips, dates exact (t_min = t_max)."""
    n = len(tips)
    t = np.array([x["t"] for x in tips], np.float32)
    assert np.array_equal(t.astype(np.float64), [x["t"] for x in tips]), "dates must be exact in float32"
    doff, moff = np.zeros(n + 1, np.int32), np.zeros(n + 1, np.int32)
    dsite, dto, ms, me = [], [], [], []
    for i, x in enumerate(tips):
        sites = sorted(x["deltas"])
        miss = sorted(x["miss"])
        for s in sites:
            assert 0 <= s < len(ref) and x["deltas"][s] != ref[s] and not any(a <= s < e for a, e in miss), (i, s)
        for (a, e), (a2, _) in zip(miss, miss[1:]):
            assert a < e < a2, (i, a, e, a2)
        dsite += sites; dto += [x["deltas"][s] for s in sites]
        ms += [a for a, _ in miss]; me += [e for _, e in miss]
        doff[i + 1] = len(dsite); moff[i + 1] = len(ms)
    return d.TipDescs(t, t.copy(), doff, np.array(dsite, np.int32), np.array(dto, np.uint8), moff, np.array(ms, np.int32), np.array(me, np.int32))


def head_of(tips, k):
    """The first k descriptors."""
    dh, mh = int(tips.delta_offset[k]), int(tips.miss_offset[k])
    return d.TipDescs(tips.t_min[:k].copy(), tips.t_max[:k].copy(), tips.delta_offset[: k + 1].copy(), tips.delta_site[:dh].copy(), tips.delta_to[:dh].copy(),
                      tips.miss_offset[: k + 1].copy(), tips.miss_start[:mh].copy(), tips.miss_end[:mh].copy())


class Sites:
    """Hands out sites nobody has used yet.  Sites 100 j + 40 .. 100 j + 59 are kept for missing intervals (`gap`), the others go to deltas."""

    def __init__(self, L, seed=7):
        free = np.array([s for s in range(L) if not 40 <= s % 100 < 60], np.int64)
        self.free = list(np.random.default_rng(seed).permutation(free))

    def take(self, count):
        out, self.free = self.free[:count], self.free[count:]
        assert len(out) == count, "out of sites"
        return sorted(int(s) for s in out)

    @staticmethod
    def gap(j):
        """The j-th missing interval: lengths 1 .. 17, never adjacent to the next."""
        return (100 * j + 40, 100 * j + 41 + j % 17)


def ladder(ref, rungs, t0=1000.0, dt=10.0, k=1):
    """Tip i carries rungs 0 .. i (`rungs`: one list of sites per tip)."""
    out, have = [], {}
    for i, r in enumerate(rungs):
        have.update(alt(ref, r, k))
        out.append(tip(t0 + dt * i, have))
    return out


def stem(count, t0=1000.0, dt=10.0):
    return [tip(t0 + dt * i) for i in range(count)]


def fat_tip(ref, sites, base, t, num_deltas=None, private=0, num_miss=0):
    """`base`'s deltas where the tip has data, private deltas (`private` of them, or up to num_deltas in all), missing intervals
    gap(0) .. gap(num_miss - 1)."""
    miss = [Sites.gap(j) for j in range(num_miss)]
    assert not miss or miss[-1][1] <= len(ref)
    keep = {s: v for s, v in base.items() if not any(a <= s < e for a, e in miss)}
    if num_deltas is not None:
        private = num_deltas - len(keep)
    assert private >= 0
    keep.update(alt(ref, sites.take(private), 2))
    return tip(t, keep, miss)


# ---- which branch a case takes ----------------------------------------------------------------------------------------------

@dataclasses.dataclass
class GraftFacts:
    X: int
    dxn: int            # the tip's deltas against the reference sequence
    mxn: int            # its missing intervals
    above_root: bool
    S: int              # the node it was hung above
    np: int             # nodes from S up to the root, S and the root included (0 above the root)
    T: int              # mutations on that path with t_root <= t <= t_P
    T_sites: int        # ... distinct sites among them (< T: some site mutates twice on the way down)
    max_path_site: int  # the largest of them (-1: none)
    nsd: int            # the tip's new mutations as the graft step writes them (before fix_up_missations)
    tree: object        # the oracle's tree of the prefix


def graft_facts(ob, tips, seed, X):
    """What the graft of tip X looked like, from the oracle's tree over descriptors 0 .. X (OracleBuild.build_usher_like): the tree a
    builder holds just after that graft, up to the closing passes.  Those re-time nodes and mutations and drop mutations at missing sites, but
    move no mutation to another branch and keep a site's mutations in order, so
      np   = the ancestors of P = X + n - 1 plus S (P itself was not there yet), P's sibling-to-be;
      T    = the mutations on P's branch (the part of S's branch above t_P) and on every branch above it (the root has none while building);
      nsd  = the sites at which the sequence at P differs from the tip's, the tip standing at the reference state where it has no delta,
             missing or not: what the composition of the deltas leaves, whatever fix_up_missations removes afterwards.
    T and nsd hold when no mutation on the path was dropped, i.e. no site is missing in BOTH subtrees of a node on the path: the cases that
    assert T or nsd put missing intervals on one tip only (the bush with q and the pool case read dxn and the topology).  The tip dates are drawn before the first graft, one per tip, so a prefix consumes the stream
    differently from the whole input: the facts are those of the whole build when X is the last tip (every case here), and otherwise
    where they do not depend on a draw (a ladder: one tying region per tip)."""
    n = X + 1
    ref = ob.ref
    head = head_of(tips, n) if tips.num_tips != n else tips
    tr = ob.build_usher_like(head, seed)
    dxn = int(head.delta_offset[n] - head.delta_offset[X]); mxn = int(head.miss_offset[n] - head.miss_offset[X])
    P = X + n - 1
    assert int(tr.parent[X]) == P and int(tr.child0[P]) == X
    S = int(tr.child1[P])
    if tr.root == P:
        return GraftFacts(X, dxn, mxn, True, S, 0, 0, 0, -1, dxn, tr)
    path = []
    v = P
    while v != -1:
        path.append(v); v = int(tr.parent[v])
    seq, T = {}, 0                                                     # the sequence at P where a mutation on the path touched it
    for v in reversed(path):                                           # root first
        for k in range(int(tr.mut_offset[v]), int(tr.mut_offset[v + 1])):
            s = int(tr.mut_site[k])
            assert int(tr.mut_from[k]) == seq.get(s, int(ref[s])), "mutation chain broken at site %d" % s
            seq[s] = int(tr.mut_to[k]); T += 1
    lo, hi = int(head.delta_offset[X]), int(head.delta_offset[n])
    xstate = dict(zip(head.delta_site[lo:hi].tolist(), head.delta_to[lo:hi].tolist()))
    nsd = sum(1 for s in set(seq) | set(xstate) if seq.get(s, int(ref[s])) != xstate.get(s, int(ref[s])))
    if mxn == 0:                                                       # nothing for fix_up_missations to drop on the tip's own branch
        assert nsd == int(tr.mut_offset[X + 1] - tr.mut_offset[X])
    return GraftFacts(X, dxn, mxn, False, S, len(path), T, len(seq), max(seq) if seq else -1, nsd, tr)


def bush(ref, y, count, q=None, t0=1000.0, dt=10.0):
    """`count` tips that carry the one delta y, dated later and later.  With q: tip 2 also carries q, and every later tip misses q -- one more
    mutation in the tree that no later tip's distance sees, i.e. one more tying region."""
    out = [tip(t0 + dt * i, alt(ref, [y])) for i in range(count)]
    if q is not None:
        out[2]["deltas"].update(alt(ref, [q]))
        for x in out[3:]:
            x["miss"] = [(q, q + 1)]
    return out


def bush_account(tree, tips, y):
    """The tying regions the LAST tip X of a bush met, counted on the oracle's finished tree with X and its inner node P taken out again (P's
    mutations are the part of S's branch above t_P): a region is a stretch of a branch between mutations, it ties when the sequence there
    has the bush's state at y (distance 0; nothing else in a bush changes a later tip's distance), and every region starts before X's date.
    By construction that is every region but the two above the tree's two y mutations: 2 X - 2 over X tips, 2 X - 1 with the q mutation.
    Returns (n_tie, the index of the region drawn in visiting order: pre-order, the second child first).  The graft makes P the FIRST child
    of S's parent G whichever S was, but which child S had been follows from the node numbers: a graft on a branch below G puts its new
    inner node (numbered after G) first, so the first child before this graft was the one of S and its sibling made last, and with
    neither made after G, the tip G was made for (tip 0 under the first root)."""
    n = tips.num_tips; X = n - 1; P = X + n - 1
    assert int(tree.parent[X]) == P and tree.root != P
    S, G = int(tree.child1[P]), int(tree.parent[P])
    U = int(tree.child1[G]); assert int(tree.child0[G]) == P
    lo, hi = int(tips.delta_offset[X]), int(tips.delta_offset[n])
    assert hi - lo == 1 and int(tips.delta_site[lo]) == y
    y_to = int(tips.delta_to[lo])
    assert np.all(np.diff(tips.t_min) > 0)
    def muts(v):
        r = list(range(int(tree.mut_offset[v]), int(tree.mut_offset[v + 1])))
        return list(range(int(tree.mut_offset[P]), int(tree.mut_offset[P + 1]))) + r if v == S else r
    born = lambda w: w if w >= n and w > G else -1
    first = (S if born(S) > born(U) else U) if born(S) != born(U) else (0 if G == n else G - (n - 1))
    assert first in (S, U)
    total, chosen = 0, None
    stack = [(int(tree.root), False)]
    while stack:
        v, has = stack.pop()
        if v != tree.root:
            ks = muts(v)
            for j in range(len(ks) + 1):
                if v == S and j == int(tree.mut_offset[P + 1] - tree.mut_offset[P]):
                    assert has; chosen = total
                total += 1 if has else 0
                if j < len(ks) and int(tree.mut_site[ks[j]]) == y:
                    has = int(tree.mut_to[ks[j]]) == y_to
        if int(tree.child0[v]) != -1:
            a, b = int(tree.child0[v]), int(tree.child1[v])
            if v == G: a, b = (S, U) if first == S else (U, S)
            stack.append((a, has)); stack.append((b, has))                # (b, the second child, is visited first)
    return total, chosen
