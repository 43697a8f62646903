// emat_run_tree.hpp -- the run driver's host tree model: the node records (HTree) and what is done on them -- Run::normalize_root
// (core/run.cpp:258-265), the state at the cut points and the subtrees of the parts (Run::repartition, :131-184), and the gather of the
// parts back into the tree (Run::reassemble, :195-256).
//
// Included by emat_run.cpp after emat_run_partition.hpp (whose Topology, PartMap and PartKids it uses).
#ifndef EMAT_RUN_TREE_HPP_
#define EMAT_RUN_TREE_HPP_

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <limits>
#include <map>
#include <stdexcept>
#include <vector>

#include "emat_run_partition.hpp"
#include "flat_tree.hpp"

namespace emat {

struct HMut { double t; int32_t site; uint8_t from, to; };
struct HIv { int32_t start, end; };
struct HFs { int32_t site; uint8_t state; };
struct HNode {
  int32_t parent = EMAT_NO_NODE, c0 = EMAT_NO_NODE, c1 = EMAT_NO_NODE;
  float t_min = -FLT_MAX, t_max = FLT_MAX;
  double t = 0.0;
  std::vector<HMut> muts; std::vector<HIv> miss; std::vector<HFs> mfs;
  bool is_tip() const { return c0 == EMAT_NO_NODE; }
  // THE per-node spelling of the three lists of a flat tree, in both directions (V: emat_flat_tree or FlatTree -- pointers or vectors).
  template <class V> void take_lists(const V& v, int s) {   // node s of v
    const int m0 = v.mut_offset[s], m1 = v.mut_offset[s + 1], i0 = v.miss_offset[s], i1 = v.miss_offset[s + 1], f0 = v.mfs_offset[s], f1 = v.mfs_offset[s + 1];
    muts.resize(m1 - m0); for (int k = m0; k < m1; ++k) muts[k - m0] = HMut{v.mut_t[k], v.mut_site[k], v.mut_from[k], v.mut_to[k]};
    miss.resize(i1 - i0); for (int k = i0; k < i1; ++k) miss[k - i0] = HIv{v.miss_start[k], v.miss_end[k]};
    mfs.resize(f1 - f0); for (int k = f0; k < f1; ++k) mfs[k - f0] = HFs{v.mfs_site[k], v.mfs_state[k]};
  }
  struct ListCursor { size_t m = 0, i = 0, f = 0; void count(const HNode& n) { m += n.muts.size(); i += n.miss.size(); f += n.mfs.size(); } };
  void put_lists(FlatTree& f, int s, ListCursor& k) const {   // as node s of f, whose list arrays have their final size, at the cursor; closes the node's CSR ranges
    for (const auto& m : muts) { f.mut_site[k.m] = m.site; f.mut_from[k.m] = m.from; f.mut_to[k.m] = m.to; f.mut_t[k.m] = m.t; ++k.m; }
    for (const auto& iv : miss) { f.miss_start[k.i] = iv.start; f.miss_end[k.i] = iv.end; ++k.i; }
    for (const auto& fs : mfs) { f.mfs_site[k.f] = fs.site; f.mfs_state[k.f] = fs.state; ++k.f; }
    f.mut_offset[s + 1] = (int32_t)k.m; f.miss_offset[s + 1] = (int32_t)k.i; f.mfs_offset[s + 1] = (int32_t)k.f;
  }
};
struct HTree {
  int32_t root = EMAT_NO_NODE;
  std::vector<HNode> nodes;
  static HTree from_view(const emat_flat_tree& v) {
    HTree t; t.root = v.root; t.nodes.resize(v.num_nodes);
    for (int i = 0; i < v.num_nodes; ++i) {
      HNode& n = t.nodes[i];
      n.parent = v.parent[i]; n.c0 = v.child0[i]; n.c1 = v.child1[i]; n.t_min = v.t_min[i]; n.t_max = v.t_max[i]; n.t = v.t[i];
      n.take_lists(v, i);
    }
    return t;
  }
  FlatTree to_flat() const {
    FlatTree f; const int n = (int)nodes.size();
    HNode::ListCursor total; for (const HNode& nd : nodes) total.count(nd);
    f.allocate(n, (int32_t)total.m, (int32_t)total.i, (int32_t)total.f); f.root = root;
    HNode::ListCursor k;
    for (int i = 0; i < n; ++i) {
      const HNode& nd = nodes[i];
      f.parent[i] = nd.parent; f.child0[i] = nd.c0; f.child1[i] = nd.c1; f.t[i] = nd.t; f.t_min[i] = nd.t_min; f.t_max[i] = nd.t_max;
      nd.put_lists(f, i, k);
    }
    return f;
  }
  double t_max_tip() const { double t = -INFINITY; for (auto& n : nodes) if (n.is_tip() && n.t_max > t) t = n.t_max; return t; }   // phylo_tree_calc.cpp:636-644
};

inline bool iv_contains(const std::vector<HIv>& v, int l) {
  auto it = std::upper_bound(v.begin(), v.end(), l, [](int x, const HIv& iv) { return x < iv.start; });
  if (it == v.begin()) return false;
  --it; return l < it->end;
}
inline std::vector<HIv> iv_merge(const std::vector<HIv>& A, const std::vector<HIv>& B) {   // interval_set.h:238-288
  std::vector<HIv> out; size_t ia = 0, ib = 0; bool inside = false; int cs = 0, ce = 0;
  while (!(ia == A.size() && ib == B.size())) {
    bool useA = (ia == A.size()) ? false : (ib == B.size()) ? true : (A[ia].start <= B[ib].start);
    HIv f = useA ? A[ia] : B[ib];
    if (!inside) { cs = f.start; ce = f.end; (useA ? ia : ib)++; inside = true; }
    else if (f.start <= ce) { ce = std::max(ce, f.end); (useA ? ia : ib)++; }
    else { out.push_back({cs, ce}); inside = false; }
  }
  if (inside) out.push_back({cs, ce});
  return out;
}

inline void sync_topology(Topology& tp, const HTree& tree) {   // the topology of a host-resident tree
  const int N = (int)tree.nodes.size();
  tp.parent.resize(N); tp.kids_own.resize(N); tp.root = tree.root; tp.root_t = tree.nodes[tree.root].t;
  parallel_for(N, [&](int v) { const HNode& nd = tree.nodes[v]; tp.parent[v] = nd.parent; tp.kids_own[v] = Kids{nd.c0, nd.c1}; }, 4096);
  tp.kids = tp.kids_own.data(); tp.n = N;
}

// Run::normalize_root + rereference_to_root_sequence (run.cpp:258-265, phylo_tree.cpp:309-322)
inline bool normalize_root(HTree& tree, std::vector<uint8_t>& ref) {   // true: the reference sequence changed
  HNode& r = tree.nodes[tree.root];
  if (r.muts.empty()) return false;
  for (auto& m : r.muts) ref[m.site] = m.to;
  for (auto& nd : tree.nodes) {
    if (nd.miss.empty()) continue;
    for (auto& m : r.muts) {
      if (!iv_contains(nd.miss, m.site)) continue;
      auto it = std::lower_bound(nd.mfs.begin(), nd.mfs.end(), m.site, [](const HFs& f, int l) { return f.site < l; });
      if (it != nd.mfs.end() && it->site == m.site) { if (it->state == m.to) nd.mfs.erase(it); }
      else if (m.from != m.to) nd.mfs.insert(it, HFs{m.site, m.from});
    }
  }
  r.muts.clear();
  return true;
}

// State at a cut point c: the sites missing at c (union of the missations from c up to the root) and the deltas
// reference sequence -> sequence at c (reconstruct_missing_sites_at phylo_tree_calc.cpp:41-56, view_of_sequence_at
// :19-35).  The reference recomputes both by walking from every subroot to the root; here they are carried down the
// tree of cut points instead -- state(c) = state(nearest cut point above c) extended by the path between the two --
// which gives the same sets at a cost proportional to the part depth rather than the tree depth.
struct HFsPair { int32_t site; uint8_t from, to; };
struct CutState { std::vector<HIv> miss; std::vector<HFsPair> deltas; };
inline void cut_point_states(const HTree& tree, const std::vector<PartMap>& parts, const Topology& tp, std::vector<CutState>& out) {
  const int P = (int)parts.size();
  out.assign(P, CutState{});
  std::vector<int32_t> part_of_node(tree.nodes.size(), -1);
  for (int p = 0; p < P; ++p) part_of_node[parts[p].cut_point] = p;
  std::vector<int> above(P, -1);   // part whose cut point is the nearest one above this part's cut point
  std::vector<std::vector<int32_t>> path(P);   // nodes strictly below `above`'s cut point down to this cut point, top-down
  parallel_for(P, [&](int p) {
    std::vector<int32_t> up;
    int32_t cur = parts[p].cut_point;
    up.push_back(cur);
    for (cur = tp.parent[cur]; cur != EMAT_NO_NODE; cur = tp.parent[cur]) {
      if (part_of_node[cur] >= 0) { above[p] = part_of_node[cur]; break; }
      up.push_back(cur);
    }
    path[p].assign(up.rbegin(), up.rend());
  });
  // levels of the forest of cut points: a part's state needs only the state of the part above it, so the parts of
  // one level are independent
  std::vector<std::vector<int>> levels;
  {
    std::vector<std::vector<int>> below(P); std::vector<int> frontier;
    for (int p = 0; p < P; ++p) if (above[p] >= 0) below[above[p]].push_back(p); else frontier.push_back(p);
    while (!frontier.empty()) {
      std::vector<int> next;
      for (int p : frontier) for (int q : below[p]) next.push_back(q);
      levels.push_back(std::move(frontier));
      frontier = std::move(next);
    }
  }
  for (const auto& level : levels) parallel_for((int)level.size(), [&](int li) {
    const int p = level[li];
    CutState& st = out[p];
    std::map<int32_t, std::pair<uint8_t, uint8_t>> deltas;
    if (above[p] >= 0) {
      const CutState& a = out[above[p]];
      st.miss = a.miss;
      for (const auto& d : a.deltas) deltas.emplace_hint(deltas.end(), d.site, std::make_pair(d.from, d.to));
    }
    for (int32_t node : path[p]) {
      const HNode& nd = tree.nodes[node];
      if (!nd.miss.empty()) st.miss = iv_merge(st.miss, nd.miss);
      for (const auto& m : nd.muts) {   // forward in time: push_back_site_deltas
        auto f = deltas.find(m.site);
        if (f == deltas.end()) deltas[m.site] = {m.from, m.to};
        else { if (f->second.second != m.from) throw std::runtime_error("inconsistent mutation chain above a subroot"); f->second.second = m.to; if (f->second.first == f->second.second) deltas.erase(f); }
      }
    }
    st.deltas.reserve(deltas.size());
    for (const auto& [l, d] : deltas) st.deltas.push_back(HFsPair{l, d.first, d.second});
  }, 8);
}

// The subtree of every part (run.cpp:131-184), flat from the start; `states` from cut_point_states.
inline void build_subtrees(const HTree& tree, const std::vector<uint8_t>& ref, const std::vector<PartMap>& parts, const PartKids& part_kids, const std::vector<CutState>& states,
                           std::vector<FlatTree>& subtrees) {
  const int P = (int)parts.size();
  subtrees.clear(); subtrees.resize(P);
  parallel_for(P, [&](int p) {
    const PartMap& pm = parts[p];
    const int n = (int)pm.orig.size();
    const int32_t subroot = pm.cut_point;
    // the subroot's synthetic lists (run.cpp:141-153): missing sites at the cut, deltas reference -> sequence at the cut
    HNode synth; synth.miss = states[p].miss;
    for (const auto& d : states[p].deltas) if (!iv_contains(synth.miss, d.site)) synth.muts.push_back(HMut{-std::numeric_limits<double>::max(), d.site, ref[d.site], d.to});
    HNode::ListCursor total;
    for (int s = 0; s < n; ++s) total.count(pm.orig[s] == subroot ? synth : tree.nodes[pm.orig[s]]);
    FlatTree st; st.allocate(n, (int32_t)total.m, (int32_t)total.i, (int32_t)total.f); st.root = 0;
    HNode::ListCursor k;
    for (int s = 0; s < n; ++s) {
      const int32_t o = pm.orig[s];
      const HNode& on = tree.nodes[o];
      const int32_t k0 = part_kids[p][s].first, k1 = part_kids[p][s].second;
      st.child0[s] = k0; st.child1[s] = k1;
      if (k0 != EMAT_NO_NODE) { st.parent[k0] = s; st.parent[k1] = s; }
      st.t[s] = on.t;
      if (k0 == EMAT_NO_NODE && !on.is_tip()) { st.t_min[s] = (float)on.t; st.t_max[s] = (float)on.t; }   // frozen boundary node (run.cpp:165-168)
      else { st.t_min[s] = on.t_min; st.t_max[s] = on.t_max; }
      // A frozen boundary "tip" whose float-rounded bounds do not bracket t would fail the t_min <= t <= t_max
      // convention by an ulp of float; the reference tolerates 1e-2 (phylo_tree.cpp:117-121).  Keep t exact.
      (o == subroot ? synth : on).put_lists(st, s, k);
    }
    st.parent[0] = EMAT_NO_NODE;
    subtrees[p] = std::move(st);
  });
}

// The parts back into the tree (run.cpp:195-256).  Every node of the whole tree is a non-root node of exactly one part (the run's root: the
// root of the root part), and that part alone writes its time, lists and child links; a cut node's parent link is written by the part
// above it, as the parent of one of its children.  The parts therefore gather independently.
inline void gather_parts(HTree& tree, const std::vector<PartMap>& parts, const std::vector<FlatTree>& subtrees, int root_part) {
  parallel_for((int)subtrees.size(), [&](int p) {
    const PartMap& pm = parts[p]; const FlatTree& st = subtrees[p];
    for (int s = 0; s < st.num_nodes(); ++s) {
      const int32_t o = pm.orig[s]; HNode& on = tree.nodes[o];
      const bool owns = s != st.root || p == root_part;
      if (owns) { on.t = st.t[s]; on.take_lists(st, s); }
      if (!st.is_tip(s)) {
        int32_t l = pm.orig[st.child0[s]], r = pm.orig[st.child1[s]];
        on.c0 = l; on.c1 = r; tree.nodes[l].parent = o; tree.nodes[r].parent = o;
      }
    }
    if (p == root_part) { const int32_t nr = pm.orig[st.root]; tree.root = nr; tree.nodes[nr].parent = EMAT_NO_NODE; }
  });
}

}  // namespace emat
#endif  // EMAT_RUN_TREE_HPP_
