// emat_run_partition.hpp -- the run driver's partitioner: the compact topology its walks read, the reference's random stencils
// (core/tree_partitioning.h:139-194), the part-size refinement (not in the reference), partition_tree (:88-135, :196-239), and the
// object that owns what a cycle's draw needs and produces.  Nothing here knows the node records (emat_run_tree.hpp), a backend or a driver.
//
// Included by emat_run.cpp, first of its three headers (emat_run_partition.hpp, emat_run_tree.hpp, emat_run_exchange.hpp: each may use the
// ones before it; none needs a forward declaration of a later one).
#ifndef EMAT_RUN_PARTITION_HPP_
#define EMAT_RUN_PARTITION_HPP_

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <memory>
#include <utility>
#include <vector>

#include "../../include/emat_backend.h"
#include "host_parallel.hpp"
#include "synth.hpp"

namespace emat {

// Compact copy of the whole tree's topology (the node records carry three vectors each and are 100+ bytes apart:
// walking them misses the cache at every step).  Rebuilt at the start of every repartition.
// The partitioner's walks read a node's two children and nothing else: side by side, one cache line per visit (they are bound
// by misses on a 200 000-node tree).  `kids` points at this object's own copy (host-resident tree: sync_topology, emat_run_tree.hpp) or
// straight into the backend's page-locked mirror of the device-resident tree, which every reassemble refreshes.
struct Kids { int32_t c0, c1; };
struct Topology {
  std::vector<int32_t> parent; std::vector<Kids> kids_own; const Kids* kids = nullptr;
  int n = 0; int32_t root = EMAT_NO_NODE; double root_t = 0.0;
};

// A part of the partition: subtree <-> whole-tree node maps (tree_partitioning.h:31-54).
struct PartMap {
  int32_t cut_point = EMAT_NO_NODE;
  std::vector<int32_t> orig;      // subtree node -> whole-tree node
};
using PartKids = std::vector<std::vector<std::pair<int32_t, int32_t>>>;   // per part, per subtree node: its two children as subtree nodes

// tree_partitioning.h:139-194
inline std::vector<int32_t> generate_random_partition_stencil(const Topology& tp, int num_parts, SplitMix64& bitgen) {
  std::vector<int32_t> cuts;
  const int N = tp.n;
  std::vector<int> descendants(N, 0);
  long num_branches_left = N; int num_parts_left = num_parts;
  struct Item { int32_t node; int csf; };
  std::vector<Item> stack; stack.push_back({tp.root, -1});
  bool done = false;
  while (!stack.empty() && !done) {
    Item it = stack.back(); stack.pop_back();
    const int32_t nd_c0 = tp.kids[it.node].c0, nd_c1 = tp.kids[it.node].c1;
    const int nch = nd_c0 == EMAT_NO_NODE ? 0 : 2;
    if (it.csf == -1) {
      stack.push_back({it.node, nch});
      if (nch == 2) {
        if (bitgen.next() >> 63) { stack.push_back({nd_c0, -1}); stack.push_back({it.node, 1}); stack.push_back({nd_c1, -1}); stack.push_back({it.node, 0}); }
        else { stack.push_back({nd_c1, -1}); stack.push_back({it.node, 1}); stack.push_back({nd_c0, -1}); stack.push_back({it.node, 0}); }
      }
      continue;
    }
    if (it.csf != nch) continue;   // only post-order visits matter
    const int node = it.node;
    if (node == tp.root) break;
    if ((int)cuts.size() == num_parts - 1) break;
    descendants[node] = 1;
    if (nch == 2) descendants[node] += descendants[nd_c0] + descendants[nd_c1];
    long min_subtree_size = std::max(10L, num_branches_left / (num_parts_left + 1));
    if (descendants[node] >= min_subtree_size) {
      bool allowed = true;
      if (allowed && (num_branches_left - (descendants[node] - 1)) < min_subtree_size) allowed = false;
      if (allowed && (bitgen.next() >> 63)) allowed = false;
      if (allowed) {
        num_branches_left -= descendants[node] - 1;
        cuts.push_back(node);
        descendants[node] = 1;
        --num_parts_left;
      }
    }
  }
  return cuts;
}

// NOT in the reference: cut oversized parts further.  The reference sizes its parts for a handful of CPU threads; its stencils are
// lists of cut NODES drawn every 200 cycles, and as the moves re-hang subtrees the parts those nodes delimit drift apart in
// size -- by a few per cent at 8 parts of 25 000 nodes, but at 8 000 parts of 25 nodes a stencil that started balanced holds parts
// of 700-2 000 nodes after a few cycles.  Every part performs the same number of moves per pass and the GPU runs all parts at
// once, so the pass lasts as long as the chain of the largest part.  Parts above `limit` nodes therefore get further cut nodes,
// drawn UNIFORMLY AT RANDOM among their inner nodes, round after round until no piece exceeds the limit.
// Why that does not bias the sampler (the reference's own concern, run.cpp:88-93): a pass only moves nodes WITHIN a part of the
// refined partition R, so which nodes a part owns, and which of them are inner nodes, is the same before and after the pass --
// for the parts of R and for every coarser level they were cut from.  The rule reads nothing else (no subtree sizes, no times),
// so the probability of drawing R from the tree before the pass and from the tree after it is the same: the pass is a mixture of
// within-part kernels whose weights are constant on every set of trees it connects, which keeps each kernel's detailed balance.
// (Cutting at the node that halves a part best -- what this function did until round 4 -- reads subtree sizes, which a pass
// changes: a state-dependent choice of the kind the reference avoids by redrawing its stencils slowly.)
// The draws come from a stream of their own (seed, epoch): the reference-rule stream `bitgen` sees the same sequence with the
// limit on or off.
// max_part_nodes: 0 = the reference's partition rule exactly; > 0 = parts larger than this are cut further; -1 = three times the mean part size
inline int effective_max_part_nodes(int max_part_nodes, int num_parts, size_t num_nodes) {
  if (max_part_nodes >= 0) return max_part_nodes;
  const long mean = (long)num_nodes / std::max(1, num_parts);
  return (int)std::max(64L, 3 * mean);
}
struct RefinedCuts { std::vector<int32_t> cuts; int extra = 0; };   // the stencil's cut nodes followed by the `extra` ones the limit added
inline RefinedCuts refine_stencil(const Topology& tp, std::vector<int32_t> cuts, uint64_t seed, uint64_t epoch, int eff) {   // eff: effective_max_part_nodes
  const int N = tp.n;
  int extra_cuts = 0;
  if (eff <= 0) return {std::move(cuts), 0};
  const int limit = std::max(eff, 21);
  // cut marks as a bit set (25 KB at 200 000 nodes: resident in every core's cache, where a byte per node costs a second miss per
  // visited node); tasks set bits of their own parts only, but share words: atomic OR, relaxed loads
  std::vector<std::atomic<uint32_t>> cut_bits(((size_t)N + 31) / 32);
  for (auto& w : cut_bits) w.store(0, std::memory_order_relaxed);
  auto mark_cut = [&](int32_t v) { cut_bits[(size_t)v >> 5].fetch_or(1u << (v & 31), std::memory_order_relaxed); };
  auto is_cut = [&](int32_t v) { return (cut_bits[(size_t)v >> 5].load(std::memory_order_relaxed) >> (v & 31)) & 1u; };
  for (int32_t c : cuts) mark_cut(c);
  mark_cut(tp.root);
  std::vector<int32_t> roots(cuts);
  if (std::find(roots.begin(), roots.end(), tp.root) == roots.end()) roots.push_back(tp.root);
  // Every part of the stencil on its own (host threads): walk it from its cut node, and if it is oversized cut it, then its
  // oversized pieces, and so on.  A walk stops at cut nodes, so a task only ever writes is_cut of nodes its own part owns.
  std::vector<std::vector<int32_t>> extra(roots.size());
  const uint64_t round_seed = seed ^ (0x9E3779B97F4A7C15ull * (epoch + 1)) ^ 0x5A17C0DEull;
  const Kids* const kids = tp.kids;
  parallel_for((int)roots.size(), [&](int ri) {
    static thread_local std::vector<int32_t> work, inner, stack;   // (8 000 tasks per cycle: no allocation in any of them)
    static thread_local std::vector<std::pair<uint64_t, int32_t>> keyed;
    work.clear(); work.push_back(roots[(size_t)ri]);
    SplitMix64 rng(round_seed ^ (0xD6E8FEB86659FD93ull * (uint64_t)(roots[(size_t)ri] + 1)));   // a stream per part: the result does not depend on the threads
    bool first = true;
    while (!work.empty()) {
      const int32_t c = work.back(); work.pop_back();
      // the piece below c: its size (a cut child counts as one node: it is a tip here) and its inner nodes other than c
      int size = 0; inner.clear(); stack.clear(); stack.push_back(c);
      while (!stack.empty()) {
        const int32_t v = stack.back(); stack.pop_back(); ++size;
        const Kids k = kids[v];   // (both children in one cache line: the walk is bound by misses on a 200 000-node tree)
        if (k.c0 == EMAT_NO_NODE || (v != c && is_cut(v))) continue;
        if (v != c) inner.push_back(v);
        stack.push_back(k.c0); stack.push_back(k.c1);
        __builtin_prefetch(&kids[k.c0]); __builtin_prefetch(&kids[k.c1]);   // (c1 is visited next, c0 after c1's whole subtree: its line is on its way by then)
      }
      if (first && size <= limit) return;   // the common case: one walk, nothing to do
      first = false;
      if (size <= limit || inner.empty()) continue;
      // as many new cut nodes as would make the pieces `limit` nodes on average, a uniformly drawn subset of the inner nodes.
      // The subset must not depend on the ORDER in which the walk met the nodes -- that order is the piece's topology, which the pass changes, while
      // the set is not -- so that the draw is a function of (what a pass leaves alone, the stream) alone and repeating it on the tree after the pass
      // gives the very same cut nodes (round 6: emat_run_debug_redraw_partition, tests/test_host_driver.py; until then the invariance held in
      // distribution only).  Every inner node gets a pseudo-random 64-bit key from (a salt drawn from the part's stream, its own index) and the `want`
      // smallest keys are taken: a uniform subset whatever the order of `inner`, found by selection in O(n) -- sorting the nodes and shuffling, the
      // first version of this, cost the refinement 0.45 ms per cycle at C4.
      const int want = std::min((int)inner.size(), std::max(1, (size + limit - 1) / limit - 1));
      const uint64_t salt = rng.next();
      keyed.clear();
      for (int32_t v : inner) { uint64_t z = salt ^ ((uint64_t)(uint32_t)v * 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; keyed.push_back({z ^ (z >> 31), v}); }
      std::nth_element(keyed.begin(), keyed.begin() + (want - 1), keyed.end());
      std::sort(keyed.begin(), keyed.begin() + want);   // (the few that were drawn, by key: the order in which their pieces are looked at next)
      for (int k = 0; k < want; ++k) { const int32_t v = keyed[(size_t)k].second; mark_cut(v); extra[(size_t)ri].push_back(v); work.push_back(v); }
      work.push_back(c);   // what is left above the new cut nodes may still be too large
    }
  }, 16, 32);
  for (auto& e : extra) { cuts.insert(cuts.end(), e.begin(), e.end()); extra_cuts += (int)e.size(); }
  return {std::move(cuts), extra_cuts};
}

// tree_partitioning.h:88-135 and :196-239
inline int partition_tree(const Topology& tp, const std::vector<int32_t>& stencil, std::vector<PartMap>& parts, PartKids& part_kids) {   // returns the root part
  int root_idx = (int)stencil.size(); bool root_in = false;
  for (size_t i = 0; i < stencil.size(); ++i) if (stencil[i] == tp.root) { root_in = true; root_idx = (int)i; break; }
  const int P = (int)stencil.size() + (root_in ? 0 : 1);
  std::vector<char> is_cut((size_t)tp.n, 0);
  for (int32_t c : stencil) is_cut[c] = 1;
  if (!root_in) { is_cut[tp.root] = 1; root_idx = P - 1; }
  const int root_part = root_idx;
  parts.assign(P, PartMap{});
  part_kids.assign(P, {});
  parallel_for(P, [&](int i) {   // every part walks down from its own cut point: independent
    PartMap& pm = parts[i];
    pm.cut_point = (i == root_part) ? tp.root : stencil[i];
    struct W { int32_t src, dst; };
    std::vector<W> work; pm.orig.clear(); pm.orig.push_back(pm.cut_point);
    work.push_back({pm.cut_point, 0});
    // children get consecutive indices when their parent is expanded; right child expanded first (LIFO)
    std::vector<std::pair<int32_t, int32_t>> kids(1, {EMAT_NO_NODE, EMAT_NO_NODE});
    while (!work.empty()) {
      W w = work.back(); work.pop_back();
      const int32_t k0 = tp.kids[w.src].c0, k1 = tp.kids[w.src].c1;
      if (k0 == EMAT_NO_NODE || (is_cut[w.src] && w.src != pm.cut_point)) continue;
      int32_t dl = (int32_t)pm.orig.size(); pm.orig.push_back(k0);
      int32_t dr = (int32_t)pm.orig.size(); pm.orig.push_back(k1);
      kids.resize(pm.orig.size(), {EMAT_NO_NODE, EMAT_NO_NODE});
      kids[w.dst] = {dl, dr};
      work.push_back({k0, dl}); work.push_back({k1, dr});
    }
    part_kids[i] = std::move(kids);
  });
  return root_part;
}

// ---- the draw of a cycle's partition: refresh_partition_stencils (run.cpp:87-108), the pick, and the part-size limit's refinement.
// Apart from the cut itself so that the run drivers of ONE process (emat_multi: a driver per GPU, all with the same seed, all bound to
// draw the very same thing) draw once: the leader draws (emat_run_draw_partition, or implicitly at its repartition), a follower
// (emat_run_follow_draws) takes the leader's cut nodes -- 8 000-14 000 integers behind a shared pointer -- instead of walking the tree
// again on the same host cores (eight shards refined the same stencil eight times).
// A follower holds a pointer to its leader's PartitionDraw and to nothing else of the leader.
struct PartitionDraw {
  SplitMix64 bitgen{0};                                  // the reference-rule stream: the same sequence with the limit on or off
  std::vector<std::vector<int32_t>> stencils; int64_t stencil_refresh_countdown = 0;
  std::shared_ptr<const std::vector<int32_t>> drawn; uint64_t drawn_for_epoch = ~0ull;   // the cut nodes of the partition of that epoch
  int last_pick = -1; uint64_t last_refine_epoch = 0;   // which stencil the last draw picked, and the epoch its refinement's random stream was keyed with (emat_run_debug_redraw_partition)
  int last_extra_cuts = 0;                               // cut nodes its refinement added (emat_run_partition_stats)
  bool has(uint64_t epoch) const { return drawn && drawn_for_epoch == epoch; }
  void draw(const Topology& tp, int num_parts, uint64_t seed, uint64_t epoch, int eff_max_part_nodes) {   // refresh_partition_stencils (run.cpp:87-108), the pick, the refinement
    if (stencils.empty() || stencil_refresh_countdown <= 0) {
      stencils.clear();
      for (int i = 0; i < 10; ++i) stencils.push_back(generate_random_partition_stencil(tp, num_parts, bitgen));
      stencil_refresh_countdown = 200;
    }
    --stencil_refresh_countdown;
    last_pick = bitgen.below((int)stencils.size()); last_refine_epoch = epoch;
    RefinedCuts r = refine_stencil(tp, stencils[(size_t)last_pick], seed, epoch, eff_max_part_nodes);
    last_extra_cuts = r.extra;
    drawn = std::make_shared<const std::vector<int32_t>>(std::move(r.cuts));
    drawn_for_epoch = epoch;
  }
  void take(const PartitionDraw& leader) {   // a follower: the leader's draw of the same epoch (the cut nodes stay behind the shared pointer)
    drawn = leader.drawn; drawn_for_epoch = leader.drawn_for_epoch;
    last_pick = leader.last_pick; last_refine_epoch = leader.last_refine_epoch; last_extra_cuts = leader.last_extra_cuts;
  }
};

}  // namespace emat
#endif  // EMAT_RUN_PARTITION_HPP_
