// emat_mcc_host.hpp -- host side of the store of sampled trees and of the MCC derivation (emat_mcc_kernels.hpp): argument and
// state checks, sizes, the launches, and the two things that stay on the host because they are a few thousand flops: turning
// the per-sample histograms into log clade credibilities and picking the master (mcc_tree.cpp:78-108).
//
// Included by emat_backend.hip after its entry points, after emat_gtree_host.hpp (gt_require).
#ifndef EMAT_MCC_HOST_HPP_
#define EMAT_MCC_HOST_HPP_

namespace {

constexpr size_t k_mcc_store_bytes_per_node = 20;    // parent, child0, child1 (int32), t (double)
constexpr size_t k_mcc_derive_bytes_per_node = 21;   // fingerprint (8), tip count (4), arrival word (4), corresponding node (4), exact flag (1)

std::string mcc_mb(size_t bytes) { return std::to_string((bytes + (1u << 20) - 1) >> 20) + " MB"; }

// EMAT_ERR_CAPACITY, with the sizes, when the device does not have `bytes` free (an allocation that fails later would be EMAT_ERR_HIP).
emat_status mcc_check_room(emat_backend* h, const std::string& w, size_t bytes, const std::string& what_for) {
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (bytes > free_b) return fail(h, EMAT_ERR_CAPACITY, w + ": " + what_for + " needs " + mcc_mb(bytes) + ", the device has " + mcc_mb(free_b) + " free of " + mcc_mb(total_b));
  return EMAT_OK;
}

// (Re)binds the store to `capacity` samples of `n` nodes.  Frees what it held first, so that the room it asks for is the room it needs.
emat_status mcc_store_alloc(emat_backend* h, const std::string& w, int64_t capacity, int32_t n) {
  MccHost& X = h->mcc;
  const size_t nodes = (size_t)capacity * (size_t)n;
  const size_t store_bytes = nodes * k_mcc_store_bytes_per_node + (size_t)capacity * 4, derive_bytes = nodes * k_mcc_derive_bytes_per_node + (size_t)n * 64;
  if (nodes > X.parent.n || (size_t)capacity > X.root.n) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    X.release(); h->probe.release_samples(); h->mcs.release();
    emat_status st = mcc_check_room(h, w, store_bytes + derive_bytes, std::to_string(capacity) + " samples of " + std::to_string(n) + " nodes (" + mcc_mb(store_bytes) + " for the store, " + mcc_mb(derive_bytes) + " for a derivation over all of them)");
    if (st) return st;
    HIP_TRY(X.parent.alloc(nodes)); HIP_TRY(X.c0.alloc(nodes)); HIP_TRY(X.c1.alloc(nodes)); HIP_TRY(X.t.alloc(nodes)); HIP_TRY(X.root.alloc((size_t)capacity));
  }
  if (X.mut_capacity > 0 && (X.mut_slots != (int32_t)capacity || X.mut_n != n)) { HIP_TRY(hipStreamSynchronize(h->stream)); X.release_mutations(); }   // (made for other slots: emat_tree_samples_reserve_mutations again)
  X.capacity = (int32_t)capacity; X.n = n; X.count = 0; X.derived_M = 0; X.is_tip.clear(); X.mut_used = 0;
  return EMAT_OK;
}

// What a push on a store with mutation room checks before it writes anything: the store's number of sites, and `records` free in the arena.
emat_status mcc_mut_room_for(emat_backend* h, const std::string& w, int64_t records) {
  const MccHost& X = h->mcc;
  if (X.mut_L != h->L)
    return fail(h, EMAT_ERR_STATE, w + ": the store keeps mutations of " + std::to_string(X.mut_L) + " sites and the handle has " + std::to_string(h->L) + ": emat_tree_samples_clear and emat_tree_samples_reserve_mutations first (site counts are never mixed)");
  if (records > X.mut_capacity - X.mut_used)
    return fail(h, EMAT_ERR_CAPACITY, w + ": this sample has " + std::to_string(records) + " mutation records and the arena has " + std::to_string(X.mut_capacity - X.mut_used) + " free of " + std::to_string(X.mut_capacity) +
                                      ": nothing is pushed; emat_tree_samples_clear, or emat_tree_samples_reserve_mutations with more");
  return EMAT_OK;
}
// Hands slot `slot` its segment of `records` records (-1: the sample comes without mutations); returns where it starts.
int64_t mcc_mut_take(MccHost& X, int32_t slot, int64_t records) {
  if (X.mut_base.size() < (size_t)X.capacity) { X.mut_base.resize((size_t)X.capacity, -1); X.mut_len.resize((size_t)X.capacity, 0); }
  if (records < 0) { X.mut_base[(size_t)slot] = -1; X.mut_len[(size_t)slot] = 0; return -1; }
  const int64_t base = X.mut_used;
  X.mut_base[(size_t)slot] = base; X.mut_len[(size_t)slot] = (uint32_t)records; X.mut_used += records;
  return base;
}

// What every call on the store starts with; `need_tree`: the resident tree is read (and so must not be out on its slabs).
emat_status mcc_require(emat_backend* h, const std::string& w, bool need_tree) {
  return need_tree ? gt_require_tree_home(h, false, w + ": ") : gt_require(h, false);
}
emat_status mcc_require_store(emat_backend* h, const std::string& w) {
  const MccHost& X = h->mcc;
  if (X.capacity == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_tree_samples_reserve first");
  if (h->gt.resident && h->gt.n != X.n)
    return fail(h, EMAT_ERR_STATE, w + ": the store holds samples of " + std::to_string(X.n) + " nodes and the resident tree has " + std::to_string(h->gt.n) + ": emat_tree_samples_clear first (node counts are never mixed)");
  return EMAT_OK;
}

MccStore mcc_store_dev(MccHost& X) { MccStore S{}; S.parent = X.parent.p; S.c0 = X.c0.p; S.c1 = X.c1.p; S.t = X.t.p; S.root = X.root.p; S.n = X.n; return S; }

// The checks of emat_tree_sample_push_flat; empty when the arrays are a binary tree of n nodes with one root.
std::string mcc_validate_flat(int32_t n, const int32_t* parent, const int32_t* c0, const int32_t* c1, int32_t root, const std::vector<uint8_t>& is_tip) {
  auto node = [&](int32_t v) { return v >= 0 && v < n; };
  if (!node(root)) return "root " + std::to_string(root) + " is outside the valid range [0, " + std::to_string(n) + ")";
  int32_t roots = 0;
  for (int32_t v = 0; v < n; ++v) {
    const std::string sv = "node " + std::to_string(v);
    if (parent[v] == EMAT_NO_NODE) { ++roots; if (v != root) return sv + " has no parent and is not the root (" + std::to_string(root) + "): a tree has one root"; }
    else if (!node(parent[v])) return sv + ": parent " + std::to_string(parent[v]) + " is outside the valid range";
    else if (c0[parent[v]] != v && c1[parent[v]] != v) return sv + " is not a child of its parent " + std::to_string(parent[v]);
    const bool tip = c0[v] == EMAT_NO_NODE && c1[v] == EMAT_NO_NODE;
    if (!tip) {
      if (!node(c0[v]) || !node(c1[v]) || c0[v] == c1[v]) return sv + " is not binary: children " + std::to_string(c0[v]) + ", " + std::to_string(c1[v]);
      if (parent[c0[v]] != v || parent[c1[v]] != v) return sv + ": a child does not name it as its parent";
    }
    if (!is_tip.empty() && (is_tip[(size_t)v] != 0) != tip) return sv + (tip ? " is a tip here and an inner node" : " is an inner node here and a tip") + " in sample 0: tips keep their indices across samples (mcc_tree.cpp:118-124)";
  }
  if (parent[root] != EMAT_NO_NODE || roots != 1) return "the root must be the one node without a parent";
  // links are consistent and every node but the root has a parent: what is left to exclude is a cycle beside the tree
  std::vector<int32_t> stack{root}; int32_t seen = 0;
  while (!stack.empty()) { const int32_t v = stack.back(); stack.pop_back(); ++seen; if (c0[v] != EMAT_NO_NODE) { stack.push_back(c0[v]); stack.push_back(c1[v]); } if (seen > n) break; }
  if (seen != n) return std::to_string(n - seen) + " nodes are not below the root (a cycle)";
  return "";
}

emat_status mcc_status_check(emat_backend* h, const std::string& w, int32_t s) {
  if (s & k_mcc_bad_link) return fail(h, EMAT_ERR_INTERNAL, w + ": a link of a stored sample leaves the tree");
  if (s & k_mcc_key_missing) return fail(h, EMAT_ERR_INTERNAL, w + ": a clade is missing from the table of clade counts");
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* (header: emat_tree_samples_reserve) */
emat_status emat_tree_samples_reserve(emat_backend* h, int32_t capacity) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_samples_reserve";
  emat_status st = gt_require(h, true, true); if (st) return st;
  if (capacity < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": capacity must be positive, not " + std::to_string(capacity));
  if (h->mcc.count > 0) return fail(h, EMAT_ERR_STATE, w + ": the store holds " + std::to_string(h->mcc.count) + " samples: emat_tree_samples_clear first (nothing is dropped silently)");
  return mcc_store_alloc(h, w, capacity, h->gt.n);
}

/* Base_tree_vector::push_back of a copy of the run's tree, delphy_ui.cpp:770-773 (header: emat_tree_sample_push) */
emat_status emat_tree_sample_push(emat_backend* h, int32_t* index) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_sample_push";
  emat_status st = mcc_require(h, w, true); if (st) return st;
  st = mcc_require_store(h, w); if (st) return st;
  MccHost& X = h->mcc;
  if (X.count >= X.capacity) return fail(h, EMAT_ERR_CAPACITY, w + ": the store is full (" + std::to_string(X.capacity) + " samples): nothing is evicted; emat_tree_samples_clear, or reserve more");
  if (X.is_tip.empty()) {   // sample 0 says which nodes are tips (the mirror of the children is current after every upload and reassemble)
    const int32_t* k = h->gt.kids();
    X.is_tip.resize((size_t)X.n);
    for (int32_t v = 0; v < X.n; ++v) X.is_tip[(size_t)v] = k[2 * v] == EMAT_NO_NODE;
  }
  if (X.mut_capacity > 0) {   // lists, the used part of the heap and the reference sequence go with it (gt_require has finished any gather: used[0] and the device's sequence are current)
    st = mcc_mut_room_for(h, w, (int64_t)h->gt.used[0]); if (st) return st;
    if (!h->have_ref) return fail(h, EMAT_ERR_STATE, w + ": emat_set_ref_sequence first (a sample that keeps its mutations keeps the sequence its root starts from)");
  }
  hipLaunchKernelGGL(k_mcc_push, dim3((unsigned)((X.n + 255) / 256)), dim3(256), 0, h->stream, h->gt.dev(), mcc_store_dev(X), X.count);
  HIP_TRY(hipGetLastError());
  if (X.mut_capacity > 0) {
    const size_t n = (size_t)X.n, L = (size_t)X.mut_L, used = (size_t)h->gt.used[0];
    const int64_t base = mcc_mut_take(X, X.count, (int64_t)used);
    HIP_TRY(hipMemcpyAsync(X.mut_hdr.p + (size_t)X.count * n, h->gt.muts.p, n * sizeof(GList), hipMemcpyDeviceToDevice, h->stream));
    if (used) HIP_TRY(hipMemcpyAsync(X.mut_arena.p + base, h->gt.mut_heap.p, used * sizeof(MutRec), hipMemcpyDeviceToDevice, h->stream));
    if (!h->model_dirty && h->d_ref.n >= L) HIP_TRY(hipMemcpyAsync(X.mut_ref.p + (size_t)X.count * L, h->d_ref.p, L, hipMemcpyDeviceToDevice, h->stream));
    else { HIP_TRY(hipStreamSynchronize(h->stream)); HIP_TRY(hipMemcpy(X.mut_ref.p + (size_t)X.count * L, h->ref.data(), L, hipMemcpyHostToDevice)); }   // (no launch has brought the model to the device yet: the host's copy is the current one)
  }
  if (index) *index = X.count;
  ++X.count;
  return EMAT_OK;
}

}  // extern "C"
namespace {
// emat_tree_sample_push_flat and emat_tree_sample_push_flat_mutations: the checks of the tree, all made before anything is written ...
emat_status mcc_push_flat_check(emat_backend* h, const std::string& w, int32_t num_nodes, const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* t, int32_t root) {
  emat_status st = mcc_require(h, w, false); if (st) return st;
  st = mcc_require_store(h, w); if (st) return st;
  MccHost& X = h->mcc;
  if (!parent || !child0 || !child1 || !t) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": parent, child0, child1 and t must be given");
  if (num_nodes != X.n) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": a tree of " + std::to_string(num_nodes) + " nodes, and the store holds samples of " + std::to_string(X.n));
  if (X.count >= X.capacity) return fail(h, EMAT_ERR_CAPACITY, w + ": the store is full (" + std::to_string(X.capacity) + " samples): nothing is evicted; emat_tree_samples_clear, or reserve more");
  const std::string msg = mcc_validate_flat(X.n, parent, child0, child1, root, X.is_tip);
  if (!msg.empty()) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": " + msg);
  return EMAT_OK;
}
// ... and the copies into the next slot (the count is the caller's to advance).
emat_status mcc_push_flat_copy(emat_backend* h, const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* t, int32_t root) {
  MccHost& X = h->mcc;
  if (X.is_tip.empty()) { X.is_tip.resize((size_t)X.n); for (int32_t v = 0; v < X.n; ++v) X.is_tip[(size_t)v] = child0[v] == EMAT_NO_NODE; }
  const size_t o = (size_t)X.count * (size_t)X.n, n = (size_t)X.n;
  HIP_TRY(hipStreamSynchronize(h->stream));   // (a derivation may still be reading the store)
  HIP_TRY(hipMemcpy(X.parent.p + o, parent, n * 4, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(X.c0.p + o, child0, n * 4, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(X.c1.p + o, child1, n * 4, hipMemcpyHostToDevice)); HIP_TRY(hipMemcpy(X.t.p + o, t, n * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(X.root.p + X.count, &root, 4, hipMemcpyHostToDevice));
  return EMAT_OK;
}
}  // namespace
extern "C" {

/* (header: emat_tree_sample_push_flat) */
emat_status emat_tree_sample_push_flat(emat_backend* h, int32_t num_nodes, const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* t, int32_t root, int32_t* index) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_sample_push_flat";
  emat_status st = mcc_push_flat_check(h, w, num_nodes, parent, child0, child1, t, root); if (st) return st;
  st = mcc_push_flat_copy(h, parent, child0, child1, t, root); if (st) return st;
  MccHost& X = h->mcc;
  if (X.mut_capacity > 0) mcc_mut_take(X, X.count, -1);   // (a tree without its mutations: the site-state prober refuses this sample)
  if (index) *index = X.count;
  ++X.count;
  return EMAT_OK;
}

/* a base tree read from a file with its mutations, as tools/delphy_mcc.cpp reads them (header: emat_tree_sample_push_flat_mutations) */
emat_status emat_tree_sample_push_flat_mutations(emat_backend* h, int32_t num_nodes, const int32_t* parent, const int32_t* child0, const int32_t* child1, const double* t, int32_t root,
                                                 const int32_t* mut_offset, const int32_t* mut_site, const uint8_t* mut_from, const uint8_t* mut_to, const double* mut_t, const uint8_t* ref_sequence, int32_t* index) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_sample_push_flat_mutations";
  emat_status st = mcc_push_flat_check(h, w, num_nodes, parent, child0, child1, t, root); if (st) return st;
  MccHost& X = h->mcc;
  if (X.mut_capacity == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_tree_samples_reserve_mutations first (this store keeps topology and times only)");
  if (!mut_offset || !ref_sequence) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mut_offset and ref_sequence must be given");
  const int32_t n = X.n, L = h->L;
  if (mut_offset[0] != 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mut_offset must start at 0, not " + std::to_string(mut_offset[0]));
  for (int32_t v = 0; v < n; ++v)
    if (mut_offset[v + 1] < mut_offset[v]) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mut_offset must not decrease: node " + std::to_string(v) + " has " + std::to_string(mut_offset[v]) + " and then " + std::to_string(mut_offset[v + 1]));
  const int32_t nm = mut_offset[n];
  if (nm > 0 && (!mut_site || !mut_from || !mut_to || !mut_t)) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mut_site, mut_from, mut_to and mut_t must be given");
  for (int32_t k = 0; k < nm; ++k) {
    if (mut_site[k] < 0 || mut_site[k] >= L) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mutation " + std::to_string(k) + ": site " + std::to_string(mut_site[k]) + " is outside the valid range [0, " + std::to_string(L) + ")");
    if (mut_from[k] > 3 || mut_to[k] > 3) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mutation " + std::to_string(k) + ": states must be 0..3, not " + std::to_string(mut_from[k]) + " -> " + std::to_string(mut_to[k]));
  }
  for (int32_t l = 0; l < L; ++l) if (ref_sequence[l] > 3) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": reference sequence states must be 0..3, and site " + std::to_string(l) + " has " + std::to_string(ref_sequence[l]));
  st = mcc_mut_room_for(h, w, nm); if (st) return st;
  std::vector<GList> hdr((size_t)n); std::vector<MutRec> rec((size_t)nm);
  for (int32_t v = 0; v < n; ++v) hdr[(size_t)v] = GList{(uint32_t)mut_offset[v], (uint32_t)(mut_offset[v + 1] - mut_offset[v])};
  for (int32_t k = 0; k < nm; ++k) { MutRec r{}; r.t = mut_t[k]; r.site = mut_site[k]; r.from = mut_from[k]; r.to = mut_to[k]; rec[(size_t)k] = r; }
  st = mcc_push_flat_copy(h, parent, child0, child1, t, root); if (st) return st;
  HIP_TRY(hipMemcpy(X.mut_hdr.p + (size_t)X.count * (size_t)n, hdr.data(), (size_t)n * sizeof(GList), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(X.mut_ref.p + (size_t)X.count * (size_t)L, ref_sequence, (size_t)L, hipMemcpyHostToDevice));
  if (nm) HIP_TRY(hipMemcpy(X.mut_arena.p + X.mut_used, rec.data(), (size_t)nm * sizeof(MutRec), hipMemcpyHostToDevice));
  mcc_mut_take(X, X.count, nm);
  if (index) *index = X.count;
  ++X.count;
  return EMAT_OK;
}

/* (header: emat_tree_samples_reserve_mutations) */
emat_status emat_tree_samples_reserve_mutations(emat_backend* h, int64_t mutation_records) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_samples_reserve_mutations";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  if (mutation_records < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": mutation_records must not be negative, not " + std::to_string(mutation_records));
  if (X.capacity == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_tree_samples_reserve first");
  if (X.count > 0) return fail(h, EMAT_ERR_STATE, w + ": the store holds " + std::to_string(X.count) + " samples: emat_tree_samples_clear first (nothing is dropped silently)");
  HIP_TRY(hipStreamSynchronize(h->stream));
  X.release_mutations();   // (freed first, so that the room asked for is the room needed)
  if (mutation_records == 0) return EMAT_OK;
  const size_t slots = (size_t)X.capacity, n = (size_t)X.n, L = (size_t)h->L, records = (size_t)mutation_records;
  if (mutation_records > ((int64_t)1 << 40)) return fail(h, EMAT_ERR_CAPACITY, w + ": " + std::to_string(mutation_records) + " mutation records are more than any device holds");
  const size_t hdr_bytes = slots * n * sizeof(GList), ref_bytes = slots * L, arena_bytes = records * sizeof(MutRec);
  st = mcc_check_room(h, w, hdr_bytes + ref_bytes + arena_bytes, "the mutations of " + std::to_string(slots) + " samples (" + mcc_mb(hdr_bytes) + " of list headers, " + mcc_mb(ref_bytes) + " of reference sequences of " + std::to_string(L) +
                                                                 " sites, " + mcc_mb(arena_bytes) + " for " + std::to_string(mutation_records) + " records)");
  if (st) return st;
  HIP_TRY(X.mut_hdr.alloc(slots * n)); HIP_TRY(X.mut_ref.alloc(slots * L)); HIP_TRY(X.mut_arena.alloc(records));
  X.mut_capacity = mutation_records; X.mut_used = 0; X.mut_L = h->L; X.mut_slots = X.capacity; X.mut_n = X.n;
  X.mut_base.assign(slots, -1); X.mut_len.assign(slots, 0);
  return EMAT_OK;
}

/* (header: emat_tree_samples_mutation_info) */
emat_status emat_tree_samples_mutation_info(emat_backend* h, int64_t* records_used, int64_t* records_capacity, int32_t* num_sites) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = gt_require(h, false, true); if (st) return st;
  if (records_used) *records_used = h->mcc.mut_used;
  if (records_capacity) *records_capacity = h->mcc.mut_capacity;
  if (num_sites) *num_sites = h->mcc.mut_L;
  return EMAT_OK;
}

/* one slot's mutations back as CSR in node order, and its reference sequence (header: emat_tree_sample_get_mutations) */
emat_status emat_tree_sample_get_mutations(emat_backend* h, int32_t index, int32_t* mut_offset, int32_t* site, uint8_t* from, uint8_t* to, double* t, int64_t capacity, uint8_t* ref_sequence, int64_t* num_mutations) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_sample_get_mutations";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  if (X.mut_capacity == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_tree_samples_reserve_mutations first (this store keeps topology and times only)");
  if (index < 0 || index >= X.count) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": sample " + std::to_string(index) + " is outside the valid range [0, " + std::to_string(X.count) + ")");
  if (X.mut_base[(size_t)index] < 0) return fail(h, EMAT_ERR_STATE, w + ": sample " + std::to_string(index) + " was pushed without mutations (emat_tree_sample_push_flat)");
  const size_t n = (size_t)X.n, L = (size_t)X.mut_L, len = (size_t)X.mut_len[(size_t)index];
  if (num_mutations) *num_mutations = (int64_t)len;
  const bool records = site || from || to || t;
  if (records && capacity < (int64_t)len) return fail(h, EMAT_ERR_CAPACITY, w + ": sample " + std::to_string(index) + " has " + std::to_string(len) + " mutations, room for " + std::to_string(capacity));
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (ref_sequence) HIP_TRY(hipMemcpy(ref_sequence, X.mut_ref.p + (size_t)index * L, L, hipMemcpyDeviceToHost));
  if (!mut_offset && !records) return EMAT_OK;
  std::vector<GList> hdr(n); std::vector<MutRec> rec(len);
  HIP_TRY(hipMemcpy(hdr.data(), X.mut_hdr.p + (size_t)index * n, n * sizeof(GList), hipMemcpyDeviceToHost));
  if (len && records) HIP_TRY(hipMemcpy(rec.data(), X.mut_arena.p + X.mut_base[(size_t)index], len * sizeof(MutRec), hipMemcpyDeviceToHost));
  size_t km = 0;
  if (mut_offset) mut_offset[0] = 0;
  for (size_t v = 0; v < n; ++v) {   // the segment holds the lists in the order the parts wrote them: back into node order
    if ((size_t)hdr[v].off + hdr[v].cnt > len || km + hdr[v].cnt > len) return fail(h, EMAT_ERR_INTERNAL, w + ": a list of sample " + std::to_string(index) + " lies outside its segment");
    for (uint32_t k = 0; k < hdr[v].cnt; ++k, ++km) {
      const MutRec& r = rec[records ? hdr[v].off + k : 0];
      if (site) site[km] = r.site;
      if (from) from[km] = r.from;
      if (to) to[km] = r.to;
      if (t) t[km] = r.t;
    }
    if (mut_offset) mut_offset[v + 1] = (int32_t)km;
  }
  return EMAT_OK;
}

emat_status emat_tree_samples_count(emat_backend* h, int32_t* count, int32_t* capacity, int32_t* num_nodes) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  if (count) *count = h->mcc.count;
  if (capacity) *capacity = h->mcc.capacity;
  if (num_nodes) *num_nodes = h->mcc.n;
  return EMAT_OK;
}

/* (header: emat_tree_samples_clear) */
emat_status emat_tree_samples_clear(emat_backend* h) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  X.count = 0; X.derived_M = 0; X.is_tip.clear(); X.mut_used = 0;   // (the arena is handed out afresh; its room stays)
  if (X.capacity > 0 && h->gt.resident && h->gt.n != X.n) return mcc_store_alloc(h, "emat_tree_samples_clear", X.capacity, h->gt.n);   // the store follows the resident tree's node count
  return EMAT_OK;
}

/* (header: emat_tree_sample_get) */
emat_status emat_tree_sample_get(emat_backend* h, int32_t index, int32_t* parent, int32_t* child0, int32_t* child1, double* t, int32_t* root) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_sample_get";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  if (index < 0 || index >= X.count) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": sample " + std::to_string(index) + " is outside the valid range [0, " + std::to_string(X.count) + ")");
  const size_t o = (size_t)index * (size_t)X.n, n = (size_t)X.n;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (parent) HIP_TRY(hipMemcpy(parent, X.parent.p + o, n * 4, hipMemcpyDeviceToHost));
  if (child0) HIP_TRY(hipMemcpy(child0, X.c0.p + o, n * 4, hipMemcpyDeviceToHost));
  if (child1) HIP_TRY(hipMemcpy(child1, X.c1.p + o, n * 4, hipMemcpyDeviceToHost));
  if (t) HIP_TRY(hipMemcpy(t, X.t.p + o, n * 8, hipMemcpyDeviceToHost));
  if (root) HIP_TRY(hipMemcpy(root, X.root.p + index, 4, hipMemcpyDeviceToHost));
  return EMAT_OK;
}

/* derive_mcc_tree (mcc_tree.cpp:58-156) + Mcc_tree::calculate_derived_quantities (:158-179) (header: emat_mcc_derive) */
emat_status emat_mcc_derive(emat_backend* h, int32_t first, int32_t count, int32_t stride, uint64_t seed, emat_mcc_result* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_mcc_derive";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  if (count < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": the number of base trees must be positive (CHECK_GT(M, 0)), not " + std::to_string(count));
  if (stride < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": stride must be positive, not " + std::to_string(stride));
  if (first < 0 || (int64_t)first + (int64_t)(count - 1) * stride >= X.count)
    return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": samples " + std::to_string(first) + ", " + std::to_string(first) + " + " + std::to_string(stride) + ", ... (" + std::to_string(count) + " of them) are outside the valid range [0, " + std::to_string(X.count) + ")");
  const int32_t n = X.n, M = count;
  const size_t Mn = (size_t)M * (size_t)n, hist_words = (size_t)M * ((size_t)M + 1);
  X.derived_M = 0;
  if (X.fp.n < Mn || X.hist.n < hist_words) {
    st = mcc_check_room(h, w, Mn * k_mcc_derive_bytes_per_node + hist_words * 4, "a derivation over " + std::to_string(M) + " samples of " + std::to_string(n) + " nodes"); if (st) return st;
  }
  HIP_TRY(X.fp.alloc_roomy(Mn)); HIP_TRY(X.ntips.alloc_roomy(Mn)); HIP_TRY(X.arrive.alloc_roomy(Mn)); HIP_TRY(X.corr.alloc_roomy(Mn)); HIP_TRY(X.exact.alloc_roomy(Mn));
  HIP_TRY(X.hist.alloc_roomy(hist_words)); HIP_TRY(X.info.alloc(4));
  HIP_TRY(X.support.alloc_roomy((size_t)n)); HIP_TRY(X.t_out.alloc_roomy((size_t)n)); HIP_TRY(X.t_mrca.alloc_roomy((size_t)n)); HIP_TRY(X.num_exact.alloc_roomy((size_t)n));
  const MccStore S = mcc_store_dev(X);
  const MccPick pick{first, stride, M};
  const dim3 b256(256), per_node((unsigned)((n + 255) / 256), (unsigned)std::min(M, 65535));
  int32_t info[4] = {0, 0, 0, 0};
  // step 2
  HIP_TRY(hipMemsetAsync(X.fp.p, 0, Mn * 8, h->stream)); HIP_TRY(hipMemsetAsync(X.ntips.p, 0, Mn * 4, h->stream)); HIP_TRY(hipMemsetAsync(X.info.p, 0, 16, h->stream));
  hipLaunchKernelGGL(k_mcc_climb_clades, per_node, b256, 0, h->stream, S, pick, (unsigned long long)seed, X.fp.p, X.ntips.p, X.info.p);
  HIP_TRY(hipGetLastError());
  // step 3: the table, grown and refilled until every key is in and at most half the slots are taken
  int log2_slots = h->cfg_mcc_table_log2;
  if (log2_slots <= 0) { log2_slots = 10; while (((size_t)1 << log2_slots) < 4 * (size_t)n) ++log2_slots; log2_slots = std::max(log2_slots, X.table_log2_hint); }   // (at least what the last derivation ended with)
  log2_slots = std::max(2, std::min(log2_slots, 40));
  X.table_regrows = 0;
  for (;;) {
    const size_t slots = (size_t)1 << log2_slots;
    if (X.keys.n < slots) { st = mcc_check_room(h, w, slots * 12, "a table of clade counts of " + std::to_string(slots) + " slots"); if (st) return st; }
    HIP_TRY(X.keys.alloc(slots)); HIP_TRY(X.counts.alloc(slots));
    HIP_TRY(hipMemsetAsync(X.keys.p, 0, slots * 8, h->stream)); HIP_TRY(hipMemsetAsync(X.counts.p, 0, slots * 4, h->stream));
    HIP_TRY(hipMemsetAsync(X.info.p + 1, 0, 8, h->stream));
    MccTable T{}; T.keys = X.keys.p; T.counts = X.counts.p; T.info = X.info.p; T.mask = (uint32_t)(slots - 1); T.shift = 64 - log2_slots;
    const unsigned blocks = (unsigned)std::min<size_t>((Mn + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_mcc_count, dim3(blocks), b256, 0, h->stream, n, M, (const unsigned long long*)X.fp.p, T);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(info, X.info.p, 16, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    st = mcc_status_check(h, w, info[0]); if (st) return st;
    if (!(info[0] & k_mcc_table_full) && 2 * (size_t)info[1] <= slots) { X.table = T; X.table_log2_hint = h->cfg_mcc_table_log2 > 0 ? 0 : log2_slots; break; }
    if (log2_slots >= 32) return fail(h, EMAT_ERR_CAPACITY, w + ": the table of clade counts would need more than 2^32 slots");
    log2_slots = std::min(32, log2_slots + 2); ++X.table_regrows;
    HIP_TRY(hipMemsetAsync(X.info.p, 0, 4, h->stream));
  }
  // step 4
  HIP_TRY(hipMemsetAsync(X.hist.p, 0, hist_words * 4, h->stream));
  hipLaunchKernelGGL(k_mcc_hist, dim3((unsigned)std::min((n + 255) / 256, 64), (unsigned)std::min(M, 65535)), b256, 0, h->stream, S, pick, (const unsigned long long*)X.fp.p, X.table, X.hist.p);
  HIP_TRY(hipGetLastError());
  std::vector<int32_t> hist(hist_words);
  HIP_TRY(hipMemcpyAsync(hist.data(), X.hist.p, hist_words * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(info, X.info.p, 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  st = mcc_status_check(h, w, info[0]); if (st) return st;
  // log(i / M) as the reference tabulates it (:78-85); per sample the sum in ascending count; the master is the first maximum (std::max_element)
  std::vector<double> log_i_over_M((size_t)M + 1, 0.0);
  const double log_M = std::log((double)M);
  for (int i = 1; i <= M; ++i) log_i_over_M[(size_t)i] = std::log((double)i) - log_M;
  int32_t master = 0; double best = 0.0;
  std::vector<double> log_cc((size_t)M);
  for (int k = 0; k < M; ++k) {
    double s = 0.0;
    for (int c = 1; c <= M; ++c) { const int32_t m = hist[(size_t)k * ((size_t)M + 1) + (size_t)c]; if (m) s += (double)m * log_i_over_M[(size_t)c]; }
    log_cc[(size_t)k] = s;
    if (k == 0 || s > best) { best = s; master = k; }
  }
  // steps 5 and 6
  HIP_TRY(hipMemsetAsync(X.arrive.p, 0, Mn * 4, h->stream)); HIP_TRY(hipMemsetAsync(X.corr.p, 0xff, Mn * 4, h->stream)); HIP_TRY(hipMemsetAsync(X.exact.p, 0, Mn, h->stream));
  hipLaunchKernelGGL(k_mcc_climb_corr, per_node, b256, 0, h->stream, S, pick, master, (const unsigned long long*)X.fp.p, (const int32_t*)X.ntips.p, X.arrive.p, X.corr.p, X.exact.p, X.info.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(info, X.info.p, 16, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));   // (k_mcc_derived follows corr into the samples: only after the climb is known to have stayed inside the tree)
  st = mcc_status_check(h, w, info[0]); if (st) return st;
  hipLaunchKernelGGL(k_mcc_derived, dim3((unsigned)((n + 255) / 256)), b256, 0, h->stream, S, pick, (const int32_t*)X.corr.p, (const uint8_t*)X.exact.p, X.support.p, X.t_out.p, X.t_mrca.p, X.num_exact.p);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(h->stream));
  const int32_t master_slot = first + master * stride;
  const size_t mo = (size_t)master_slot * (size_t)n;
  out->master_position = master; out->master_index = master_slot;
  if (out->log_cc) std::copy(log_cc.begin(), log_cc.end(), out->log_cc);
  if (out->parent) HIP_TRY(hipMemcpy(out->parent, X.parent.p + mo, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (out->child0) HIP_TRY(hipMemcpy(out->child0, X.c0.p + mo, (size_t)n * 4, hipMemcpyDeviceToHost));
  if (out->child1) HIP_TRY(hipMemcpy(out->child1, X.c1.p + mo, (size_t)n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(&out->root, X.root.p + master_slot, 4, hipMemcpyDeviceToHost));
  if (out->support) HIP_TRY(hipMemcpy(out->support, X.support.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (out->t) HIP_TRY(hipMemcpy(out->t, X.t_out.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (out->t_mrca) HIP_TRY(hipMemcpy(out->t_mrca, X.t_mrca.p, (size_t)n * 8, hipMemcpyDeviceToHost));
  if (out->num_exact) HIP_TRY(hipMemcpy(out->num_exact, X.num_exact.p, (size_t)n * 4, hipMemcpyDeviceToHost));
  out->num_distinct_clades = info[1] + (info[2] > 0 ? 1 : 0); out->table_slots = (int64_t)X.table.mask + 1; out->table_regrows = X.table_regrows;
  X.derived_M = M; X.derived_n = n; X.derived_first = first; X.derived_stride = stride; X.derived_master = master;
  return EMAT_OK;
}

/* corresponding_node_to (mcc_tree.h:91-98) for every MCC node (header: emat_mcc_get_correspondence) */
emat_status emat_mcc_get_correspondence(emat_backend* h, int32_t k, int32_t* node_in_sample, uint8_t* is_exact) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_mcc_get_correspondence";
  emat_status st = gt_require(h, false, true); if (st) return st;
  MccHost& X = h->mcc;
  if (X.derived_M == 0) return fail(h, EMAT_ERR_STATE, w + ": emat_mcc_derive first (its table is dropped by the next derive, emat_tree_samples_clear and emat_tree_samples_reserve)");
  if (k < 0 || k >= X.derived_M) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": base tree " + std::to_string(k) + " is outside the valid range [0, " + std::to_string(X.derived_M) + ")");
  const size_t o = (size_t)k * (size_t)X.derived_n, n = (size_t)X.derived_n;
  if (node_in_sample) HIP_TRY(hipMemcpy(node_in_sample, X.corr.p + o, n * 4, hipMemcpyDeviceToHost));
  if (is_exact) HIP_TRY(hipMemcpy(is_exact, X.exact.p + o, n, hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // extern "C"
#endif  // EMAT_MCC_HOST_HPP_
