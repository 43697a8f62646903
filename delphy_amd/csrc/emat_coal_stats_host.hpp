// emat_coal_stats_host.hpp -- the whole-tree coalescent statistics the population moves read (h->coal): the grid's rules, a caller's statistics, the resident tree's.
//
// Included by emat_backend.hip after emat_probe_host.hpp (gt_require_tree_home) and before the two population groups; the kernels: emat_skygrid_kernels.hpp.
#ifndef EMAT_COAL_STATS_HOST_HPP_
#define EMAT_COAL_STATS_HOST_HPP_

namespace {

// Statistics in the caller's arrays; a null pointer to one of these stands for "the tree in HBM".
struct CoalHostStats { int32_t first_cell, num_cells; const double* k_bar; int32_t num_inner; const double* inner_t; };

emat_status coal_check_origin(emat_backend* h, const std::string& w, double t_ref, double t_step) { return std::isfinite(t_ref) && finite_positive(t_step) ? EMAT_OK : fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "t_ref must be finite and t_step finite and positive"); }
// THE capacity rule of a grid: at most k_sky_max_cells cells, numbered within [-2^30, 2^30).
emat_status coal_check_capacity(emat_backend* h, const std::string& w, int64_t first_cell, int64_t num_cells) {
  if (num_cells > k_sky_max_cells) return fail(h, EMAT_ERR_CAPACITY, w + std::to_string(num_cells) + " cells are more than the moves hold (" + std::to_string(k_sky_max_cells) + ")");
  if (first_cell < -(1ll << 30) || first_cell + num_cells > (1ll << 30)) return fail(h, EMAT_ERR_CAPACITY, w + "the cells' numbers leave [-2^30, 2^30): choose t_ref nearer the tree");
  return EMAT_OK;
}

// What handed-in statistics must be, whatever the grid's size (nothing to check for the tree's own).
emat_status coal_check_host_values(emat_backend* h, const std::string& w, double t_ref, double t_step, const CoalHostStats* s) {
  if (!s) return EMAT_OK;
  if (s->num_cells < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_cells must be at least 1");
  if (s->num_inner < 1) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "num_inner must be at least 1");
  for (int32_t c = 0; c < s->num_cells; ++c)
    if (!std::isfinite(s->k_bar[c]) || s->k_bar[c] < 0.0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "k_bar of cell " + std::to_string(c) + " is negative or not finite");
  for (int32_t i = 0; i < s->num_inner; ++i) {
    if (!std::isfinite(s->inner_t[i])) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inner_t of node " + std::to_string(i) + " is not finite");
    const double cell = std::floor((s->inner_t[i] - t_ref) / t_step);   // Scalable_coalescent_prior::cell_for
    if (cell < (double)s->first_cell || cell >= (double)s->first_cell + (double)s->num_cells) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "inner_t of node " + std::to_string(i) + " lies outside the grid");
  }
  return EMAT_OK;
}

// Scalable_coalescent_prior's grid and the inner nodes' times of the tree in HBM, into h->coal.
emat_status coal_tree_stats(emat_backend* h, const std::string& w, double t_ref, double t_step) {
  emat_status st = gt_require_tree_home(h, false, w); if (st) return st;
  if (h->pass_pending) { st = finish_pass(h); if (st) return st; }
  CoalStatsScratch& S = h->coal;
  const GTreeDev T = h->gt.dev();
  HIP_TRY(S.extent.alloc(2)); HIP_TRY(S.count.alloc(1)); HIP_TRY(S.inner_t.alloc_roomy((size_t)h->gt.n));
  hipLaunchKernelGGL(k_skygrid_tree_extent, dim3(1), dim3(k_sky_threads), 0, h->stream, T, S.extent.p);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_skygrid_tree_inner_times, dim3(1), dim3(k_sky_threads), 0, h->stream, T, S.inner_t.p, S.count.p);
  HIP_TRY(hipGetLastError());
  double ext[2]; int32_t cnt = 0;
  HIP_TRY(hipMemcpyAsync(ext, S.extent.p, sizeof ext, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipMemcpyAsync(&cnt, S.count.p, sizeof cnt, hipMemcpyDeviceToHost, h->stream));
  HIP_TRY(hipStreamSynchronize(h->stream));
  const double c_root = std::floor((ext[0] - t_ref) / t_step), c_tip = std::floor((ext[1] - t_ref) / t_step);   // Scalable_coalescent_prior::cell_for
  if (!std::isfinite(c_root) || !std::isfinite(c_tip) || c_tip < c_root) return fail(h, EMAT_ERR_INTERNAL, w + "the resident tree's root is later than its latest tip");
  const double far = 0x1p61;   // (cell numbers beyond +-2^61 are refused as they stand at +-2^61: the sums below stay within int64_t)
  const int64_t first = (int64_t)std::min(std::max(c_root, -far), far), last = (int64_t)std::min(std::max(c_tip, -far), far);
  st = coal_check_capacity(h, w, first, last - first + 1); if (st) return st;
  S.first_cell = (int32_t)first; S.num_cells = (int32_t)(last - first + 1); S.num_inner = cnt;
  HIP_TRY(S.k_bar.alloc_roomy((size_t)S.num_cells));
  hipLaunchKernelGGL(k_skygrid_tree_k_bar, dim3((unsigned)S.num_cells), dim3(k_sky_threads), 0, h->stream, T, t_ref, t_step, S.first_cell, S.num_cells, S.k_bar.p);
  HIP_TRY(hipGetLastError());
  return EMAT_OK;
}

// The statistics a population group runs on, into h->coal: the caller's checked ones, or those of the tree in HBM where `host` is null.
emat_status coal_obtain(emat_backend* h, const std::string& w, double t_ref, double t_step, const CoalHostStats* host) {
  CoalStatsScratch& S = h->coal;
  if (!host) {
    emat_status st = coal_tree_stats(h, w, t_ref, t_step); if (st) return st;
    return S.num_inner < 1 ? fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "the resident tree has no inner node") : EMAT_OK;
  }
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (h->pass_pending) { emat_status st = finish_pass(h); if (st) return st; }
  HIP_TRY(S.k_bar.alloc_roomy((size_t)host->num_cells)); HIP_TRY(S.inner_t.alloc_roomy((size_t)host->num_inner));
  HIP_TRY(hipMemcpyAsync(S.k_bar.p, host->k_bar, (size_t)host->num_cells * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIP_TRY(hipMemcpyAsync(S.inner_t.p, host->inner_t, (size_t)host->num_inner * sizeof(double), hipMemcpyHostToDevice, h->stream));
  S.first_cell = host->first_cell; S.num_cells = host->num_cells; S.num_inner = host->num_inner;
  return EMAT_OK;
}

}  // namespace

extern "C" {

/* the whole-tree statistics of the tree in HBM (header: emat_tree_coalescent_stats) */
emat_status emat_tree_coalescent_stats(emat_backend* h, double t_ref, double t_step, int32_t* first_cell, int32_t* num_cells, double* k_bar, int32_t k_bar_capacity,
                                       double* inner_t, int32_t inner_capacity, int32_t* num_inner) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_tree_coalescent_stats: ";
  if (!first_cell || !num_cells || !num_inner) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + "first_cell, num_cells and num_inner must not be null");
  emat_status st = coal_check_origin(h, w, t_ref, t_step); if (st) return st;
  st = coal_tree_stats(h, w, t_ref, t_step); if (st) return st;
  CoalStatsScratch& S = h->coal;
  *first_cell = S.first_cell; *num_cells = S.num_cells; *num_inner = S.num_inner;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (k_bar && k_bar_capacity < S.num_cells) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, w + std::to_string(S.num_cells) + " cells, room for " + std::to_string(k_bar_capacity));
  if (k_bar) HIP_TRY(hipMemcpy(k_bar, S.k_bar.p, (size_t)S.num_cells * sizeof(double), hipMemcpyDeviceToHost));
  if (inner_t && inner_capacity < S.num_inner) return fail(h, EMAT_ERR_BUFFER_TOO_SMALL, w + std::to_string(S.num_inner) + " inner nodes, room for " + std::to_string(inner_capacity));
  if (inner_t) HIP_TRY(hipMemcpy(inner_t, S.inner_t.p, (size_t)S.num_inner * sizeof(double), hipMemcpyDeviceToHost));
  return EMAT_OK;
}

}  // extern "C"

#endif  // EMAT_COAL_STATS_HOST_HPP_
