// emat_align_host.hpp -- host side of the alignment store (emat_align_kernels.hpp): argument and state checks, sizes, the launches, and the one
// thing that stays on the host because it is a walk over a few bytes a row: which rows are tips (valid and dated, in input order).
//
// Included by emat_backend.hip after its entry points, after emat_mcc_host.hpp (mcc_check_room, mcc_mb).
#ifndef EMAT_ALIGN_HOST_HPP_
#define EMAT_ALIGN_HOST_HPP_

namespace {

// What every call on the store starts with.
emat_status al_require(emat_backend* h, const std::string& w, bool need_bound) {
  if (h->host_only) return no_device(h);
  if (!bind_device(h)) return fail(h, EMAT_ERR_HIP, "hipSetDevice failed");
  if (need_bound && !h->al.bound) return fail(h, EMAT_ERR_STATE, w + ": emat_align_begin first");
  return EMAT_OK;
}

AlignStore al_store(emat_backend* h) { return AlignStore{(int32_t)h->L, h->al.row_bytes, h->al.packed.p, h->al.bad.p, h->al.counts.p}; }

int al_which_row_buffer(const AlignHost& X, const uint8_t* p) {
  for (int k = 0; k < 2; ++k) if (X.row_buf[k].p && p >= X.row_buf[k].p && p < X.row_buf[k].p + X.row_buf[k].cap) return k;
  return -1;
}

}  // namespace

extern "C" {

emat_status emat_align_begin(emat_backend* h, int64_t max_rows) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_align_begin";
  emat_status st = al_require(h, w, false); if (st) return st;
  if (max_rows < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": max_rows is negative");
  if (max_rows > (int64_t)INT32_MAX) return fail(h, EMAT_ERR_CAPACITY, w + ": rows are numbered in int32, " + std::to_string(max_rows) + " are too many");
  AlignHost& X = h->al;
  HIP_TRY(hipStreamSynchronize(h->stream));
  X.release(); X.drop_attached();
  if (max_rows == 0) return EMAT_OK;
  const size_t L = (size_t)h->L, row_bytes = (L + 1) / 2;
  const size_t packed_bytes = (size_t)max_rows * row_bytes + k_al_row_pad, bytes = packed_bytes + (size_t)max_rows * 8 + L * 16;
  st = mcc_check_room(h, w, bytes, std::to_string(max_rows) + " rows of " + std::to_string(L) + " sites (" + mcc_mb(packed_bytes) + " of packed codes, " + mcc_mb(L * 16) + " of counts)");
  if (st) return st;
  HIP_TRY(X.packed.alloc(packed_bytes)); HIP_TRY(X.bad.alloc((size_t)max_rows)); HIP_TRY(X.counts.alloc(L * 4)); HIP_TRY(X.ref.alloc(L + 2 * k_al_lane_sites));
  HIP_TRY(hipMemsetAsync(X.bad.p, 0xFF, (size_t)max_rows * 8, h->stream));
  HIP_TRY(hipMemsetAsync(X.counts.p, 0, L * 16, h->stream));
  HIP_TRY(hipMemsetAsync(X.ref.p, 0, L + 2 * k_al_lane_sites, h->stream));
  X.row_bytes = (int64_t)row_bytes; X.max_rows = max_rows; X.rows = 0; X.bound = true; X.finished = false;
  return EMAT_OK;
}

emat_status emat_align_row_buffer(emat_backend* h, int32_t which, int64_t bytes, uint8_t** buffer) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_align_row_buffer";
  emat_status st = al_require(h, w, false); if (st) return st;
  if (which < 0 || which > 1 || bytes < 0 || !buffer) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": which is 0 or 1, bytes >= 0, buffer not null");
  AlignHost& X = h->al;
  if (X.row_ev_pending[which]) { HIP_TRY(hipEventSynchronize(X.row_ev[which])); X.row_ev_pending[which] = false; }
  HIP_TRY(X.row_buf[which].resize((size_t)bytes));
  *buffer = X.row_buf[which].p;
  return EMAT_OK;
}

emat_status emat_align_push_rows(emat_backend* h, int32_t num_rows, const uint8_t* chars, int64_t row_stride) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_align_push_rows";
  emat_status st = al_require(h, w, true); if (st) return st;
  AlignHost& X = h->al;
  if (num_rows < 0) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": num_rows is negative");
  if (row_stride < h->L) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": row_stride " + std::to_string(row_stride) + " is smaller than the " + std::to_string(h->L) + " sites of a row");
  if (num_rows == 0) return EMAT_OK;
  if (!chars) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": chars must not be null");
  if (X.rows + num_rows > X.max_rows)
    return fail(h, EMAT_ERR_CAPACITY, w + ": " + std::to_string(num_rows) + " rows on top of " + std::to_string(X.rows) + " are more than the " + std::to_string(X.max_rows) + " reserved: nothing is pushed");
  const int64_t site_tiles = ((int64_t)h->L + k_al_tile_sites - 1) / k_al_tile_sites, row_tiles = ((int64_t)num_rows + k_al_tile_rows - 1) / k_al_tile_rows;
  if (site_tiles * row_tiles > (int64_t)INT32_MAX) return fail(h, EMAT_ERR_CAPACITY, w + ": " + std::to_string(num_rows) + " rows in one call take more than 2^31 workgroups: push fewer at a time");
  const size_t bytes = (size_t)(num_rows - 1) * (size_t)row_stride + (size_t)h->L;
  HIP_TRY(X.chars.alloc_roomy(bytes));
  for (hipEvent_t* e : {&X.row_ev[0], &X.row_ev[1], &X.copy_ev}) if (!*e) HIP_TRY(hipEventCreateWithFlags(e, hipEventDisableTiming));
  const int own = al_which_row_buffer(X, chars);
  HIP_TRY(hipMemcpyAsync(X.chars.p, chars, bytes, hipMemcpyHostToDevice, h->stream));
  hipEvent_t copied = own >= 0 ? X.row_ev[own] : X.copy_ev;
  HIP_TRY(hipEventRecord(copied, h->stream));
  if (own >= 0) X.row_ev_pending[own] = true;
  const AlignStore s = al_store(h);
  hipLaunchKernelGGL(k_al_code, dim3((unsigned)(site_tiles * row_tiles)), dim3(k_al_threads), 0, h->stream, s, X.chars.p, row_stride, X.rows, num_rows, (int32_t)site_tiles);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_al_count, dim3((unsigned)(site_tiles * row_tiles)), dim3(k_al_threads), 0, h->stream, s, X.rows, num_rows, (int32_t)site_tiles);
  HIP_TRY(hipGetLastError());
  X.rows += num_rows; X.finished = false;
  if (own < 0) HIP_TRY(hipEventSynchronize(copied));   // (the caller's memory is the caller's again)
  return EMAT_OK;
}

emat_status emat_align_finish(emat_backend* h, const uint8_t* given_ref, const uint8_t* row_dated, emat_align_report* out) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const std::string w = "emat_align_finish";
  emat_status st = al_require(h, w, true); if (st) return st;
  AlignHost& X = h->al;
  const int32_t L = (int32_t)h->L;
  if (given_ref) for (int32_t l = 0; l < L; ++l) if (given_ref[l] > 3) return fail(h, EMAT_ERR_INVALID_ARGUMENT, w + ": given_ref[" + std::to_string(l) + "] = " + std::to_string((int)given_ref[l]) + ": states are 0..3");
  X.finished = false;
  if (given_ref) HIP_TRY(hipMemcpyAsync(X.ref.p, given_ref, (size_t)L, hipMemcpyHostToDevice, h->stream));
  else { hipLaunchKernelGGL(k_al_consensus, dim3((unsigned)((L + k_al_threads - 1) / k_al_threads)), dim3(k_al_threads), 0, h->stream, X.counts.p, X.ref.p, L); HIP_TRY(hipGetLastError()); }
  // which rows are tips
  const size_t R = (size_t)X.rows;
  std::vector<unsigned long long> bad(R);
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (R) HIP_TRY(hipMemcpy(bad.data(), X.bad.p, R * 8, hipMemcpyDeviceToHost));
  emat_align_report rep{};
  rep.num_rows = X.rows;
  X.row_status.assign(R, 0); X.row_bad_site.assign(R, -1); X.row_bad_byte.assign(R, 0); X.row_not_n.assign(R, 0);
  std::vector<int32_t> tip_row;
  for (size_t r = 0; r < R; ++r) {
    if (bad[r] != k_al_row_ok) { X.row_status[r] = -2; X.row_bad_site[r] = (int32_t)(bad[r] >> 8); X.row_bad_byte[r] = (uint8_t)(bad[r] & 0xFF); ++rep.num_invalid; }
    else if (row_dated && !row_dated[r]) { X.row_status[r] = -1; ++rep.num_undated; }
    else { X.row_status[r] = (int32_t)tip_row.size(); tip_row.push_back((int32_t)r); }
  }
  const int32_t T = (int32_t)tip_row.size();
  rep.num_tips = T;
  HIP_TRY(X.tip_row.alloc_roomy((size_t)T)); HIP_TRY(X.n_delta.alloc_roomy((size_t)T)); HIP_TRY(X.n_iv.alloc_roomy((size_t)T)); HIP_TRY(X.n_not_n.alloc_roomy((size_t)T));
  HIP_TRY(X.delta_off.alloc_roomy((size_t)T + 1)); HIP_TRY(X.miss_off.alloc_roomy((size_t)T + 1)); HIP_TRY(X.totals.alloc(2));
  if (T) HIP_TRY(hipMemcpyAsync(X.tip_row.p, tip_row.data(), (size_t)T * 4, hipMemcpyHostToDevice, h->stream));
  AlignTips a{};
  a.L = L; a.row_bytes = X.row_bytes; a.num_tips = T; a.packed = X.packed.p; a.ref = X.ref.p; a.tip_row = X.tip_row.p;
  a.n_delta = X.n_delta.p; a.n_iv = X.n_iv.p; a.n_not_n = X.n_not_n.p; a.delta_off = X.delta_off.p; a.miss_off = X.miss_off.p;
  if (T) { hipLaunchKernelGGL(k_al_tip_count, dim3((unsigned)T), dim3(k_al_wave), 0, h->stream, a); HIP_TRY(hipGetLastError()); }
  hipLaunchKernelGGL(k_al_scan, dim3(1), dim3(k_al_scan_threads), 0, h->stream, X.n_delta.p, X.n_iv.p, T, X.delta_off.p, X.miss_off.p, X.totals.p);
  HIP_TRY(hipGetLastError());
  long long totals[2] = {0, 0};
  std::vector<int32_t> not_n((size_t)T);
  HIP_TRY(hipStreamSynchronize(h->stream));   // (tip_row is the host's until here)
  HIP_TRY(hipMemcpy(totals, X.totals.p, sizeof totals, hipMemcpyDeviceToHost));
  if (T) HIP_TRY(hipMemcpy(not_n.data(), X.n_not_n.p, (size_t)T * 4, hipMemcpyDeviceToHost));
  if (totals[0] > (long long)INT32_MAX || totals[1] > (long long)INT32_MAX)
    return fail(h, EMAT_ERR_CAPACITY, w + ": " + std::to_string(totals[0]) + " deltas and " + std::to_string(totals[1]) + " missing intervals over " + std::to_string(T) + " tips: the offsets of emat_tip_descs are int32");
  rep.num_deltas = totals[0]; rep.num_intervals = totals[1];
  for (int32_t t = 0; t < T; ++t) { X.row_not_n[(size_t)tip_row[(size_t)t]] = not_n[(size_t)t]; rep.num_precision_loss += not_n[(size_t)t]; }
  HIP_TRY(X.delta_site.alloc_roomy((size_t)totals[0])); HIP_TRY(X.delta_to.alloc_roomy((size_t)totals[0]));
  HIP_TRY(X.miss_start.alloc_roomy((size_t)totals[1])); HIP_TRY(X.miss_end.alloc_roomy((size_t)totals[1]));
  a.delta_site = X.delta_site.p; a.delta_to = X.delta_to.p; a.miss_start = X.miss_start.p; a.miss_end = X.miss_end.p;
  if (T) { hipLaunchKernelGGL(k_al_tip_write, dim3((unsigned)T), dim3(k_al_wave), 0, h->stream, a); HIP_TRY(hipGetLastError()); }
  HIP_TRY(hipStreamSynchronize(h->stream));
  X.report = rep; X.finished = true;
  if (out) *out = rep;
  return EMAT_OK;
}

emat_status emat_align_sizes(emat_backend* h, emat_align_report* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = al_require(h, "emat_align_sizes", false); if (st) return st;
  if (!h->al.finished) return fail(h, EMAT_ERR_STATE, "emat_align_sizes: emat_align_finish first");
  *out = h->al.report;
  return EMAT_OK;
}

emat_status emat_align_get(emat_backend* h, const emat_align_arrays* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  emat_status st = al_require(h, "emat_align_get", false); if (st) return st;
  AlignHost& X = h->al;
  if (!X.finished) return fail(h, EMAT_ERR_STATE, "emat_align_get: emat_align_finish first");
  const size_t T = (size_t)X.report.num_tips, nd = (size_t)X.report.num_deltas, ni = (size_t)X.report.num_intervals, L = (size_t)h->L;
  HIP_TRY(hipStreamSynchronize(h->stream));
  if (out->delta_offset) HIP_TRY(hipMemcpy(out->delta_offset, X.delta_off.p, (T + 1) * 4, hipMemcpyDeviceToHost));
  if (out->miss_offset) HIP_TRY(hipMemcpy(out->miss_offset, X.miss_off.p, (T + 1) * 4, hipMemcpyDeviceToHost));
  if (out->delta_site && nd) HIP_TRY(hipMemcpy(out->delta_site, X.delta_site.p, nd * 4, hipMemcpyDeviceToHost));
  if (out->delta_to && nd) HIP_TRY(hipMemcpy(out->delta_to, X.delta_to.p, nd, hipMemcpyDeviceToHost));
  if (out->miss_start && ni) HIP_TRY(hipMemcpy(out->miss_start, X.miss_start.p, ni * 4, hipMemcpyDeviceToHost));
  if (out->miss_end && ni) HIP_TRY(hipMemcpy(out->miss_end, X.miss_end.p, ni * 4, hipMemcpyDeviceToHost));
  if (out->ref_sequence) HIP_TRY(hipMemcpy(out->ref_sequence, X.ref.p, L, hipMemcpyDeviceToHost));
  if (out->counts) HIP_TRY(hipMemcpy(out->counts, X.counts.p, L * 16, hipMemcpyDeviceToHost));
  if (out->row_status) std::copy(X.row_status.begin(), X.row_status.end(), out->row_status);
  if (out->row_bad_site) std::copy(X.row_bad_site.begin(), X.row_bad_site.end(), out->row_bad_site);
  if (out->row_bad_byte) std::copy(X.row_bad_byte.begin(), X.row_bad_byte.end(), out->row_bad_byte);
  if (out->row_precision_loss) std::copy(X.row_not_n.begin(), X.row_not_n.end(), out->row_precision_loss);
  return EMAT_OK;
}

emat_status emat_align_attach(emat_backend* h, void* record, void (*destroy)(void*)) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  h->al.drop_attached();
  h->al.attached = record; h->al.attached_free = destroy;
  return EMAT_OK;
}
void* emat_align_attached(const emat_backend* h) { return h ? h->al.attached : nullptr; }
int32_t emat_align_num_sites(const emat_backend* h) { return h ? (int32_t)h->L : 0; }
emat_status emat_align_refuse(emat_backend* h, emat_status status, const char* text) { return h ? fail(h, status, text ? text : "") : EMAT_ERR_INVALID_ARGUMENT; }

}  // extern "C"

#endif  // EMAT_ALIGN_HOST_HPP_
