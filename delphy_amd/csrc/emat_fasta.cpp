// emat_fasta.cpp -- aligned FASTA in (include/emat_host.h: emat_seq_id_date_range, emat_fasta_*): the framing of records and the dates in
// their ids (emat_fasta_pure.hpp), and the hand-over of the rows, chunk by chunk, to the alignment store of the backend.  Plain host code
// above the engine boundary: it reaches the handle through include/emat_backend.h alone.
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cmath>
#include <algorithm>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/emat_host.h"
#include "emat_fasta_pure.hpp"

namespace {

using namespace emat;

// What a framing leaves on the handle (emat_align_attach).
struct FastaRecords {
  std::vector<std::string> names; std::vector<int64_t> lengths; std::vector<float> t_min, t_max; std::vector<uint8_t> dated;
  emat_fasta_report report{};
  void add(const std::string& id, int64_t len) {
    double a = 0.0, b = 0.0;
    const bool ok = seq_id_date_range(id.data(), id.size(), &a, &b);
    const float nan = std::numeric_limits<float>::quiet_NaN();
    names.push_back(id); lengths.push_back(len); dated.push_back(ok ? 1 : 0);
    t_min.push_back(ok ? (float)a : nan); t_max.push_back(ok ? (float)b : nan);   // (floats, as Tip_desc holds them: cmdline.cpp:74-75)
    ++report.num_records; report.num_dated += ok; report.names_bytes += (int64_t)id.size() + 1;
  }
};
void destroy_records(void* p) { delete (FastaRecords*)p; }

const std::string k_who = "emat_fasta_load: ";

// fasta_to_maple's complaint (cmdline.cpp:38-45), against the handle's L
emat_status refuse_length(emat_backend* h, const FastaRecords& R, const std::string& id, int64_t len, int32_t L) {
  const std::string first = R.names.empty() ? "the handle" : "'" + R.names[0] + "'";
  const int64_t first_len = R.names.empty() ? L : R.lengths[0];
  return emat_align_refuse(h, EMAT_ERR_INVALID_ARGUMENT, (k_who + "sequences have different lengths: '" + id + "' has " + std::to_string(len) + " sites, while " + first + " has " +
                                                            std::to_string(first_len) + " (the handle has " + std::to_string(L) + ").  Are these sequences aligned?").c_str());
}
emat_status refuse_empty(emat_backend* h) { return emat_align_refuse(h, EMAT_ERR_INVALID_ARGUMENT, (k_who + "Input has no sequences!").c_str()); }

// Framing alone: names, lengths, dates, and the two refusals.
emat_status frame_only(emat_backend* h, const uint8_t* text, int64_t len, FastaRecords& R) {
  const int32_t L = emat_align_num_sites(h);
  FastaFramer f(text, len);
  std::string id; int64_t n = 0;
  while (f.next(&id, nullptr, 0, &n)) {
    if (n != L) return refuse_length(h, R, id, n, L);
    R.add(id, n);
  }
  return R.report.num_records ? EMAT_OK : refuse_empty(h);
}

emat_status load_memory(emat_backend* h, const uint8_t* text, int64_t len, const uint8_t* given_ref, int32_t chunk_rows, emat_fasta_report* out) {
  if (!h || (!text && len > 0) || len < 0 || chunk_rows < 0) return EMAT_ERR_INVALID_ARGUMENT;
  const int32_t L = emat_align_num_sites(h);
  auto R = std::make_unique<FastaRecords>();
  emat_status st = emat_align_begin(h, fasta_count_headers(text, len));
  if (st == EMAT_ERR_NO_DEVICE) {   // as far as it goes without one: the framing and its refusals
    const emat_status fs = frame_only(h, text, len, *R); if (fs) return fs;
    if (out) *out = R->report;
    (void)emat_align_attach(h, R.release(), destroy_records);
    return emat_align_refuse(h, st, (k_who + "the text is framed; its rows need a device (host-only handle: the engine has no CPU fallback)").c_str());
  }
  if (st) return st;
  if (chunk_rows == 0) chunk_rows = (int32_t)std::max<int64_t>(1, std::min<int64_t>(4096, ((int64_t)32 << 20) / L));
  const int64_t buf_bytes = (int64_t)chunk_rows * L;
  auto give_up = [&](emat_status why, bool keep_text) {   // release the store, keep the refusal's text
    const std::string text_now = emat_last_error(h);
    (void)emat_align_begin(h, 0);
    return keep_text ? emat_align_refuse(h, why, text_now.c_str()) : why;
  };
  FastaFramer f(text, len);
  std::string id; int64_t n = 0; int which = 0; int32_t in_buf = 0;
  uint8_t* buf = nullptr;
  st = emat_align_row_buffer(h, which, buf_bytes, &buf); if (st) return give_up(st, true);
  for (;;) {
    const bool more = f.next(&id, buf + (int64_t)in_buf * L, L, &n);
    if (more) {
      if (n != L) { (void)refuse_length(h, *R, id, n, L); return give_up(EMAT_ERR_INVALID_ARGUMENT, true); }
      R->add(id, n); ++in_buf;
    }
    if (in_buf == chunk_rows || (!more && in_buf > 0)) {   // the framing of the next chunk overlaps this one's copy
      st = emat_align_push_rows(h, in_buf, buf, L); if (st) return give_up(st, true);
      which ^= 1; in_buf = 0;
      if (more) { st = emat_align_row_buffer(h, which, buf_bytes, &buf); if (st) return give_up(st, true); }
    }
    if (!more) break;
  }
  if (R->report.num_records == 0) { (void)refuse_empty(h); return give_up(EMAT_ERR_INVALID_ARGUMENT, true); }
  st = emat_align_finish(h, given_ref, R->dated.data(), &R->report.rows); if (st) return give_up(st, true);
  if (out) *out = R->report;
  return emat_align_attach(h, R.release(), destroy_records);
}

}  // namespace

extern "C" {

emat_status emat_seq_id_date_range(const char* id, double* t_min, double* t_max, int32_t* ok) {
  if (!id || !t_min || !t_max || !ok) return EMAT_ERR_INVALID_ARGUMENT;
  double a = 0.0, b = 0.0;
  *ok = seq_id_date_range(id, strlen(id), &a, &b) ? 1 : 0;
  if (*ok) { *t_min = a; *t_max = b; }
  return EMAT_OK;
}

emat_status emat_fasta_frame_memory(emat_backend* h, const uint8_t* text, int64_t len, emat_fasta_report* out) {
  if (!h || (!text && len > 0) || len < 0) return EMAT_ERR_INVALID_ARGUMENT;
  auto R = std::make_unique<FastaRecords>();
  emat_status st = frame_only(h, text, len, *R); if (st) return st;
  if (out) *out = R->report;
  return emat_align_attach(h, R.release(), destroy_records);
}

emat_status emat_fasta_load_memory(emat_backend* h, const uint8_t* text, int64_t len, const uint8_t* given_ref, int32_t chunk_rows, emat_fasta_report* out) {
  return load_memory(h, text, len, given_ref, chunk_rows, out);
}

emat_status emat_fasta_load(emat_backend* h, const char* path, const uint8_t* given_ref, int32_t chunk_rows, emat_fasta_report* out) {
  if (!h || !path) return EMAT_ERR_INVALID_ARGUMENT;
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return emat_align_refuse(h, EMAT_ERR_IO, (k_who + "cannot open '" + path + "'").c_str());
  struct stat sb;
  if (fstat(fd, &sb) != 0) { close(fd); return emat_align_refuse(h, EMAT_ERR_IO, (k_who + "cannot stat '" + path + "'").c_str()); }
  const int64_t len = (int64_t)sb.st_size;
  void* m = len > 0 ? mmap(nullptr, (size_t)len, PROT_READ, MAP_PRIVATE, fd, 0) : nullptr;
  close(fd);
  if (len > 0 && m == MAP_FAILED) return emat_align_refuse(h, EMAT_ERR_IO, (k_who + "cannot map '" + path + "'").c_str());
  const emat_status st = load_memory(h, (const uint8_t*)m, len, given_ref, chunk_rows, out);
  if (m) munmap(m, (size_t)len);
  return st;
}

emat_status emat_fasta_sizes(emat_backend* h, emat_fasta_report* out) {
  if (!h || !out) return EMAT_ERR_INVALID_ARGUMENT;
  const FastaRecords* R = (const FastaRecords*)emat_align_attached(h);
  if (!R) return emat_align_refuse(h, EMAT_ERR_STATE, "emat_fasta_sizes: emat_fasta_load (or emat_fasta_frame_memory) first");
  *out = R->report;
  return EMAT_OK;
}

emat_status emat_fasta_get(emat_backend* h, char* names, int64_t* lengths, float* t_min, float* t_max, uint8_t* dated) {
  if (!h) return EMAT_ERR_INVALID_ARGUMENT;
  const FastaRecords* R = (const FastaRecords*)emat_align_attached(h);
  if (!R) return emat_align_refuse(h, EMAT_ERR_STATE, "emat_fasta_get: emat_fasta_load (or emat_fasta_frame_memory) first");
  for (size_t i = 0; i < R->names.size(); ++i) {
    if (names) { memcpy(names, R->names[i].c_str(), R->names[i].size() + 1); names += R->names[i].size() + 1; }
    if (lengths) lengths[i] = R->lengths[i];
    if (t_min) t_min[i] = R->t_min[i];
    if (t_max) t_max[i] = R->t_max[i];
    if (dated) dated[i] = R->dated[i];
  }
  return EMAT_OK;
}

}  // extern "C"
