// emat_fasta_pure.hpp -- the two pieces of FASTA input that are plain host code with nothing of the engine in them: the framing of records
// (reference core/io.cpp:14-97, read_fasta) and the date range at the end of a sequence id (core/sequence_utils.cpp:98-211,
// extract_date_range_from_sequence_id, over core/dates.cpp:12-46).  Included by emat_fasta.cpp, and by scripts/micro/fasta_host.cpp, which
// runs them under the host sanitizers.
#ifndef EMAT_FASTA_PURE_HPP_
#define EMAT_FASTA_PURE_HPP_

#include <cstdint>
#include <cstring>
#include <string>

namespace emat {

// ---- dates ------------------------------------------------------------------------------------------------------------------------
// Days from 1970-01-01 in the proleptic Gregorian calendar (the well-known era arithmetic; exact for every int year).
inline int64_t days_from_civil(int64_t y, int m, int d) {
  y -= m <= 2;
  const int64_t era = (y >= 0 ? y : y - 399) / 400;
  const int64_t yoe = y - era * 400;
  const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
  const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
  return era * 146097 + doe - 719468;
}
inline int days_in_month(int64_t y, int m) {
  static const int k[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
  return m == 2 && (y % 4 == 0 && (y % 100 != 0 || y % 400 == 0)) ? 29 : k[m - 1];
}
// 2020-01-01 is day 0 (dates.cpp:12-13)
inline double days_since_epoch(int64_t y, int m, int d) { return (double)(days_from_civil(y, m, d) - days_from_civil(2020, 1, 1)); }

inline bool all_digits(const char* s, int n) { for (int i = 0; i < n; ++i) if (s[i] < '0' || s[i] > '9') return false; return true; }
inline int digits_value(const char* s, int n) { int v = 0; for (int i = 0; i < n; ++i) v = 10 * v + (s[i] - '0'); return v; }
inline bool is_date_str(const char* s) { return all_digits(s, 4) && s[4] == '-' && all_digits(s + 5, 2) && s[7] == '-' && all_digits(s + 8, 2); }   // YYYY-MM-DD
// A month outside 1-12 or a day the month does not have is no date (the reference leaves such strings to absl::ParseCivilTime).
inline bool parse_date(const char* s, double* t) {
  const int y = digits_value(s, 4), m = digits_value(s + 5, 2), d = digits_value(s + 8, 2);
  if (m < 1 || m > 12 || d < 1 || d > days_in_month(y, m)) return false;
  *t = days_since_epoch(y, m, d);
  return true;
}

// The date is a suffix after '|' or '-': YYYY-MM-DD/YYYY-MM-DD, YYYY-MM-DD, YYYY-MM, YYYY, tried in that order; the first form whose
// shape fits decides (a well-shaped suffix that is no date makes the id undated, as the exception does in the reference).
inline bool seq_id_date_range(const char* id, size_t n, double* t_min, double* t_max) {
  auto suffix = [&](size_t len) -> const char* { return n >= len + 1 && (id[n - len - 1] == '|' || id[n - len - 1] == '-') ? id + n - len : nullptr; };
  if (const char* s = suffix(21); s && is_date_str(s) && s[10] == '/' && is_date_str(s + 11)) return parse_date(s, t_min) && parse_date(s + 11, t_max);
  if (const char* s = suffix(10); s && is_date_str(s)) { if (!parse_date(s, t_min)) return false; *t_max = *t_min; return true; }
  if (const char* s = suffix(7); s && all_digits(s, 4) && s[4] == '-' && all_digits(s + 5, 2)) {
    const int y = digits_value(s, 4), m = digits_value(s + 5, 2);
    if (m < 1 || m > 12) return false;
    *t_min = days_since_epoch(y, m, 1); *t_max = m == 12 ? days_since_epoch(y + 1, 1, 1) : days_since_epoch(y, m + 1, 1);
    return true;
  }
  if (const char* s = suffix(4); s && all_digits(s, 4)) {
    const int y = digits_value(s, 4);
    *t_min = days_since_epoch(y, 1, 1); *t_max = days_since_epoch(y + 1, 1, 1);
    return true;
  }
  return false;
}

// ---- framing ----------------------------------------------------------------------------------------------------------------------
inline bool fasta_is_space(uint8_t c) { return c == ' ' || (c >= '\t' && c <= '\r'); }   // isspace in the "C" locale

// Records of a FASTA text, one call of next() each, as read_fasta frames them: lines end at '\n'; empty lines and lines that begin with ';' are
// skipped; a line that begins with '>' starts a record whose id is the rest of the line without the white space at its two ends; white
// space inside sequence lines (a '\r' before the '\n' included) is skipped; data before the first '>' belongs to a record named "".
struct FastaFramer {
  const uint8_t* p; const uint8_t* end;
  FastaFramer(const uint8_t* text, int64_t len) : p(text), end(text + (len > 0 ? len : 0)) {}

  // The next record: its id, and its characters without white space -- the first `cap` of them in `row` (may be null), all of them counted in *len.
  bool next(std::string* id, uint8_t* row, int64_t cap, int64_t* len) {
    bool have = false;
    *len = 0;
    while (p < end) {
      const uint8_t* nl = (const uint8_t*)memchr(p, '\n', (size_t)(end - p));
      const uint8_t* b = p; const uint8_t* e = nl ? nl : end;
      if (b == e || *b == ';') { p = nl ? nl + 1 : end; continue; }
      if (*b == '>') {
        if (have) break;   // (the next call's: the line is read again)
        ++b;
        while (b < e && fasta_is_space(*b)) ++b;
        while (b < e && fasta_is_space(e[-1])) --e;
        id->assign((const char*)b, (size_t)(e - b));
        have = true;
        p = nl ? nl + 1 : end;
        continue;
      }
      if (!have) { id->clear(); have = true; }
      int64_t n = *len;
      for (; b < e; ++b) if (!fasta_is_space(*b)) { if (row && n < cap) row[n] = *b; ++n; }
      *len = n;
      p = nl ? nl + 1 : end;
    }
    return have;
  }
};

// An upper bound of the records of a text: its lines that begin with '>', and one for data before the first.
inline int64_t fasta_count_headers(const uint8_t* text, int64_t len) {
  int64_t n = 1;
  const uint8_t* p = text; const uint8_t* end = text + (len > 0 ? len : 0);
  while (p < end) {
    if (*p == '>') ++n;
    const uint8_t* nl = (const uint8_t*)memchr(p, '\n', (size_t)(end - p));
    if (!nl) break;
    p = nl + 1;
  }
  return n;
}

}  // namespace emat

#endif  // EMAT_FASTA_PURE_HPP_
