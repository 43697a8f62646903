// fasta_host.cpp -- the FASTA framer and the date parser (delphy_amd/csrc/emat_fasta_pure.hpp) compiled for the host alone, to be run
// under the address and undefined-behaviour sanitizers: every framing case of tests/test_alignment_model.py with the records it must
// give, each text also cut short at every length (a reader must never look past the end it was given), and the date parser over ids of
// every form and over every prefix and suffix of them.  The run fails (exit status 1) when a record differs; the sanitizers abort it.
//
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I delphy_amd/csrc
//       scripts/micro/fasta_host.cpp -o fasta_host && ./fasta_host
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "emat_fasta_pure.hpp"

using Records = std::vector<std::pair<std::string, std::string>>;

// The text in a heap block of exactly its size (so that one byte past it is poisoned), framed with rows of `cap` characters.
static Records frame(const std::string& text, int64_t cap) {
  uint8_t* copy = (uint8_t*)malloc(text.size() ? text.size() : 1);
  memcpy(copy, text.data(), text.size());
  emat::FastaFramer f(copy, (int64_t)text.size());
  Records out;
  std::string id; int64_t len = 0;
  std::vector<uint8_t> row((size_t)cap);
  while (f.next(&id, row.data(), cap, &len)) out.push_back({id, std::string((const char*)row.data(), (size_t)(len < cap ? len : cap)) + (len > cap ? "+" + std::to_string(len - cap) : "")});
  if ((int64_t)out.size() > emat::fasta_count_headers(copy, (int64_t)text.size())) { printf("FAIL: more records than fasta_count_headers promised\n"); exit(1); }
  free(copy);
  return out;
}

int main() {
  struct Case { const char* name; std::string text; Records want; };
  const std::vector<Case> cases = {
    {"plain", ">a|2024-01-05\nACGT\nACGT\n>b\nAAAA\nCCCC\n", {{"a|2024-01-05", "ACGTACGT"}, {"b", "AAAACCCC"}}},
    {"crlf", ">a|2024-01-05\r\nACGT\r\nACGT\r\n>b\r\nAAAACCCC\r\n", {{"a|2024-01-05", "ACGTACGT"}, {"b", "AAAACCCC"}}},
    {"no final newline", ">a\nACGTACGT\n>b|2021\nAAAACCCC", {{"a", "ACGTACGT"}, {"b|2021", "AAAACCCC"}}},
    {"blank and comment lines", ";a comment\n\n>a|2024-01\n\nACGT\n;ACGT is not read\nACGT\n\n\n>b\nAAAACCCC\n\n", {{"a|2024-01", "ACGTACGT"}, {"b", "AAAACCCC"}}},
    {"ids with spaces", ">  hCoV-19/some place/1 2 | x|2022-10-01  \t\nACGTACGT\n>\tb c\nACGTACGT\n", {{"hCoV-19/some place/1 2 | x|2022-10-01", "ACGTACGT"}, {"b c", "ACGTACGT"}}},
    {"white space inside lines", ">a\nAC GT\tAC\x0bG\x0cT\n>b\n A C G T A C G T \n", {{"a", "ACGTACGT"}, {"b", "ACGTACGT"}}},
    {"record before the first header", "ACGT\nACGT\n>b|2020-02-02\nAAAACCCC\n", {{"", "ACGTACGT"}, {"b|2020-02-02", "AAAACCCC"}}},
    {"empty ids", ">\nACGTACGT\n>   \nACGTACGT\n", {{"", "ACGTACGT"}, {"", "ACGTACGT"}}},
    {"a lone carriage return", "\r\nACGTACGT\n>b\nAAAACCCC\n", {{"", "ACGTACGT"}, {"b", "AAAACCCC"}}},
    {"unequal lengths", ">a\nACGTACGTAC\n>b\n>c\nACG\n", {{"a", "ACGTACGT+2"}, {"b", ""}, {"c", "ACG"}}},
    {"empty", "", {}},
    {"nothing but blank lines and comments", "\n\n;x\n", {}},
  };
  int bad = 0;
  for (const Case& c : cases) {
    const Records got = frame(c.text, 8);
    if (got != c.want) { printf("FAIL %s: %zu records\n", c.name, got.size()); for (auto& r : got) printf("  '%s' '%s'\n", r.first.c_str(), r.second.c_str()); ++bad; }
    for (size_t n = 0; n <= c.text.size(); ++n) { (void)frame(c.text.substr(0, n), 8); (void)frame(c.text.substr(n), 3); }
  }
  const std::vector<std::string> ids = {"hCoV-19/England/PLYM-3258B175/2022|EPI_ISL_15330011|2022-10-01", "hRSV-A-England-160340212-2016-EPI_ISL_11428309-2016-01-19",
                                        "Seq123|2024-07-14/2024-09-22", "Seq123|2024-12", "Seq123|2024", "a|2023-02-29", "a|2024-13-01", "a|2024-00", "a|9999-12-31", "a|0000", "|", ""};
  long dated = 0;
  for (const std::string& s : ids)
    for (size_t a = 0; a <= s.size(); ++a)
      for (size_t n = 0; a + n <= s.size(); ++n) {
        const std::string t = s.substr(a, n);
        char* copy = (char*)malloc(t.size() ? t.size() : 1);   // (no terminator: the parser is given a length)
        memcpy(copy, t.data(), t.size());
        double lo = 0.0, hi = 0.0;
        dated += emat::seq_id_date_range(copy, t.size(), &lo, &hi);
        free(copy);
      }
  double lo = 0.0, hi = 0.0;
  if (!emat::seq_id_date_range("x|2020-03-01", 12, &lo, &hi) || lo != 60.0 || hi != 60.0) { printf("FAIL: 2020-03-01 is day 60\n"); ++bad; }
  if (!emat::seq_id_date_range("x|1900-02", 9, &lo, &hi) || hi - lo != 28.0) { printf("FAIL: February 1900 has 28 days\n"); ++bad; }
  if (!emat::seq_id_date_range("x-2000", 6, &lo, &hi) || hi - lo != 366.0) { printf("FAIL: 2000 has 366 days\n"); ++bad; }
  printf("%zu framing cases, every cut of each; %zu ids, every substring of each (%ld dated): %s\n", cases.size(), ids.size(), dated, bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
