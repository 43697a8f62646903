// rng_pos_host.cpp -- the chain's place in its random stream, kept as one cursor (delphy_amd/csrc/emat_rng_pos.hpp and the functions of
// emat_device_core.hpp that use it: rng_next64, rng_next64_computed, rng_fill, rng_wants_fill, rng_rewind_to_move_start, rng_enter_leg,
// rng_leave_leg) against a literal host copy of the state machine it replaces (counter, spare, flag), over random schedules of draws,
// fills, leg ends with re-entry, move starts and rewinds: the same word at every draw and the same header triple at every leg end.
//
// What a schedule may do is what the device can do: a fill anywhere BETWEEN two moves (by either machine's rule or for no reason), a
// rewind only to the start of the current move, a leg end anywhere.  Buffers of 32 blocks (the shipped size), 4, 1 and none; the fold of
// a runaway cursor is exercised with a small threshold (the device's is 2^30), and a move is never rewound across a fold, as on the device.
// The header's spare is compared whenever it is defined: always while has_spare is set, and otherwise unless the stream was rewound to
// an even position and has not drawn since (there the old machine leaves the spare of a block opened AFTER that position; nothing reads it).
//
// The stream itself is a stand-in for Philox (a 64-bit mixer per word): the arithmetic under test never looks at the words.
//
//   c++ -O2 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I delphy_amd/csrc
//       scripts/micro/rng_pos_host.cpp -o rng_pos_host && ./rng_pos_host [schedules, default 1000000]
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "emat_rng_pos.hpp"

static uint64_t mix(uint64_t z) { z += 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static void block_of(uint64_t ctr, uint64_t key, uint64_t out[2]) { out[0] = mix(mix(ctr) ^ key); out[1] = mix(out[0] ^ ctr); }

struct Header { uint64_t key, counter, spare; uint32_t has_spare; };

// ---- the old machine, word for word from the device headers before the cursor ------------------------------------------------------
struct Old {
  uint32_t blocks; std::vector<uint64_t> buf;
  uint64_t key, ctr, base, spare; bool has_spare;
  uint64_t mv_ctr; bool mv_had_spare;
  void enter(const Header& h) { key = h.key; ctr = h.counter; spare = h.spare; has_spare = h.has_spare != 0; base = ctr - (uint64_t)blocks; }
  uint64_t computed() { uint64_t w[2]; block_of(ctr++, key, w); spare = w[1]; has_spare = true; return w[0]; }
  uint64_t next64() {
    if (has_spare) { has_spare = false; return spare; }
    if (blocks != 0) {
      const uint64_t k = ctr - base;
      if (k < (uint64_t)blocks) { const uint64_t w0 = buf[2 * k], w1 = buf[2 * k + 1]; ctr += 1; spare = w1; has_spare = true; return w0; }
    }
    return computed();
  }
  void fill() { if (blocks == 0) return; const uint64_t b = ctr; for (uint32_t l = 0; l < blocks; ++l) block_of(b + l, key, &buf[2 * l]); base = b; }
  bool wants_fill(uint32_t margin) const { return blocks != 0 && ctr - base + (uint64_t)margin > (uint64_t)blocks; }
  void move_start() { mv_ctr = ctr; mv_had_spare = has_spare; }
  void rewind() { ctr = mv_ctr; has_spare = mv_had_spare; if (has_spare) { uint64_t w[2]; block_of(ctr - 1, key, w); spare = w[1]; } }
  void leave(Header& h) const { h.counter = ctr; h.spare = spare; h.has_spare = has_spare ? 1u : 0u; }
};

// ---- the new machine: emat_device_core.hpp's functions with the context's fields as members ------------------------------------------
struct New {
  uint32_t blocks, fold_at; std::vector<uint64_t> buf;
  uint64_t key, base, spare; uint32_t pos, mv_pos;
  uint64_t folds = 0;
  void enter(const Header& h) { const emat::RngPos at = emat::rng_pos_enter(h.counter, h.has_spare, blocks); key = h.key; base = at.base; pos = at.pos; mv_pos = at.pos; spare = h.spare; }
  uint64_t computed() {
    const emat::RngPos at = emat::rng_pos_folded(base, pos, blocks, fold_at);
    if (at.pos != pos) { base = at.base; ++folds; }
    pos = at.pos + 1u;
    if (at.pos & 1u) return spare;
    uint64_t w[2]; block_of(emat::rng_pos_block(at.base, at.pos), key, w);
    spare = w[1];
    return w[0];
  }
  uint64_t next64() {
    const uint32_t p = pos;
    if (emat::rng_pos_in_buffer(p, blocks)) { pos = p + 1u; return buf[p]; }
    return computed();
  }
  void fill() {
    if (blocks == 0) return;
    const uint32_t p = pos;
    const emat::RngPos to = emat::rng_pos_after_fill(base, p);
    if ((p & 1u) == 0 && emat::rng_pos_in_buffer(emat::rng_pos_spare_word(p), blocks)) spare = buf[emat::rng_pos_spare_word(p)];
    for (uint32_t l = 0; l < blocks; ++l) block_of(to.base + l, key, &buf[2 * l]);
    base = to.base; pos = to.pos;
  }
  bool wants_fill(uint32_t margin) const { return emat::rng_pos_wants_fill(pos, blocks, margin); }
  void move_start() { mv_pos = pos; }
  void rewind() {
    const uint32_t p = mv_pos;
    pos = p;
    if ((p & 1u) != 0 && !emat::rng_pos_in_buffer(p, blocks)) { uint64_t w[2]; block_of(emat::rng_pos_block(base, p), key, w); spare = w[1]; }
  }
  void leave(Header& h) const {
    const uint32_t sw = emat::rng_pos_spare_word(pos);
    h.counter = emat::rng_pos_counter(base, pos); h.has_spare = emat::rng_pos_has_spare(pos);
    h.spare = emat::rng_pos_in_buffer(sw, blocks) ? buf[sw] : spare;
  }
};

static uint64_t s_state = 0x2545F4914F6CDD1Dull;
static uint64_t rnd() { return s_state = mix(s_state); }
static uint32_t below(uint32_t n) { return (uint32_t)((rnd() >> 32) * (uint64_t)n >> 32); }

int main(int argc, char** argv) {
  const long schedules = argc > 1 ? atol(argv[1]) : 1000000;
  const uint32_t margin = 8;
  uint64_t draws = 0, beyond = 0, legs = 0, legs_odd = 0, fills = 0, rewinds = 0, rewinds_odd_beyond = 0, folds = 0, spare_skipped = 0, ended_on_last_word = 0;
  for (long it = 0; it < schedules; ++it) {
    static const uint32_t sizes[4] = {32, 32, 4, 0};
    const uint32_t blocks = it % 7 == 3 ? 1u : sizes[it & 3];
    Old o; New n;
    o.blocks = n.blocks = blocks; o.buf.assign(2 * (size_t)blocks, 0); n.buf.assign(2 * (size_t)blocks, 0);
    n.fold_at = 2 * blocks + 4 + below(60);
    Header ho, hn;
    ho.key = rnd(); ho.counter = below(4) == 0 ? 0 : (below(2) ? rnd() >> (2 + below(58)) : below(1000)); ho.has_spare = ho.counter != 0 && below(2); ho.spare = 0;
    if (ho.has_spare) { uint64_t w[2]; block_of(ho.counter - 1, ho.key, w); ho.spare = w[1]; } else ho.spare = rnd();
    hn = ho;
    o.enter(ho); n.enter(hn);
    o.move_start(); n.move_start();
    bool stale = false; uint64_t folds_at_move = n.folds;
    const int ops = 10 + (int)below(60);
    for (int k = 0; k < ops; ++k) {
      const uint32_t what = below(100);
      if (what < 60) {   // a move's draws: mostly a few, sometimes past the margin and the buffer
        const uint32_t cnt = below(10) == 0 ? below(3 * (2 * blocks + 8)) : 1 + below(6);
        for (uint32_t d = 0; d < cnt; ++d) {
          if (!emat::rng_pos_in_buffer(n.pos, blocks)) ++beyond;
          const uint64_t a = o.next64(), b = n.next64();
          ++draws; stale = false;
          if (a != b) { printf("schedule %ld op %d draw %u: old %016" PRIx64 " new %016" PRIx64 "\n", it, k, d, a, b); return 1; }
          if (n.pos == 2 * blocks && blocks != 0) ++ended_on_last_word;
        }
      } else if (what < 75) {   // between two moves: the rule asks, then the next move starts
        if (o.wants_fill(margin)) o.fill();
        if (n.wants_fill(margin)) { n.fill(); ++fills; }
        o.move_start(); n.move_start(); folds_at_move = n.folds;
      } else if (what < 80) {   // a fill for no reason, in one machine, the other or both (between two moves)
        const uint32_t who = 1 + below(3);
        if (who & 1) o.fill();
        if (who & 2) { n.fill(); ++fills; }
        o.move_start(); n.move_start(); folds_at_move = n.folds;
      } else if (what < 88) {   // the move stops and the stream goes back to its first draw
        if (n.folds == folds_at_move) {   // (every fill above is followed by a move start)
          if ((n.mv_pos & 1u) && !emat::rng_pos_in_buffer(n.mv_pos, blocks)) ++rewinds_odd_beyond;
          o.rewind(); n.rewind(); ++rewinds;
          if (!(n.pos & 1u)) stale = true;
        }
      } else {   // the leg ends; the next one begins from the header
        o.leave(ho); n.leave(hn); ++legs; legs_odd += hn.has_spare;
        const bool spare_defined = hn.has_spare != 0 || !stale;
        if (!spare_defined) ++spare_skipped;
        if (ho.counter != hn.counter || ho.has_spare != hn.has_spare || (spare_defined && ho.spare != hn.spare)) {
          printf("schedule %ld op %d leg end: old (%" PRIu64 ", %016" PRIx64 ", %u) new (%" PRIu64 ", %016" PRIx64 ", %u)\n", it, k, ho.counter, ho.spare, ho.has_spare, hn.counter, hn.spare, hn.has_spare);
          return 1;
        }
        o.enter(ho); n.enter(hn);
        o.move_start(); n.move_start(); folds_at_move = n.folds;
      }
    }
    folds += n.folds;
  }
  printf("%ld schedules: %" PRIu64 " draws (%" PRIu64 " beyond the buffer, %" PRIu64 " took its last word), %" PRIu64 " fills, %" PRIu64 " leg ends (%" PRIu64
         " with a spare, %" PRIu64 " with the spare undefined), %" PRIu64 " rewinds (%" PRIu64 " to a half-used block beyond the buffer), %" PRIu64 " folds: all equal\n",
         schedules, draws, beyond, ended_on_last_word, fills, legs, legs_odd, spare_skipped, rewinds, rewinds_odd_beyond, folds);
  return (beyond && fills && legs_odd && rewinds_odd_beyond && folds && ended_on_last_word) ? 0 : 2;
}
