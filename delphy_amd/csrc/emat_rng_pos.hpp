// emat_rng_pos.hpp -- where a part's random stream stands, as arithmetic on integers and nothing else.
//
// The stream is Philox4x32-10 blocks of consecutive counters; a block is two 64-bit words, word 0 = x | y << 32, word 1 = z | w << 32,
// and a draw takes the next word.  The slab header names a position as (rng_counter, rng_has_spare): `rng_counter` blocks have been
// opened, and with `rng_has_spare` the second word of the last one is still to come -- word 2 * rng_counter - rng_has_spare of the
// stream is next.  The chain names the same position as (base, pos): `base` is the counter of the block at words 0 and 1 of the buffer
// the wave computes ahead (emat_lds_rng, `blocks` blocks), `pos` the next word counted from there -- word 2 * base + pos of the stream.
// Words at pos < 2 * blocks lie in the buffer; from there on a draw computes its own block (rng_next64_computed).
//
// Plain C++, compiled for the device (emat_device_core.hpp, emat_part_kernels.hpp) and for the host (scripts/micro/rng_pos_host.cpp, which
// runs this cursor beside the (counter, spare, flag) state machine it replaces).
#ifndef EMAT_RNG_POS_HPP_
#define EMAT_RNG_POS_HPP_

#include <cstdint>

#ifndef EMAT_HD
#if defined(__HIPCC__)
#define EMAT_HD __host__ __device__ __forceinline__
#else
#define EMAT_HD inline
#endif
#endif

namespace emat {

struct RngPos { uint64_t base; uint32_t pos; };

// Header -> cursor, where a leg begins: nothing counts as computed ahead, and pos is at least 2 * blocks + 2, which no position reached
// from inside the buffer without a draw of its own block can be mistaken for (rng_pos_spare_word: 2 * blocks itself is "the buffer's last
// word has just been drawn").  (base may wrap below zero for a stream that has drawn nothing: rng_pos_block wraps back.)
EMAT_HD RngPos rng_pos_enter(uint64_t counter, uint32_t has_spare, uint32_t blocks) {
  const uint64_t word = 2 * counter - (has_spare != 0 ? 1u : 0u);
  RngPos r; r.base = (word >> 1) - (uint64_t)blocks - 1u; r.pos = 2u * blocks + 2u + (uint32_t)(word & 1u);
  return r;
}
// Cursor -> header, where a leg ends.
EMAT_HD uint64_t rng_pos_counter(uint64_t base, uint32_t pos) { return base + (uint64_t)((pos + 1u) >> 1); }   // blocks opened
EMAT_HD uint32_t rng_pos_has_spare(uint32_t pos) { return pos & 1u; }
// The header's rng_spare is the second word of the last block opened: word `pos` if that is still to come (pos odd), else word pos - 1.
// Below 2 * blocks it is the buffer's; otherwise the context's rng_spare holds it -- also at pos == 0 (wraps), where rng_fill kept it.
EMAT_HD uint32_t rng_pos_spare_word(uint32_t pos) { return (pos - 1u) | 1u; }

EMAT_HD bool rng_pos_in_buffer(uint32_t pos, uint32_t blocks) { return pos < 2u * blocks; }
EMAT_HD uint64_t rng_pos_block(uint64_t base, uint32_t pos) { return base + (uint64_t)(pos >> 1); }              // counter of the block that holds word `pos`

// THE rule for when the wave computes ahead again, asked between two moves: the blocks started so far, plus the `margin` a move may use
// before it has to compute its own, no longer fit the buffer.
EMAT_HD bool rng_pos_wants_fill(uint32_t pos, uint32_t blocks, uint32_t margin) { return blocks != 0 && ((pos + 1u) >> 1) + margin > blocks; }
// A fill computes the `blocks` blocks from the one that holds the next word: that word is then word 0 or 1 of the buffer.
EMAT_HD RngPos rng_pos_after_fill(uint64_t base, uint32_t pos) { RngPos r; r.base = rng_pos_block(base, pos); r.pos = pos & 1u; return r; }
// Beyond the buffer, whole blocks move from pos into base once pos has reached `fold_at` (a hook that draws millions of numbers on a
// context nobody fills): the same word of the stream, the same parity, pos back at the value a leg begins with.
EMAT_HD RngPos rng_pos_folded(uint64_t base, uint32_t pos, uint32_t blocks, uint32_t fold_at) {
  RngPos r; r.base = base; r.pos = pos;
  if (pos >= fold_at && pos >= 2u * blocks + 4u) { const uint32_t over = (pos - (2u * blocks + 2u)) >> 1; r.base = base + (uint64_t)over; r.pos = pos - 2u * over; }
  return r;
}

}  // namespace emat
#endif  // EMAT_RNG_POS_HPP_
