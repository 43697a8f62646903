// emat_run_exchange.hpp -- exchange format of part subtrees between the processes of a sharded run: per part the header
// {int32 id, nodes, muts, intervals, from_states, root, 0, 0}, followed by the arrays of the FlatTree in the order of FlatTree::for_each_array
// (the order of `emat_flat_tree`), every array padded to 8 bytes.  Size, writer and reader are all written from that one enumeration.
//
// Included by emat_run.cpp after emat_run_tree.hpp; uses flat_tree.hpp alone.
#ifndef EMAT_RUN_EXCHANGE_HPP_
#define EMAT_RUN_EXCHANGE_HPP_

#include <cstdint>
#include <cstring>

#include "flat_tree.hpp"

namespace emat {

constexpr uint64_t kPartHeaderBytes = 8 * sizeof(int32_t);
inline uint64_t pad8(uint64_t x) { return (x + 7u) & ~(uint64_t)7u; }

inline uint64_t packed_bytes(const FlatTree& t) {
  uint64_t bytes = kPartHeaderBytes;
  FlatTree::for_each_array(t, [&](const auto& vec, auto, FlatTree::Count) { bytes += pad8(vec.size() * sizeof(vec[0])); });
  return bytes;
}
inline void pack_part(uint8_t*& w, int32_t id, const FlatTree& t) {   // packed_bytes(t) bytes at w, which moves past them
  const int32_t hdr[8] = {id, t.num_nodes(), t.num_muts(), t.num_intervals(), t.num_from_states(), t.root, 0, 0};
  std::memcpy(w, hdr, kPartHeaderBytes); w += kPartHeaderBytes;
  FlatTree::for_each_array(t, [&](const auto& vec, auto, FlatTree::Count) { std::memcpy(w, vec.data(), vec.size() * sizeof(vec[0])); w += pad8(vec.size() * sizeof(vec[0])); });
}
// The arrays of a part whose header gave `shape`, from [r, end); r moves past them.  false: the buffer ends before the part does.
inline bool unpack_arrays(const uint8_t*& r, const uint8_t* end, const FlatTree::Shape& shape, FlatTree& t) {
  bool ok = true;
  FlatTree::for_each_array(t, [&](auto& vec, auto, FlatTree::Count c) {
    const uint64_t bytes = shape.of(c) * sizeof(vec[0]);
    if (!ok || (uint64_t)(end - r) < pad8(bytes)) { ok = false; return; }
    vec.resize(shape.of(c)); std::memcpy(vec.data(), r, bytes); r += pad8(bytes);
  });
  return ok;
}

}  // namespace emat
#endif  // EMAT_RUN_EXCHANGE_HPP_
