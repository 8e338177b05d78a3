// One grid row per leaf: every launch whose grid's second dimension is a number of leaves goes through for_leaf_chunks, which
// cuts the table into runs of at most LEAF_CHUNK leaves.  A grid's second and third dimensions are 16-bit quantities on some
// runtimes (65,535) and 65,536 on others; LEAF_CHUNK is below both, and the kernels take the first leaf of their run as an
// argument (leaf0 + blockIdx.y).  Plain C++17, neither HIP nor dsmgp_hip.h (the pattern of kfold_plan.hpp), so that a host
// test compiles it with g++ (tests/leaf_chunks_check.cpp).
#pragma once
#include <algorithm>
#include <cstddef>

namespace leaf_chunks {

constexpr size_t LEAF_CHUNK = 32768;

// f(first, cnt) for first = 0, LEAF_CHUNK, 2 LEAF_CHUNK, ... below `count`, cnt = min(LEAF_CHUNK, count - first): a partition of
// 0 .. count - 1 in ascending order.  count <= LEAF_CHUNK is one call f(0, count); count = 0 is none.
template <class F>
inline void for_leaf_chunks(size_t count, F&& f) {
    for (size_t first = 0; first < count; first += LEAF_CHUNK) f(first, std::min(LEAF_CHUNK, count - first));
}

}  // namespace leaf_chunks
