// The blocks of dsmgp_kfold: which positions of every factor owner each fold label holds out.  Plain C++17, neither HIP nor
// dsmgp_hip.h (the pattern of ctx_state.hpp and route_walk.hpp), so that a host test compiles it with g++
// (tests/kfold_plan_check.cpp).
//
// For owner o with positions 0 .. n_o - 1 and label k, block (o, k) = { i : fold[obs_idx[obs_off_o + i]] == k }, the positions in
// ascending order (a stable counting sort by label).  Rows with label -1 belong to no block.  Empty blocks are not stored.  The
// blocks are stored label by label (round k of the packing), owners ascending inside a label; their positions lie owner by owner.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kfold_plan {

constexpr int TILE = 128;

struct Owner {
    int32_t id;             // the caller's name of the owner (a leaf index)
    int32_t n;              // its rows
    int64_t obs_off;        // its first entry in obs_idx
};

struct Block {
    int32_t owner;          // index into the owners handed to build()
    int32_t label;
    int32_t m;              // rows held out
    int32_t mpad;           // m rounded up to 128
    int64_t pos_off;        // first entry of the block in Plan::pos (m entries, ascending)
    int64_t tile_off;       // first entry in Plan::tile_first (mpad / 128 entries)
};

struct Plan {
    std::vector<Block> blocks;              // label-major, owners ascending inside a label
    std::vector<int32_t> pos;               // positions inside the owner
    std::vector<int32_t> tile_first;        // per 128-row tile of a block: the position of its first row
    std::vector<int64_t> label_first;       // K + 1: blocks [label_first[k], label_first[k + 1]) have label k
    std::vector<int64_t> owner_first;       // owners + 1: by_owner[owner_first[o] .. owner_first[o + 1]) are owner o's blocks
    std::vector<int32_t> by_owner;          // block indices, labels ascending inside an owner

    // the block of (owner, label), or -1 when it is empty
    int32_t find(size_t owner, int32_t label) const {
        int64_t lo = owner_first[owner], hi = owner_first[owner + 1];
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (blocks[(size_t)by_owner[(size_t)mid]].label < label) lo = mid + 1;
            else hi = mid;
        }
        return (lo < owner_first[owner + 1] && blocks[(size_t)by_owner[(size_t)lo]].label == label) ? by_owner[(size_t)lo] : -1;
    }
};

// 0 on success; -1 when a label of a held row lies outside -1 .. K - 1 (the plan is then unspecified): the header's own guard --
// it indexes by label -- for a caller that has not validated the labels.  Labels of rows that no owner holds are not looked at.
// Host memory: one counter per label and what the blocks themselves take (at most one block per held row), whatever owners x K is.
inline int build(const std::vector<Owner>& owners, const int64_t* obs_idx, const int32_t* fold, int32_t K, Plan& out) {
    out = Plan{};
    const size_t no = owners.size();
    out.label_first.assign((size_t)K + 1, 0);
    out.owner_first.assign(no + 1, 0);
    std::vector<int32_t> cnt((size_t)K, 0), slot((size_t)K, -1), touched;
    std::vector<Block> made;                // owner-major, labels ascending inside an owner
    int64_t ptot = 0, ttot = 0;
    for (size_t o = 0; o < no; ++o) {
        touched.clear();
        for (int32_t i = 0; i < owners[o].n; ++i) {
            const int32_t k = fold[obs_idx[owners[o].obs_off + i]];
            if (k < -1 || k >= K) return -1;
            if (k >= 0 && cnt[(size_t)k]++ == 0) touched.push_back(k);
        }
        std::sort(touched.begin(), touched.end());
        for (const int32_t k : touched) {
            Block b{};
            b.owner = (int32_t)o;
            b.label = k;
            b.m = cnt[(size_t)k];
            b.mpad = (b.m + TILE - 1) / TILE * TILE;
            b.pos_off = ptot;
            b.tile_off = ttot;
            ptot += b.m;
            ttot += b.mpad / TILE;
            slot[(size_t)k] = (int32_t)made.size();
            made.push_back(b);
            cnt[(size_t)k] = 0;             // from here on: the next free slot of the block
        }
        out.pos.resize((size_t)ptot);
        out.tile_first.resize((size_t)ttot);
        // the stable pass: positions ascending, each to the next free slot of its block
        for (int32_t i = 0; i < owners[o].n; ++i) {
            const int32_t k = fold[obs_idx[owners[o].obs_off + i]];
            if (k < 0) continue;
            const Block& b = made[(size_t)slot[(size_t)k]];
            const int32_t at = cnt[(size_t)k]++;
            out.pos[(size_t)b.pos_off + (size_t)at] = i;
            if (at % TILE == 0) out.tile_first[(size_t)b.tile_off + (size_t)(at / TILE)] = i;
        }
        for (const int32_t k : touched) cnt[(size_t)k] = 0;
        out.owner_first[o + 1] = (int64_t)made.size();
    }
    // label-major order: a counting sort by label, owners stay ascending inside a label
    for (const Block& b : made) ++out.label_first[(size_t)b.label + 1];
    for (int32_t k = 0; k < K; ++k) out.label_first[(size_t)k + 1] += out.label_first[(size_t)k];
    std::vector<int64_t> next(out.label_first.begin(), out.label_first.end() - 1);
    out.blocks.resize(made.size());
    out.by_owner.resize(made.size());
    for (size_t i = 0; i < made.size(); ++i) {
        const int64_t at = next[(size_t)made[i].label]++;
        out.blocks[(size_t)at] = made[i];
        out.by_owner[i] = (int32_t)at;      // `made` is owner-major with labels ascending: so is by_owner
    }
    return 0;
}

}  // namespace kfold_plan
