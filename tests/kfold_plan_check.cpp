// csrc/kfold_plan.hpp on the host (tests/test_kfold_host.py compiles this with g++): the blocks of dsmgp_kfold for two owners that
// share rows.  Owner 0 has 546 rows with blocks of exactly 1, 127, 128 and 129 rows, an empty label, rows with label -1, and a
// block whose first row lies in the third row tile (position 300); owner 1 holds every second row of it, in reverse row order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kfold_plan.hpp"

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main() {
    using namespace kfold_plan;
    const int32_t K = 7;                     // label 4: empty; label 6: outside owner 0's rows only
    const int N = 600;
    std::vector<int32_t> fold((size_t)N, -1);
    // rows 0 .. 545 are owner 0's, in order.  label 0: 1 row; 1: 127; 2: 128; 3: 129; 5: 150 rows from position 300 on; rest -1
    int at = 0;
    fold[(size_t)at++] = 0;
    for (int i = 0; i < 127; ++i) fold[(size_t)at++] = 1;
    for (int i = 0; i < 128; ++i) fold[(size_t)at++] = (i % 2) ? 2 : 3;     // interleaved: 64 of each
    for (int i = 0; i < 64; ++i) fold[(size_t)at++] = 2;
    for (int i = 0; i < 65; ++i) fold[(size_t)at++] = 3;
    CHECK(at == 385);
    // label 5 must start in the third row tile: nothing of it before position 300
    for (int i = 300; i < 450; ++i) fold[(size_t)i] = 5;                    // overwrites 85 rows of labels 2 / 3 above
    for (int i = 546; i < N; ++i) fold[(size_t)i] = 6;
    std::vector<int64_t> obs_idx;
    for (int i = 0; i < 546; ++i) obs_idx.push_back(i);
    for (int i = 544; i >= 0; i -= 2) obs_idx.push_back(i);                 // owner 1: 273 rows, descending row numbers
    std::vector<Owner> owners = {{10, 546, 0}, {11, 273, 546}};
    Plan p;
    CHECK(build(owners, obs_idx.data(), fold.data(), K, p) == 0);
    // sizes by a direct count
    for (size_t o = 0; o < owners.size(); ++o)
        for (int32_t k = 0; k < K; ++k) {
            int m = 0;
            for (int i = 0; i < owners[o].n; ++i) m += fold[(size_t)obs_idx[(size_t)owners[o].obs_off + i]] == k;
            const int32_t b = p.find(o, k);
            if (m == 0) {
                CHECK(b < 0);
                continue;
            }
            CHECK(b >= 0);
            const Block& B = p.blocks[(size_t)b];
            CHECK(B.owner == (int32_t)o && B.label == k && B.m == m && B.mpad == (m + 127) / 128 * 128 && B.mpad >= m);
            CHECK(b >= p.label_first[(size_t)k] && b < p.label_first[(size_t)k + 1]);
            int32_t prev = -1;
            for (int i = 0; i < B.m; ++i) {       // ascending positions, each of the label
                const int32_t pos = p.pos[(size_t)B.pos_off + i];
                CHECK(pos > prev && pos < owners[o].n);
                CHECK(fold[(size_t)obs_idx[(size_t)owners[o].obs_off + pos]] == k);
                if (i % 128 == 0) CHECK(p.tile_first[(size_t)B.tile_off + i / 128] == pos);
                prev = pos;
            }
        }
    // the named shapes of owner 0
    CHECK(p.blocks[(size_t)p.find(0, 0)].m == 1 && p.blocks[(size_t)p.find(0, 0)].mpad == 128);
    CHECK(p.blocks[(size_t)p.find(0, 1)].m == 127);
    const Block& b5 = p.blocks[(size_t)p.find(0, 5)];
    CHECK(b5.m == 150 && b5.mpad == 256 && p.tile_first[(size_t)b5.tile_off] == 300 && p.tile_first[(size_t)b5.tile_off] / 128 == 2);
    CHECK(p.tile_first[(size_t)b5.tile_off + 1] == 428);
    CHECK(p.find(0, 4) < 0 && p.find(1, 4) < 0 && p.find(0, 6) < 0);      // an empty label; label 6 lies outside the owners
    CHECK(p.label_first[4] == p.label_first[5] && p.label_first[(size_t)K] == (int64_t)p.blocks.size());
    // blocks of exactly 128 and 129 rows: relabel so that owner 0 has them
    {
        std::vector<int32_t> f2((size_t)N, -1);
        for (int i = 0; i < 128; ++i) f2[(size_t)(2 * i)] = 0;
        for (int i = 0; i < 129; ++i) f2[(size_t)(2 * i + 1)] = 1;
        Plan q;
        CHECK(build(owners, obs_idx.data(), f2.data(), 2, q) == 0);
        const Block& a = q.blocks[(size_t)q.find(0, 0)];
        const Block& c = q.blocks[(size_t)q.find(0, 1)];
        CHECK(a.m == 128 && a.mpad == 128 && c.m == 129 && c.mpad == 256);
        CHECK(q.tile_first[(size_t)c.tile_off + 1] == 257);
        // owner 1 holds the even rows only: label 1 is empty there, and its positions ascend although its rows descend
        CHECK(q.find(1, 1) < 0);
        const Block& d = q.blocks[(size_t)q.find(1, 0)];
        CHECK(d.m == 128 && q.pos[(size_t)d.pos_off] == 272 - 127 && q.pos[(size_t)d.pos_off + 127] == 272);
    }
    // a label outside -1 .. K - 1 on a held row is refused; on a row nobody holds it is not looked at
    {
        std::vector<int32_t> f3 = fold;
        f3[599] = 99;
        Plan q;
        CHECK(build(owners, obs_idx.data(), f3.data(), K, q) == 0);
        f3[3] = K;
        CHECK(build(owners, obs_idx.data(), f3.data(), K, q) == -1);
        f3[3] = -2;
        CHECK(build(owners, obs_idx.data(), f3.data(), K, q) == -1);
    }
    std::printf("all cases passed\n");
    return 0;
}
