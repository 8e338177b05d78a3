// Host check of csrc/leaf_chunks.hpp (compiled with g++ by tests/test_many_leaves_host.py): for every count the calls
// (first, cnt) are a partition of 0 .. count - 1 in ascending order, every cnt is between 1 and LEAF_CHUNK, and a count of at
// most LEAF_CHUNK is ONE call (0, count) -- the launch of a table that fits one chunk is the launch it always was.
#include <cstdio>
#include <utility>
#include <vector>

#include "leaf_chunks.hpp"

int main() {
    using leaf_chunks::LEAF_CHUNK;
    int failed = 0;
    if (LEAF_CHUNK != 32768 || LEAF_CHUNK > 65535) {
        std::printf("FAILED: LEAF_CHUNK = %zu\n", (size_t)LEAF_CHUNK);
        ++failed;
    }
    const size_t counts[] = {0, 1, 32767, 32768, 32769, 65535, 65536, 65537, 65600, 1000000};
    for (size_t count : counts) {
        std::vector<std::pair<size_t, size_t>> calls;
        leaf_chunks::for_leaf_chunks(count, [&](size_t first, size_t cnt) { calls.emplace_back(first, cnt); });
        size_t next = 0;
        bool ok = true;
        for (auto& c : calls) {
            ok = ok && c.first == next && c.second >= 1 && c.second <= LEAF_CHUNK;
            next = c.first + c.second;
        }
        ok = ok && next == count && calls.size() == (count + LEAF_CHUNK - 1) / LEAF_CHUNK;
        if (count >= 1 && count <= LEAF_CHUNK) ok = ok && calls.size() == 1 && calls[0].first == 0 && calls[0].second == count;
        // every call but the last is a whole chunk: the first leaf of run i is i * LEAF_CHUNK
        for (size_t i = 0; i + 1 < calls.size(); ++i) ok = ok && calls[i].second == LEAF_CHUNK;
        std::printf("count %zu: %zu calls, last cnt %zu%s\n", count, calls.size(), calls.empty() ? (size_t)0 : calls.back().second,
                    ok ? "" : "  FAILED");
        failed += ok ? 0 : 1;
    }
    if (failed) return 1;
    std::printf("all cases passed\n");
    return 0;
}
