// The owners of csrc/dev_owner.hpp on a counting host allocator: every block is in a set of live blocks from its allocation to
// its free, a free of a block that is not live aborts, and the blocks still live at exit fail the run.  The allocator keeps a
// log of its calls and can be told to fail the n-th allocation.
// (tests/test_call_sequences_host.py compiles this with the host compiler and runs it; it prints one line per case.)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "dev_owner.hpp"

struct Counting {
    static std::set<void*> live;
    static std::vector<std::pair<char, size_t>> log;      // ('a', bytes) | ('f', 0)
    static int allocs, frees, fail_at;                      // fail_at: the allocation (counted from 1, from now on) that fails; 0 = none
    static int alloc(void** p, size_t bytes) {
        if (fail_at > 0 && --fail_at == 0) return 2;        // (an error code of the allocator's own: passed through)
        *p = std::malloc(bytes);
        if (!*p) std::abort();
        live.insert(*p);
        log.push_back({'a', bytes});
        ++allocs;
        return 0;
    }
    static void free(void* p) {
        if (!live.erase(p)) {
            std::fprintf(stderr, "free of a block that is not live: %p\n", p);
            std::abort();
        }
        std::free(p);
        log.push_back({'f', 0});
        ++frees;
    }
    static void reset() {
        log.clear();
        allocs = frees = fail_at = 0;
    }
};
std::set<void*> Counting::live;
std::vector<std::pair<char, size_t>> Counting::log;
int Counting::allocs = 0, Counting::frees = 0, Counting::fail_at = 0;

using Pool = dev_owner::Pool<Counting>;
using Arena = dev_owner::Arena<Counting>;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

static void begin(const char* name) {
    CHECK(Counting::live.empty());
    Counting::reset();
    std::printf("case: %s\n", name);
}
static size_t live() { return Counting::live.size(); }

struct Ctx { Arena F, Dinv; };      // what of dsmgp_ctx the adoption sequence of grow_rows touches

// grow_rows: the arena is moved out of the context; `build` adopts it into the second context unless it returns early
static bool adopt(Ctx& c, Arena&& a, bool fail_before_the_move) {
    if (fail_before_the_move) return false;
    c.F = std::move(a);
    return true;
}

int main() {
    begin("moving out of a holder and destroying both: one free, nothing live");
    {
        Arena a;
        CHECK(a.get(nullptr, 100) == 0 && a.own && a.cap == 100 && live() == 1);
        {
            Arena b = std::move(a);
            CHECK(!a.p && a.cap == 0 && !a.own && b.p && b.cap == 100 && b.own);
            Arena d;
            d = std::move(b);
            CHECK(!b.p && b.cap == 0 && d.p && d.cap == 100 && live() == 1 && Counting::frees == 0);
        }
        CHECK(live() == 0 && Counting::frees == 1);
    }
    CHECK(Counting::allocs == 1 && Counting::frees == 1);

    begin("adoption: an early return after the move leaves exactly that block live in the second context");
    {
        Ctx second;
        void* block = nullptr;
        {
            Ctx first;
            CHECK(first.F.get(nullptr, 64) == 0);
            block = first.F.p;
            Arena old = std::move(first.F);       // moved out of the context
            CHECK(!first.F.p && live() == 1);
            CHECK(adopt(second, std::move(old), false));
            // the early return: `old` and `first` go
        }
        CHECK(live() == 1 && Counting::live.count(block) == 1 && second.F.p == block && second.F.own && Counting::frees == 0);
    }
    CHECK(live() == 0 && Counting::frees == 1);

    begin("adoption: an early return before the move frees the block once");
    {
        Ctx second;
        {
            Ctx first;
            CHECK(first.F.get(nullptr, 64) == 0);
            Arena old = std::move(first.F);
            CHECK(!adopt(second, std::move(old), true));
            CHECK(old.p && live() == 1 && Counting::frees == 0);       // still the caller's
        }
        CHECK(live() == 0 && Counting::frees == 1 && !second.F.p);
    }
    CHECK(Counting::frees == 1);

    begin("pool carving: offsets, the zero-count request, put without a free, the plan mark, one free of the block");
    {
        Pool pool;
        CHECK(!pool.active() && pool.reserve(1 << 16) == 0 && pool.active() && Counting::allocs == 1);
        Arena a, b, z, t;
        CHECK(a.get(&pool, 3) == 0 && !a.own && a.cap == 3);
        CHECK((char*)a.p - pool.base == 0 && pool.top == 24);
        CHECK(b.get(&pool, 33) == 0 && (char*)b.p - pool.base == 256 && pool.top == 256 + 33 * 8);
        CHECK(z.get(&pool, 0) == 0 && z.p && z.cap == 0 && (char*)z.p - pool.base == 768 && pool.top == 768 + 8);
        pool.mark();
        const size_t mark = pool.mark_plan;
        CHECK(mark == 776);
        CHECK(t.get(&pool, 1000) == 0 && (char*)t.p - pool.base == 1024 && ((char*)t.p - pool.base) % 256 == 0);
        t.put();
        CHECK(!t.p && t.cap == 0 && Counting::frees == 0);
        pool.reset_to_mark();
        CHECK(pool.top == mark);
        CHECK(t.get(&pool, 5) == 0 && (char*)t.p - pool.base == (ptrdiff_t)((mark + 255) & ~size_t(255)));
        // a request that does not fit: the status, what it needed, and an empty arena; the pool's top stays
        const size_t top = pool.top;
        Arena big;
        CHECK(big.get(&pool, 1 << 16) == dev_owner::POOL_FULL && !big.p && big.cap == 0 && pool.top == top);
        CHECK(pool.need == ((top + 255) & ~size_t(255)) + (size_t(1) << 16) * 8);
        pool.reset();
        CHECK(pool.top == 0 && pool.mark_plan == 0);
        a.put();
        b.put();
        z.put();
        t.put();
        CHECK(Counting::frees == 0 && live() == 1);
    }
    CHECK(live() == 0 && Counting::allocs == 1 && Counting::frees == 1);

    begin("an own allocation made while a pool is active is freed by put()");
    {
        Pool pool;
        CHECK(pool.reserve(4096) == 0);
        Arena carved, outside;
        CHECK(carved.get(&pool, 16) == 0 && outside.get(nullptr, 16) == 0 && outside.own && !carved.own && live() == 2);
        CHECK((char*)outside.p < pool.base || (char*)outside.p >= pool.base + pool.cap);
        outside.put();
        CHECK(Counting::frees == 1 && live() == 1 && !outside.p);
        carved.put();
        CHECK(Counting::frees == 1);
        CHECK(pool.reserve(8192) == 0 && Counting::frees == 2 && live() == 1 && pool.top == 0);      // the block is replaced
        Counting::fail_at = 1;
        CHECK(pool.reserve(64) == 2 && !pool.active() && pool.cap == 0 && live() == 0);
    }
    CHECK(live() == 0 && Counting::frees == 3);

    begin("grow-only: a request that fits makes no allocator call, a failed growth leaves an empty owner");
    {
        Arena a;
        CHECK(a.grow(nullptr, 0) == 0 && !a.p && Counting::allocs == 0);
        CHECK(a.grow(nullptr, 100) == 0 && a.cap == 100 && Counting::allocs == 1);
        const double* p = a.p;
        CHECK(a.grow(nullptr, 100) == 0 && a.grow(nullptr, 7) == 0 && a.grow(nullptr, 0) == 0 && a.p == p && a.cap == 100);
        CHECK(Counting::allocs == 1 && Counting::frees == 0);
        Counting::fail_at = 1;
        CHECK(a.grow(nullptr, 101) == 2 && !a.p && a.cap == 0 && !a.own && live() == 0 && Counting::frees == 1);
        CHECK(Counting::log.size() == 2 && Counting::log[1].first == 'f');       // put back BEFORE the new one is asked for
        CHECK(a.grow(nullptr, 101) == 0 && a.cap == 101 && Counting::log.back() == std::make_pair('a', size_t(808)));
        Pool pool;
        CHECK(pool.reserve(4096) == 0);
        Arena s;
        CHECK(s.grow(&pool, 10) == 0 && !s.own && s.grow(&pool, 10) == 0 && pool.top == 80);
        CHECK(s.grow(&pool, 1000) == dev_owner::POOL_FULL && !s.p && s.cap == 0);
    }
    CHECK(live() == 0);

    begin("fit-or-replace: kept up to 2 need + 2^20, replaced by need + need / 8 beyond; under a pool it always carves");
    {
        const size_t need = 4096, edge = 2 * need + (size_t(1) << 20);
        Arena a;
        CHECK(a.get(nullptr, edge) == 0);
        const double* p = a.p;
        Counting::reset();
        CHECK(a.fit(nullptr, need) == 0 && a.p == p && a.cap == edge && Counting::log.empty());
        CHECK(a.fit(nullptr, edge) == 0 && a.p == p && Counting::log.empty());         // exactly full
        Arena b;
        CHECK(b.get(nullptr, edge + 1) == 0);
        Counting::reset();
        CHECK(b.fit(nullptr, need) == 0 && b.cap == need + need / 8 && b.own);
        CHECK(Counting::log.size() == 2 && Counting::log[0].first == 'f' &&
              Counting::log[1] == std::make_pair('a', (need + need / 8) * sizeof(double)));
        Counting::reset();
        CHECK(b.fit(nullptr, b.cap + 1) == 0 && b.cap == (need + need / 8 + 1) + (need + need / 8 + 1) / 8);       // too small: replaced
        CHECK(Counting::log.size() == 2 && Counting::log[0].first == 'f');
        Counting::fail_at = 1;
        CHECK(b.fit(nullptr, 10 * need) == 2 && !b.p && b.cap == 0);
        Pool pool;
        CHECK(pool.reserve(1 << 20) == 0);
        Arena c;
        Counting::reset();
        CHECK(c.fit(&pool, need) == 0 && !c.own && c.cap == need && pool.top == need * 8);
        const double* first = c.p;
        CHECK(c.fit(&pool, need) == 0 && c.p != first && (char*)c.p - pool.base == (ptrdiff_t)(need * 8) && c.cap == need);
        CHECK(Counting::log.empty());
    }
    CHECK(live() == 0);

    begin("exact: an equal count keeps the arena, a different one frees first and then allocates");
    {
        Arena a;
        CHECK(a.exact(nullptr, 50) == 0 && a.cap == 50);
        const double* p = a.p;
        Counting::reset();
        CHECK(a.exact(nullptr, 50) == 0 && a.p == p && Counting::log.empty());
        CHECK(a.exact(nullptr, 49) == 0 && a.cap == 49);
        CHECK(Counting::log.size() == 2 && Counting::log[0].first == 'f' && Counting::log[1] == std::make_pair('a', size_t(49 * 8)));
        Counting::reset();
        CHECK(a.exact(nullptr, 51) == 0 && a.cap == 51 && Counting::log.size() == 2 && Counting::log[0].first == 'f');
        Arena e;
        CHECK(e.exact(nullptr, 0) == 0 && e.p && e.cap == 0 && Counting::log.back() == std::make_pair('a', size_t(8)));
        Counting::reset();
        CHECK(e.exact(nullptr, 0) == 0 && Counting::log.empty());
    }

    if (!Counting::live.empty()) {
        std::printf("%zu blocks still live at exit\n", Counting::live.size());
        ++failures;
    }
    if (failures) std::printf("%d checks FAILED\n", failures);
    else std::printf("all cases passed\n");
    return failures ? 1 : 0;
}
