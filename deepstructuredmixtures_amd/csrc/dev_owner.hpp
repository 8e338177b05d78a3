// Who owns the large device arenas: a Pool (one reserved block, carved in stack order) and an Arena (a move-only owner of `cap`
// doubles that knows whether it is an allocation of its own or a carved piece of the pool), with the three growth policies the
// library uses.  Plain C++17, neither HIP nor dsmgp_hip.h: `Mem` supplies the allocator as two static functions,
//     int Mem::alloc(void** p, size_t bytes)   0 on success, else the allocator's error code (> 0), passed through unchanged
//     void Mem::free(void* p)
// csrc/dsmgp_hip.cpp instantiates both with hipMalloc / hipFree and turns a status into its error code and message;
// tests/dev_owner_check.cpp instantiates them with a counting host allocator.
#pragma once
#include <algorithm>
#include <cstddef>
namespace dev_owner {

constexpr int POOL_FULL = -1;       // status of a carve that does not fit: Pool::need says what it asked for

template <class Mem>
struct Pool {
    char* base = nullptr;
    size_t cap = 0, top = 0;        // bytes
    size_t mark_plan = 0;           // top when the plan was complete: what is carved above it goes with the test set
    size_t need = 0;                // POOL_FULL: the top the refused carve would have reached

    Pool() = default;
    Pool(const Pool&) = delete;
    Pool& operator=(const Pool&) = delete;
    ~Pool() { release(); }

    bool active() const { return base != nullptr; }
    void release() {
        if (base) Mem::free(base);
        base = nullptr;
        cap = top = mark_plan = need = 0;
    }
    int reserve(size_t bytes) {     // replaces the block: nothing may be carved from the old one any more
        release();
        void* p = nullptr;
        if (int rc = Mem::alloc(&p, bytes)) return rc;
        base = static_cast<char*>(p);
        cap = bytes;
        return 0;
    }
    // `count` doubles (at least one) at the next multiple of 256 bytes; null, and `need` set, when they do not fit
    double* carve(size_t count) {
        const size_t bytes = std::max<size_t>(1, count) * sizeof(double);
        const size_t off = (top + 255) & ~size_t(255);
        if (off + bytes > cap) {
            need = off + bytes;
            return nullptr;
        }
        top = off + bytes;
        return reinterpret_cast<double*>(base + off);
    }
    void mark() { mark_plan = top; }
    void reset() { top = mark_plan = 0; }
    void reset_to_mark() { top = mark_plan; }
};

template <class Mem>
struct Arena {
    double* p = nullptr;
    size_t cap = 0;         // doubles asked for: set only once they are there
    bool own = false;       // an allocation of its own (put() frees it), not a piece of the pool (put() forgets it)

    Arena() = default;
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    Arena(Arena&& o) noexcept : p(o.p), cap(o.cap), own(o.own) { o.forget(); }
    Arena& operator=(Arena&& o) noexcept {
        if (this != &o) {
            put();
            p = o.p;
            cap = o.cap;
            own = o.own;
            o.forget();
        }
        return *this;
    }
    ~Arena() { put(); }

    // `count` doubles (at least one): carved from `pool` when there is one, else an allocation of its own.  What the arena held
    // is put back first; on failure it is empty.
    int get(Pool<Mem>* pool, size_t count) {
        put();
        if (pool) {
            p = pool->carve(count);
            if (!p) return POOL_FULL;
        } else {
            void* q = nullptr;
            if (int rc = Mem::alloc(&q, std::max<size_t>(1, count) * sizeof(double))) return rc;
            p = static_cast<double*>(q);
            own = true;
        }
        cap = count;
        return 0;
    }
    void put() {
        if (p && own) Mem::free(p);
        forget();
    }

    // Grow-only: kept while it holds `count` doubles, else put back BEFORE the new one is asked for (peak memory)
    int grow(Pool<Mem>* pool, size_t count) {
        if (count == 0 || (p && cap >= count)) return 0;
        return get(pool, count);
    }
    // Fit-or-replace: kept while it holds `need` doubles and is not wastefully large (at most twice what is needed, and 1 Mi
    // doubles), else replaced by one with an eighth to spare; under a pool it is carved anew, exactly
    int fit(Pool<Mem>* pool, size_t need) {
        if (pool) return get(pool, need);
        if (p && cap >= need && cap <= 2 * need + (size_t(1) << 20)) return 0;
        return get(nullptr, need + need / 8);
    }
    // Exact: kept only while it was asked for exactly `count` doubles
    int exact(Pool<Mem>* pool, size_t count) {
        if (p && cap == count) return 0;
        return get(pool, count);
    }

private:
    void forget() {
        p = nullptr;
        cap = 0;
        own = false;
    }
};
}  // namespace dev_owner
