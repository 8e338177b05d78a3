// C ABI (include/dsmgp_hip.h) and host orchestration of the GP-expert hot path on one MI355X.
// The host builds, once per leaf table, flat task lists for every block step of the batched
// left-looking Cholesky; fit!/predict then replay them as a fixed launch sequence on one stream.
#include "../../include/dsmgp_hip.h"
#ifdef DSMGP_DIAG
#include "../../include/dsmgp_hip_diag.h"
#endif
#include "kernels.hpp"
#include "kernels_agg.hpp"
#include "kernels_fused.hpp"
#include "kernels_targets.hpp"
#include "kernels_sample.hpp"
#include "kernels_kfold.hpp"
#include "kfold_plan.hpp"
#include "leaf_chunks.hpp"
#include "ctx_state.hpp"
#include "dev_owner.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <type_traits>
#include <array>
#include <chrono>
#include <dlfcn.h>
#include <limits>
#include <vector>

using namespace dsmgp;
using namespace ctx_state;
using leaf_chunks::for_leaf_chunks;

namespace {

std::string g_create_error;

struct HyperHost {
    int kind = -1;
    std::vector<double> loghyp;   // [logl..., logs, logNoise]
};

struct LeafHost {
    int n = 0, npad = 0, nb = 0, kid = 0;
    double mean = 0.0;
    int64_t obs_off = 0;
    int op = DSMGP_SHARE_FULL, src = -1;
    int64_t prefix = 0;
    int owner = -1;          // leaf whose factor buffer this leaf uses (itself unless COPY)
    int kb = 0;              // PREFIX: number of leading 128-blocks copied from src
    size_t f_off = 0, dinv_off = 0, vec_off = 0, xg_off = 0;
    // prediction
    int nt = 0, ntpad = 0;
    size_t vt_off = 0, xt_off = 0, pv_off = 0;
    int64_t route_off = 0;
};

// The large arenas and the reserved pool they may be carved from (dev_owner.hpp), on hipMalloc / hipFree.  A status of theirs
// becomes an error code and a message in arena_status.
struct HipMem {
    static int alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
using DevPool = dev_owner::Pool<HipMem>;
using DevArena = dev_owner::Arena<HipMem>;

// The one owner of a device array: every device allocation of the library that is not an arena or the pool (DevArena, DevPool)
// lives in one of these and is freed by it -- nothing is outside an owner.  `cap` is assigned in one place only, after a
// successful allocation (grow).
template <class T>
struct DevBuf {
    T* p = nullptr;
    size_t count = 0;       // entries in use (what a launch may cover)
    size_t cap = 0;         // entries allocated: a list that is replaced keeps its allocation while the new one fits (dev_upload)

    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), count(o.count), cap(o.cap) {
        o.p = nullptr;
        o.count = o.cap = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            std::swap(p, o.p);
            std::swap(count, o.count);
            std::swap(cap, o.cap);
        }
        return *this;
    }
    ~DevBuf() { release(); }

    // room for `need` entries, `count` = need: the allocation stays while it holds them, else the old one is freed BEFORE
    // `want` entries are asked for (peak memory).  On failure the owner is empty (p null, count and cap 0).
    int grow(dsmgp_ctx* c, size_t need, size_t want);
    int grow(dsmgp_ctx* c, size_t need) { return grow(c, need, std::max<size_t>(1, need + need / 8)); }
    int alloc(dsmgp_ctx* c, size_t n) { return grow(c, n, n); }      // exactly n entries when there is no room for n yet
    void clear() { count = 0; }             // an empty list; the allocation stays for the list that replaces it
    void release() {                        // a freed list is an EMPTY list: nobody may launch over its old count
        if (p) (void)hipFree(p);
        p = nullptr;
        count = cap = 0;
    }
    void drop(bool keep) { keep ? clear() : release(); }
};

// DSMGP_HOSTLOG=1: wall time of the host-side phases of plan building to stderr (diagnostic)
struct HostLog {
    const char* what;
    std::chrono::steady_clock::time_point t0;
    explicit HostLog(const char* w) : what(w), t0(std::chrono::steady_clock::now()) {}
    void lap(const char* next) {      // close the running phase, open the next
        done();
        what = next;
        t0 = std::chrono::steady_clock::now();
    }
    void done() {
        static const bool on = std::getenv("DSMGP_HOSTLOG") != nullptr;
        if (on && what)
            std::fprintf(stderr, "hostlog %-28s %.4f s\n", what,
                         std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
        what = nullptr;
    }
    ~HostLog() { done(); }
};

enum { STEP_CLASSIC = 0, STEP_FUSED = 1 };
constexpr int MAX_LANES = 4;
#ifndef DSMGP_FUSED_SHALLOW
#define DSMGP_FUSED_SHALLOW 4
#endif
constexpr int FUSED_SHALLOW_STEPS = DSMGP_FUSED_SHALLOW;   // block steps 0..4 (K <= 512) run fused where at least ...
constexpr int FUSED_SHALLOW_MIN_LEAVES = 32;               // ... this many leaves take part in the step
#ifndef DSMGP_STREAM_FLAGS
#define DSMGP_STREAM_FLAGS hipStreamDefault
#endif
#ifndef DSMGP_LANES_AUTO_MIN
#define DSMGP_LANES_AUTO_MIN 8
#endif
// two leaf lanes (dsmgp_ctx::nlanes) from this many sharing groups on.  Same-box A/B, one lane -> two (profiles/r05_lanes_ab.log): headline
// (144 leaves) 0.4084 / 0.4079 -> 0.3926 / 0.3912 s; depth 4 (18k leaves) 0.0512 / 0.0514 -> 0.0498 / 0.0499; the shards of 2-, 4- and
// 8-rank jobs (72 / 36 / 18 leaves) 0.2110 -> 0.1994, 0.1082 -> 0.1044, 0.0584 -> 0.0572; PoE of 128 experts 4.72 -> 4.67 ms
constexpr int LANES_AUTO_MIN_LEAVES = DSMGP_LANES_AUTO_MIN;
// The tail of an update launch (UpdateSplitter::add_step): K pieces per tile, and full rounds of tiles that join the tail in
// launches of under two rounds -- with ONE leaf lane, and with two or more (where the other lane's launch fills the slots a tail
// leaves idle and cutting it only costs: see add_step)
#ifndef DSMGP_TAIL_SPLIT_DEFAULT
#define DSMGP_TAIL_SPLIT_DEFAULT 4
#endif
#ifndef DSMGP_TAIL_ROUNDS_DEFAULT
#define DSMGP_TAIL_ROUNDS_DEFAULT 1
#endif
#ifndef DSMGP_TAIL_SPLIT_LANES
#define DSMGP_TAIL_SPLIT_LANES 1
#endif
#ifndef DSMGP_TAIL_ROUNDS_LANES
#define DSMGP_TAIL_ROUNDS_LANES 0
#endif
#ifndef DSMGP_SYM_SHARE
#define DSMGP_SYM_SHARE 0                // > 0: diagonal tiles run as FULL tiles where they are under 1 / this of a launch's tiles (A/B builds)
#endif
#ifndef DSMGP_PAD_SHARE
#define DSMGP_PAD_SHARE 0                // > 0: short tiles take the column-split form only from 1 / this of a launch's tiles on (A/B builds)
#endif
#ifndef DSMGP_SOLO_FACTOR
#define DSMGP_SOLO_FACTOR 1.56             // time of one workgroup alone on a CU relative to its share of a co-resident pair
#endif
#ifndef DSMGP_DFIN_BACK
#define DSMGP_DFIN_BACK (-1)             // < 0: the diagonal-block tasks of a full update launch go last; >= 0: that many rounds of
                                         // whole tiles before its tail pieces (diagnostic builds: A/B of the placement)
#endif

struct StepLists {
    // one phase (wave) of factorisation: per block step k the tasks for update / split-K reduce / diag / trsm
    std::vector<int> upd_off, red_off, diag_off, trsm_off;   // size nsteps+1
    std::vector<int> step_tiles;                             // whole update tiles per step (before split-K)
    std::vector<char> pad;                                   // per step: >= 10 % of the tiles have rows 64.. all padding
    DevBuf<TileTask> upd, trsm;
    DevBuf<ReduceTask> red;
    DevBuf<DiagTask> diag;
    // steps with more diagonal blocks than CUs run fused (kernels_fused.hpp): diag_fused_reg_kernel, then tile_fused8_kernel
    std::vector<int> fdiag_off, ftile8_off;                  // size nsteps+1; a fused step has no classic tasks and vice versa
    std::vector<char> mode;                                  // STEP_* per step
    DevBuf<DiagFusedTask> fdiag;
    DevBuf<FusedTask8> ftile8;                               // eight 16-row blocks below a diagonal block each
    // classic steps with the diagonal block INSIDE the update launch (DiagFinishTask, kernels_fused.hpp): the update launch of
    // step k carries dfin[dfin_off[k] .. dfin_off[k+1]) behind its first dpos[k] tile tasks; a leaf whose diagonal block rides
    // there has no `diag` task in that step
    std::vector<int> dpos, dfin_off;                         // size nsteps / nsteps+1
    DevBuf<DiagFinishTask> dfin;
    int nsteps = 0;

    void drop(bool keep) {
        upd.drop(keep);
        trsm.drop(keep);
        red.drop(keep);
        diag.drop(keep);
        fdiag.drop(keep);
        ftile8.drop(keep);
        dfin.drop(keep);
    }
};

// A blocked triangular sweep after a fit -- the prediction sweep V^T = K_tn L^-T, the L^-T inversion of the gradient pass -- run
// lane by lane like the factorisation (dsmgp_ctx::nlanes): one device list of each kind for all lanes, lane q's tasks behind those
// of the lanes before it and its split-K slabs behind theirs; the tasks of lane q's block step k are entry q * nsteps + k of the
// offset tables.  One lane's panel solves and reduces run under the other's update launches.
struct SweepLists {
    int nsteps = 0, nlanes = 1;
    std::vector<int> upd_off, red_off, trsm_off;   // size nlanes * nsteps + 1
    DevBuf<TileTask> upd, trsm;
    DevBuf<ReduceTask> red;
    std::vector<int> f8_off;                       // fused 8-block tasks per (lane, step), made on the device (build_sweep8_kernel);
    DevBuf<FusedTask8> f8;                         // empty where the sweep has none (the gradient pass)
    DevArena slab;                                 // split-K workspace of all lanes (grow-only)

    void drop(bool keep) {   // keep: empty lists; the allocations and the slab stay for the lists that replace them
        nsteps = 0;
        upd.drop(keep);
        trsm.drop(keep);
        red.drop(keep);
        f8.drop(keep);
        if (!keep) slab.put();
    }
};

// Collects the update tiles of one block step and splits their K range over several workgroups when
// the step has too few tiles to fill the chip (tail of the factorisation, prediction sweeps).
// Cost model in units of one K column on one CU: a workgroup costs (K/S + C0), rounds = ceil(T*S / CUs).
// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b+8 share an XCD and its L2), so a run
// of tasks that read the same B panel should sit at positions x, x+8, x+16, ...  Reorder [begin,end) so
// that XCD slot x receives a contiguous chunk of the natural (leaf-major) order.  Speed only.
template <class T, class U>
void xcd_permute(std::vector<T>& a, std::vector<U>& b, size_t begin, size_t end, bool enable) {
    const size_t n = end - begin;
    if (!enable || n < 16) return;
    const size_t q = n / 8, r = n % 8;
    std::vector<T> ta(a.begin() + begin, a.begin() + end);
    std::vector<U> tb(b.begin() + begin, b.begin() + end);
    size_t src = 0;
    for (size_t x = 0; x < 8; ++x) {
        const size_t len = q + (x < r ? 1 : 0);
        for (size_t j = 0; j < len; ++j, ++src) {
            a[begin + x + 8 * j] = ta[src];
            b[begin + x + 8 * j] = tb[src];
        }
    }
}

// The same for a launch whose tasks differ in depth (the contraction tiles of the gradient pass: one launch, depths from
// 1 to nb blocks).  An XCD slot works through its share of the list on its own, so equal COUNTS per slot leave the slots
// with unequal work and the launch waits for the slowest eighth of the chip.  Blocks of tasks that share operands
// (`block_start`, natural order = deepest first) are dealt to the slot with the least work so far; the counts are then
// evened out (the positions of a slot are x, x+8, ...: every slot needs n/8 tasks) by moving tasks from the ends of the
// fuller slots, which are the shallowest.
template <class T, class U>
void xcd_deal_by_work(std::vector<T>& a, std::vector<U>& b, size_t begin, size_t end, const std::vector<size_t>& block_start,
                      const std::vector<double>& work, bool enable) {   // block_start / work: relative to `begin`
    const size_t n = end - begin;
    if (!enable || n < 16) return;
    std::vector<std::vector<size_t>> q(8);
    double load[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (size_t bi = 0; bi + 1 < block_start.size(); ++bi) {
        int x = 0;
        for (int y = 1; y < 8; ++y)
            if (load[y] < load[x]) x = y;
        for (size_t i = block_start[bi]; i < block_start[bi + 1]; ++i) {
            q[x].push_back(i);
            load[x] += work[i];
        }
    }
    std::vector<size_t> pool;
    for (size_t x = 0; x < 8; ++x) {
        const size_t target = n / 8 + (x < n % 8 ? 1 : 0);
        while (q[x].size() > target) {
            pool.push_back(q[x].back());
            q[x].pop_back();
        }
    }
    for (size_t x = 0; x < 8; ++x) {
        const size_t target = n / 8 + (x < n % 8 ? 1 : 0);
        while (q[x].size() < target) {
            q[x].push_back(pool.back());
            pool.pop_back();
        }
    }
    const std::vector<T> ta(a.begin() + begin, a.begin() + end);
    const std::vector<U> tb(b.begin() + begin, b.begin() + end);
    for (size_t x = 0; x < 8; ++x)
        for (size_t j = 0; j < q[x].size(); ++j) {
            a[begin + x + 8 * j] = ta[q[x][j]];
            b[begin + x + 8 * j] = tb[q[x][j]];
        }
}

struct UpdateSplitter {
    int ncu = 256;
    bool xcd = true;
    int tail_split = DSMGP_TAIL_SPLIT_DEFAULT;     // K pieces per tile in the tail of a launch (1 = the tail is not cut)
    int tail_rounds = DSMGP_TAIL_ROUNDS_DEFAULT;   // full rounds (of ncu tiles) that belong to the tail
    std::vector<TileTask> upd;
    std::vector<ReduceTask> red;
    std::vector<int64_t> upd_slab, red_slab;   // slab index of a task's output / first slab, -1 = none
    size_t tail_begin = 0;                     // add_step: index in `upd` where the tail pieces of the last step begin (its end if none)
    size_t max_slabs = 0;

    // Cost model in units of one K column at the matrix pipe's full rate on one CU.  A CU holds two workgroups: two co-resident
    // pieces of depth d share the pipe and are both done after 2 d; ONE piece alone on a CU cannot saturate it (a wave issues an
    // f64 MFMA every ~100 cycles where the pipe takes one every 64: kernels.hpp, chol_diag_packed_body) and takes 1.56 d.
    // (Until round 4 the model counted rounds over `ncu` slots at d per round: right for pairs, but it left a step of 129..255
    // tiles unsplit -- one workgroup per CU at 64 % of the pipe -- where two half-depth pieces per CU take 36 % less time.)
    static int choose_split(int T, int K, int ncu) {
        if (T <= 0 || K < 512) return 1;
        const double C0 = 96.0, CRED = 64.0;
        const int chunks = K / KC;
        auto cost = [&](int S) {
            const double depth = (double)((chunks + S - 1) / S) * KC;
            const long P = (long)T * S, slots = 2L * ncu;
            const long full = P / slots, rem = P % slots;
            double t = (double)full * 2.0 * (depth + C0);
            if (rem > ncu) t += 2.0 * (depth + C0);
            else if (rem > 0) t += DSMGP_SOLO_FACTOR * depth + C0;
            return t + (S > 1 ? CRED : 0.0);
        };
        int best = 1;
        double bc = cost(1);
        for (int S = 2; S <= 64 && S * 256 <= K && (long)T * S <= 4096; ++S) {
            const double c = cost(S);
            if (c < 0.93 * bc) {     // (0.65 / 0.80 / 1.0 under two lanes: no difference, profiles/r05_tail_ab.log)
                bc = c;
                best = S;
            }
        }
        return best;
    }
    // Emit `tiles[from, to)` split S ways (S = 1: as they are), split-major, XCD-ordered.
    void emit(const std::vector<TileTask>& tiles, size_t from, size_t to, int S, size_t& slab) {
        const size_t begin = upd.size();
        if (S <= 1) {
            for (size_t i = from; i < to; ++i) {
                upd.push_back(tiles[i]);
                upd_slab.push_back(-1);
            }
            xcd_permute(upd, upd_slab, begin, upd.size(), xcd);
            return;
        }
        const size_t first = slab;
        for (size_t i = from; i < to; ++i) {
            ReduceTask r{};
            r.C = tiles[i].C;
            r.ldc = tiles[i].ldc;
            r.nsplit = S;
            // piece 0 stores product - Gram value, or the tile is defined as -product: nothing to read from it
            r.fresh = (tiles[i].gram != 0 || tiles[i].update == 2) ? 1 : 0;
            red.push_back(r);
            red_slab.push_back((int64_t)(first + (i - from) * S));
        }
        // split-major order: tasks with the same K range (and, per leaf, the same B panel) stay adjacent
        for (int s = 0; s < S; ++s)
            for (size_t i = from; i < to; ++i) {
                TileTask p = tiles[i];
                const long chunks = (tiles[i].k1 - tiles[i].k0) / KC;   // this tile's own K range
                p.k0 = tiles[i].k0 + (int)(chunks * s / S) * KC;
                p.k1 = tiles[i].k0 + (int)(chunks * (s + 1) / S) * KC;
                p.update = 0;
                p.C = nullptr;
                p.ldc = TB;
                if (s != 0) p.gram = 0;
                upd.push_back(p);
                upd_slab.push_back((int64_t)(first + (i - from) * S + s));
            }
        xcd_permute(upd, upd_slab, begin, upd.size(), xcd);
        slab += (to - from) * (size_t)S;
    }
    // tiles: tasks of one block step with update = 1 and (nearly) equal depth K.
    // Fewer tiles than CUs: split all of them (cost model).  Otherwise the step runs in rounds of one tile
    // per CU; the last, partial round would hold the whole launch for a full tile time, so only the
    // remainder tiles are split, finely enough to fit one short extra round, and issued last.
    void add_step(const std::vector<TileTask>& tiles, int K) {
        const size_t T = tiles.size();
        size_t slab = 0;
        if ((int)T < ncu) {
            tail_begin = upd.size();       // every tile is cut along K: one short round
            emit(tiles, 0, T, choose_split((int)T, K, ncu), slab);
        } else {
            // Whole tiles first, in rounds of one per CU; the tail of the launch -- the partial last round plus
            // `tail_rounds` full ones -- is cut into `tail_split` K pieces per tile and issued last, so the
            // launch ends on short tasks instead of idling CUs for up to a whole tile time.
            // The extra full round(s) in the tail pay off only in launches of under two rounds (measured, round 2: a round
            // of 256 extra tiles cut in four costs the headline step 3 ms of reduce traffic for nothing, while the 8-rank
            // shard, whose launches are that short, gains 1.7 % from it; with this rule: headline 0.4048 / 0.4019 ->
            // 0.3989 / 0.3993 s, 4-rank shard 0.1080 / 0.1070 -> 0.1051 / 0.1054 s, 8-rank shard and depth 4 unchanged).
            // Round 5: with two leaf lanes the other lane's launch runs in the slots a tail leaves idle, and the cut tail only
            // costs (its slabs, the reduce launch on the chain): tail_split 4 -> 1 and tail_rounds 1 -> 0 WHERE THE PLAN HAS LANES,
            // same box, alternating: headline 0.3871 / 0.3862 -> 0.3825 / 0.3838 s, 8-rank shards 0.0548 / 0.0559 -> 0.0531 / 0.0534
            // and 0.0551 / 0.0557 -> 0.0531 / 0.0531, 4-rank shard 0.1018 / 0.1024 -> 0.1000 / 0.1009, depth 4 unchanged; with one
            // lane the same setting costs 4 % (0.4090 / 0.4116 -> 0.4261 / 0.4266; shards +2-3 %): profiles/r05_tail_ab.log.  What
            // stays with lanes: a remainder of under a quarter round is cut finely enough to fill one round (below).
            const size_t r = T % (size_t)ncu;
            size_t ntail = r + (T < (size_t)(2 * ncu) ? (size_t)tail_rounds * ncu : 0);
            if (ntail > T) ntail = T;
            int S = std::min(tail_split, std::max(1, K / 256));
            if (r > 0 && r * 4 < (size_t)ncu) S = std::max(S, (int)std::min<size_t>((size_t)ncu / r, 16));   // tiny remainder: finer
            S = std::min(S, std::max(1, K / 256));
            if (S <= 1 || r == 0) ntail = 0;   // an exact multiple of the CU count already ends evenly
            // (Round 4 tried cutting the last ncu whole tiles in two along K where the whole tiles make an odd number of ncu-rounds
            // -- the reasoning: two workgroups per CU, so an odd round would run one workgroup per CU at 64 % of the pipe.  No
            // effect: headline 0.3847 / 0.3848 / 0.3854 without, 0.3847 / 0.3860 / 0.3853 with; slots free up one by one, there
            // is no such round.)
            emit(tiles, 0, T - ntail, 1, slab);
            tail_begin = upd.size();
            if (ntail) emit(tiles, T - ntail, T, S, slab);
        }
        max_slabs = std::max(max_slabs, slab);
    }
    // A step whose tiles have every depth from 1 to `kblocks` blocks (the blocks of L^-T), listed leaf by leaf, deepest
    // first.  Tasks are dispatched in list order, so the deepest tiles of the last leaves start when the launch is nearly
    // over and the chip waits for them (15 % of a launch at k = 41).  Reordering by depth is not an option -- the tiles
    // of a leaf must run together to share their B panel through L2 (passes over the leaves by depth class: 35 % slower)
    // -- so the last two rounds' worth of tiles are cut along K into pieces of at most a quarter of the step's depth.
    int ragged_rounds = 2, ragged_div = 4;
    void add_step_ragged(const std::vector<TileTask>& tiles, int Kavg, int kblocks) {
        const size_t T = tiles.size();
        if (kblocks < 8) {
            add_step(tiles, Kavg);
            return;
        }
        size_t slab = 0;
        size_t cut = 0;
        int maxb;
        if (T < (size_t)((ragged_rounds + 2) * ncu)) {
            // few tiles (the late steps: a handful of leaves, every depth): all of them in pieces of equal depth, about
            // three pieces per workgroup slot of the chip
            long W = 0;
            for (const TileTask& u : tiles) W += (u.k1 - u.k0) / TB;
            maxb = (int)std::min<long>(kblocks, std::max<long>(2, W / (long)(2 * ncu * 3)));
        } else {
            cut = T - (size_t)(ragged_rounds * ncu);
            emit(tiles, 0, cut, 1, slab);
            maxb = std::max(1, kblocks / ragged_div);
        }
        auto pieces = [&](const TileTask& u) { return std::max(1, ((u.k1 - u.k0) / TB + maxb - 1) / maxb); };
        for (size_t i = cut; i < T;) {
            const int S = pieces(tiles[i]);
            size_t j = i + 1;
            while (j < T && pieces(tiles[j]) == S) ++j;
            emit(tiles, i, j, S, slab);
            i = j;
        }
        max_slabs = std::max(max_slabs, slab);
    }
    void bind(double* workspace) {
        for (size_t i = 0; i < upd.size(); ++i)
            if (upd_slab[i] >= 0) upd[i].C = workspace + (size_t)upd_slab[i] * TB * TB;
        for (size_t i = 0; i < red.size(); ++i) red[i].slabs = workspace + (size_t)red_slab[i] * TB * TB;
    }
};

// One lane's part of a SweepLists while the host builds it: the update tiles through the lane's splitter, the panel solves, and
// per block step where its tasks begin in the two (the gradient pass's step 0 has no tasks and is not marked: it begins at 0)
struct SweepLane {
    UpdateSplitter U;
    std::vector<TileTask> trsm;
    std::vector<int> upd_at, red_at, trsm_at;     // size nsteps
    void mark(int k) {
        upd_at[(size_t)k] = (int)U.upd.size();
        red_at[(size_t)k] = (int)U.red.size();
        trsm_at[(size_t)k] = (int)trsm.size();
    }
};

}  // namespace

// A contraction list of the gradient passes (build_dot_list): tasks [first[p], first[p + 1]) belong to the kinds of KindInfo::dot_pass == p and are run by that pass's
// kernel; leaf_of[i] is the leaf of task i.
struct DotRanges {
    size_t first[5] = {0, 0, 0, 0, 0};
    std::vector<int> leaf_of;
    size_t count() const { return first[4]; }
};

// The context's storage, one struct per LIFETIME: each is a base of dsmgp_ctx, and what it declares falls together, in one place.
// A group that is only ever released falls by assignment from a default-constructed value (reset<G>): the owners release or put
// on move-assignment and the default member initialisers are the resets, so a member added to such a group needs no further line.
// A group that is sometimes emptied and kept has one drop(bool keep) under its declarations.

// PlanStore.  Built by build_plan (arenas, leaf table, build_schedule's lists) and ensure_phase (phase, slabF); stands behind
// P_PLAN and P_PHASE; falls in free_plan: new training data, leaf table, sharing schedule, plan option, pool or dsmgp_release.
struct PlanStore {
    // the large arenas: each owns its doubles or knows that they are a piece of the pool (dev_owner.hpp)
    DevArena arenaF, arenaDinv;
    DevArena arenaVec;              // per leaf: yc, w, z, alpha (4 x npad)
    DevArena arenaXg;
    DevBuf<int> d_info;
    DevBuf<int> d_owner;            // per leaf: the leaf whose factor (and info slot) it uses (dsmgp_fit_exchange packs info per owner)
    DevBuf<double> d_mll;
    DevBuf<LeafDev> d_leaves;
    DevBuf<GramTask> gram;          // Gram launch of fit!: every lower tile, or (fused) the tiles no update task writes
    std::vector<char> fused_step[2];    // per phase and block step: STEP_* (build_schedule; see dsmgp_ctx::fuse_steps)
    std::vector<char> leaf_lane;    // per leaf (COPY / PREFIX leaves: their source's)
    StepLists phase[MAX_LANES][2];  // [lane][0: FULL leaves, 1: PREFIX leaves (need their source first)]
    std::vector<char> leaf_group;   // per leaf: the phase it belongs to (COPY leaves ride with their source)
    DevArena slabF[MAX_LANES];      // split-K workspace of the factorisation, per lane
    std::vector<int> fwd_off, bwd_off;
    DevBuf<SolveTask> fwd, bwd;
    int solve_steps = 0;
    DevBuf<DiagTask> dinvc_prefix;  // copied blocks of PREFIX leaves whose source factorised them in a fused step: completed right
                                    // after the copy (the classic steps of the PREFIX phase solve against Dinv_k)
    DevBuf<DiagTask> dinvc_fwd;     // blocks of the leaves whose z comes from the forward sweep (COPY, PREFIX): completed before it
    DevBuf<DiagTask> dinvc_all;     // every diagonal block a fused step factorises WITHOUT its inverse (only L_kk and the 16x16 diagonal
                                    // inverses exist after a fit): dinv_complete_kernel over this list produces the rest of Dinv_k for
                                    // whoever needs it (ensure_dinv).  Owned by the PLAN -- the list is the same with and without test
                                    // rows riding along, and must outlive a test set that is replaced between a fit and its first use
};
static_assert(std::is_nothrow_move_assignable_v<PlanStore>, "PlanStore falls by assignment (reset)");

// TestInputs.  The registered test set as the caller gave it: the rows, the route CSR, the row / entry index.  Built by the
// registration (dsmgp_set_test*); stands behind P_TEST; falls in free_test, NOT in free_test_products: dsmgp_add_rows_keep_test
// keeps it across a rebuilt plan.  Its counts (n_t, route_ptr, route_total, vt_first) are plain members of the context.
struct TestInputs {
    DevBuf<double> dXt;
    DevBuf<int64_t> d_route_ptr, d_route_idx;
    // aggregation of the leaf moments per test row + scores (dsmgp_aggregate*, dsmgp_scores)
    DevBuf<int64_t> d_row_ptr;      // n_t + 1: entries of every test row (built by set_test)
    DevBuf<int32_t> d_row_ent;      // entry positions, ascending per row
    DevBuf<int32_t> d_ent_leaf;     // leaf of every entry position

    void drop(bool keep) {          // keep: a registration that replaces another
        dXt.drop(keep);
        d_route_ptr.drop(keep);
        d_route_idx.drop(keep);
        d_row_ptr.drop(keep);
        d_row_ent.drop(keep);
        d_ent_leaf.drop(keep);
    }
};

// TestProducts.  What is made from a registered test set: built by register_test, ensure_joint and, on first use and not part of
// bytes_needed, by the prediction entry points (predict_cov, predict_gradients, predict_targets, aggregate); stands behind P_TEST,
// P_JOINT and what is below them; falls in free_test_products: the set is dropped or replaced, or the plan under it goes.
struct TestProducts {
    DevBuf<double> d_agg_part;      // W x n_t partial sums
    DevBuf<double> d_agg_coef;      // L
    DevBuf<int32_t> d_agg_group;    // L
    DevBuf<double> d_agg_out;       // mu | var (n_t each) | y_test (n_t) | score block sums
    DevBuf<double> d_agg_gpart;     // dsmgp_aggregate_gradients*: Wg x n_t gradient sums (agg_width with D)
    DevBuf<double> d_agg_gout;      // dmu | dvar of the aggregated prediction, n_t x D each
    DevBuf<double> d_col_coef;      // dsmgp_aggregate_columns*: L, a state of its own beside d_agg_*
    DevBuf<int32_t> d_col_group;    // L
    DevBuf<double> d_col_out;       // mu | var of every column, n_t x Q each
    DevBuf<double> d_col_gout;      // dmu | dvar of every column, n_t x D x Q each
    DevArena arenaVt;               // K_tn: a test set that replaces another takes the arenas of the old one over while it fits
                                    // (DevArena::fit; releasing ~10 GB and asking the driver for them again took up to 0.6 s of a
                                    // 0.06 s predict)
    DevArena arenaXt;
    DevArena arenaPV;               // mu | var (route order, unpadded) | macc | sacc (padded accumulators of the sweep)
    DevBuf<GramTask> pgram;         // K_tn tiles the standalone sweep reads from memory (all of them only when D > 32)
    DevBuf<GramTask> pgram0;        // ... of the joint fit when the Gram is fused: block column 0 only
    DevBuf<PredTask> ptasks;
    DevBuf<PredTask> ptasks_slow;   // test tiles of leaves whose z is not produced during the factorisation
    SweepLists psweep;              // V^T = K_tn L^-T; in the block steps that run fused: update + solve of eight 16-row blocks per task
    DevBuf<SweepSeg> psegs;         // (leaf, block step) pairs of the sweep's fused steps: build_sweep8_kernel makes the tasks
    // dsmgp_add_rows_keep_test (see dsmgp_ctx::vt_first)
    DevBuf<KeptSumTask> kept_tasks; // the moment sums of the kept columns (kept_sums_kernel), their partial sums and finish tasks
    DevBuf<KeptFinTask> kept_fin;
    DevBuf<double> d_kept_part;
    bool resume_armed = false;
    bool sweep_resumed = false;     // psweep / pgram skip block steps (built from vt_first): rebuilt from block 0 when next needed
    DevArena arenaCov;              // ntpad x ntpad of the leaf dsmgp_predict_cov was last asked for (grow-only, from the pool when there is one)
    DevBuf<PredCovTask> pcov;       // its lower tiles, rebuilt per call
    // joint draws (dsmgp_predict_sample, kernels_sample.hpp).  P_SAMPLE: arenaSample holds chol(Sigma_l + jitter I) of every leaf with
    // routed rows for the tag (sample_noise, sample_jitter); the lists are rebuilt per factorisation, the draw's per call
    DevArena arenaSample;           // ntpad x ntpad per leaf with routed rows, at sample_off (grow-only, from the pool when there is one)
    DevArena arenaSampleDinv;       // the inverted diagonal blocks of the block steps, ntpad x 128 per leaf (scratch of the factorisation)
    std::vector<size_t> sample_off; // per leaf: offset of its factor in arenaSample
    std::vector<int32_t> sample_info;       // per leaf: 0, the first bad minor, or -1 (the flags of the current factors)
    int sample_noise = 0;
    double sample_jitter = 0.0;
    double sample_seconds[3] = {0.0, 0.0, 0.0};     // device seconds of the last call: Sigma, factorisation (0, 0: the factors were current), draws
    DevBuf<PredCovTask> scov;       // the lower tiles of every Sigma_l
    DevBuf<TileTask> supd, strsm;   // the block steps: step k's tasks are [s*_off[k], s*_off[k + 1])
    DevBuf<TileTask> sres, strsm2, sadd;    // the refinement of a step's panel solves, task for task beside strsm
    DevBuf<DiagTask> sdiag;
    DevBuf<int> d_sinfo;            // L flags
    DevBuf<SampleDrawTask> sdraw;   // (row tile, 16 columns) pairs
    DevBuf<double> d_seps, d_sout;  // the staged normals and the draws, route_total x S rounded up to 16 (ld = route_total)
    // input gradients of the predictive moments (dsmgp_predict_gradients): lists rebuilt per call
    DevArena arenaB;                // B = Vt L^-1 (rows K_y^-1 k_t), ntpad x npad per leaf with routed rows, laid out like arenaVt (grow-only,
                                    //   from the pool when there is one)
    DevBuf<PredBetaTask> pgbeta;    // the tiles of B
    DevBuf<PredGradTask> pgtasks;   // (test tile, slab of training rows) pairs
    DevBuf<PredGradFinTask> pgfin;  // test tiles
    DevBuf<double> d_pgpart;        // the slabs' sums
    DevBuf<double> d_pgout;         // dmu | dvar (absent in a mean-only call), route_total x D each (ld = route_total)
    // dsmgp_predict_targets.  They depend on the resident columns as well: free_targets releases these two by name
    DevBuf<TargetsMuTask> tmu;      // test tiles, rebuilt per call
    DevBuf<double> d_tmu;           // mu, route_total x Q (ld = route_total)
    // dsmgp_predict_columns_gradients: a group of its own (nothing of dsmgp_predict_gradients is written), lists rebuilt per call
    DevBuf<TargetsInputGradTask> tigtasks;      // (test tile, slab of training rows) pairs
    DevBuf<TargetsInputGradFinTask> tigfin;     // test tiles
    DevBuf<double> d_tigpart;       // the slabs' sums: D x Qpad planes of 128 rows per task
    DevBuf<double> d_tigout;        // dmu, route_total x D x Q (ld = route_total)
    StepLists phaseJ[MAX_LANES][2]; // PlanStore::phase with the resident test rows riding along (ensure_joint)
    DevArena slabJ[MAX_LANES];

    // keep: every buffer stays allocated for what replaces it (emptied, not freed).  Two asymmetries, on purpose: the three big
    // arenas (Vt, Xt, PV) stay under `keep` as they are -- DevArena::fit takes them over or replaces them -- and arenaCov, arenaB
    // and slabJ are put back either way.
    void drop(bool keep) {
        d_agg_part.drop(keep);
        d_agg_coef.drop(keep);
        d_agg_group.drop(keep);
        d_agg_out.drop(keep);
        d_agg_gpart.drop(keep);
        d_agg_gout.drop(keep);
        d_col_coef.drop(keep);
        d_col_group.drop(keep);
        d_col_out.drop(keep);
        d_col_gout.drop(keep);
        if (!keep) {
            arenaVt.put();
            arenaXt.put();
            arenaPV.put();
        }
        pgram.drop(keep);
        pgram0.drop(keep);
        ptasks.drop(keep);
        ptasks_slow.drop(keep);
        psweep.drop(keep);
        psegs.drop(keep);
        kept_tasks.drop(keep);
        kept_fin.drop(keep);
        d_kept_part.drop(keep);
        resume_armed = sweep_resumed = false;
        arenaCov.put();
        pcov.drop(keep);
        arenaSample.put();
        arenaSampleDinv.put();
        sample_off.clear();
        sample_info.clear();
        scov.drop(keep);
        supd.drop(keep);
        strsm.drop(keep);
        sres.drop(keep);
        strsm2.drop(keep);
        sadd.drop(keep);
        sdiag.drop(keep);
        d_sinfo.drop(keep);
        sdraw.drop(keep);
        d_seps.drop(keep);
        d_sout.drop(keep);
        arenaB.put();
        pgbeta.drop(keep);
        pgtasks.drop(keep);
        pgfin.drop(keep);
        d_pgpart.drop(keep);
        d_pgout.drop(keep);
        tmu.drop(keep);
        d_tmu.drop(keep);
        tigtasks.drop(keep);
        tigfin.drop(keep);
        d_tigpart.drop(keep);
        d_tigout.drop(keep);
        for (auto& lane : phaseJ)
            for (auto& ph : lane) ph.drop(keep);
        for (auto& sl : slabJ) sl.put();
    }
};

// GradLists.  The task lists of the gradient pass under the current mask, and what describes them.  Built by build_grad_plan;
// stand behind P_GRAD_LISTS; emptied in free_grad_lists (the mask changes: finetune! changes it L times per iteration,
// src/finetuning.jl:34-57, and the lists that replace these fit into the same buffers), released in free_grad.
struct GradLists {
    DevBuf<TransTask> gtrans;
    SweepLists ginv;                // Xt = L^-T (no fused tasks)
    DevBuf<FrobTask> gfrob;
    std::vector<int> gfrob_leaf;    // owner leaf of each frob task
    DevBuf<GradTask> gdot;
    DotRanges gdot_ranges;          // its four kernel ranges and the leaf of each task
    DevBuf<ArdLinTask> gardlin;     // ArdLinear leaves: column groups of L^-T (ardlin_quad_kernel)
    std::vector<int> gardlin_leaf;  // leaf of each of them
    int gstride = 2;                // doubles per contraction task in d_gpart
    size_t gpart_count = 0;         // doubles of d_gpart (GradStore) these lists write

    void drop(bool keep) {          // keep: the allocations and the sweep's slab stay
        gtrans.drop(keep);
        ginv.drop(keep);
        gfrob.drop(keep);
        gfrob_leaf.clear();
        gdot.drop(keep);
        gdot_ranges = DotRanges{};
        gardlin.drop(keep);
        gardlin_leaf.clear();
        gstride = 2;
        gpart_count = 0;
    }
};

// GradStore.  What the gradient pass, dsmgp_loo and dsmgp_loo_gradients keep beside GradLists: built on first use (build_grad_plan,
// build_loo_plan, the lists of dsmgp_loo_gradients), not part of bytes_needed; stands behind P_XINV, P_LOO_LISTS and P_LG_LISTS;
// falls in free_grad: with the plan, with a change of kernel kind or of the ARD gradient option, and with whatever moves the pool's
// stack below it.
struct GradStore {
    DevArena arenaX;                // Xt = L^-T per factor owner, npad x npad (kept only while the total is exactly the same)
    DevBuf<double> d_gpart;         // partial results: frob | graddot pairs | per-leaf dots | ArdLinear quadratic forms (2 D per task)
    // leave-one-out (dsmgp_loo): reads the same L^-T arena
    DevBuf<RowNormTask> lrow;
    DevBuf<LooTask> lleaf;
    DevBuf<double> d_loo;           // row-sum planes of every owner | mu | var (obs_ptr[L] each) | lpd (L)
    // gradients of the LOO density (dsmgp_loo_gradients)
    DevArena arenaH;                // H = K_y^-1 diag(sqrt w) per computing leaf, npad x npad
    DevBuf<double> d_lgvec;         // [alpha | u | sqrt w | alpha / (d sqrt w)] per computing leaf, npad each
    DevBuf<LooVecTask> lgvec;
    DevBuf<GinvTask> lginv;
    DevBuf<LooHvecTask> lghvec;
    std::vector<int> lghvec_leaf;
    DevBuf<GradTask> lgdot;         // as gdot: IsoSE / ArdSE | ArdSEProduct | Matern | rational quadratic
    DotRanges lgdot_ranges;
    int lgstride = 2;               // doubles per contraction task in d_lgpart: 2 + D, one more with a rational quadratic id
    DevBuf<ArdLinTask> lgardlin;
    std::vector<int> lgardlin_leaf;
    DevBuf<double> d_lgpart;        // weights 2 L | hvec pairs | graddot x (2 + D) | ArdLinear 3 D per task
};
static_assert(std::is_nothrow_move_assignable_v<GradStore>, "GradStore falls by assignment (reset)");

// TargetsStore.  Several target columns on the current factors (dsmgp_solve_targets and what reads its Z, kernels_targets.hpp):
// built on first use, not part of bytes_needed, the arenas from the pool when there is one; stands behind P_TG_LISTS and P_Z;
// falls in free_targets: with the plan, and with whatever moves the pool's stack below it.
struct TargetsStore {
    DevArena arenaT;                // per leaf Yc | Z, npad x Qpad each (grow-only)
    int tg_Q = 0;                   // columns of the resident Z
    int tg_qpad = 0;                // P_TG_LISTS: the Qpad they were built for
    std::vector<size_t> toff;       // per leaf: offset of its Yc in arenaT
    DevBuf<long long> d_toff;
    DevBuf<double> d_tY, d_tmean, d_tmll;       // Y (N x Q), mean and mll (L x Q)
    DevBuf<TargetsFwdTask> tfwd;    // the sweep's tasks, lane after lane: lane q's launch s is entry q * tfwd_steps + s of tfwd_off
    std::vector<int> tfwd_off;      //   (launch 0: Z_0 of every leaf; launch s: block column s - 1)
    int tfwd_steps = 0, tfwd_lanes = 1;
    // dsmgp_mll_columns_gradients: A = L^-T Z per leaf, npad x Qpad at offset toff / 2 of an arena of its own; its task lists are
    // rebuilt per call
    DevArena arenaA;
    DevBuf<TargetsATask> tga;
    DevBuf<GradTaskTg> tgdot;
    DevBuf<FrobTask> tgfrob;
    DevBuf<ArdLinTask> tgquad;
    DevBuf<TargetsArdLinTask> tgardlin;
    DevBuf<double> d_tgw, d_tgpart; // the weights (L x Q); frob | contraction x gstride | 2 L | ArdLinear 2 D per column group | D per leaf
    // dsmgp_loo_columns / dsmgp_loo_columns_gradients: H = K_y^-1 diag(sqrt W), npad^2 per leaf, and U = K_y^-1 (A / d), npad x Qpad
    // at offset toff / 2, in arenas of their own (the rule of arenaA); the lists are rebuilt per call
    DevArena arenaHc, arenaU;
    DevBuf<LooColsTask> lcleaf;
    DevBuf<GinvTask> lcginv;
    DevBuf<LooColsUTask> lcu;
    DevBuf<LooColsRowTask> lcrow;
    DevBuf<GradTaskLc> lcdot;
    DevBuf<ArdLinTask> lcquad;
    DevBuf<LooColsArdLinTask> lcardlin;
    DevBuf<double> d_lcw, d_lcvec, d_lcpart, d_lcout;   // weights (L x Q); [d | sqrt W | 1 / (d sqrt W)] per leaf; partial sums; mu | var | lpd
};
static_assert(std::is_nothrow_move_assignable_v<TargetsStore>, "TargetsStore falls by assignment (reset)");

// KfoldStore.  dsmgp_kfold (kernels_kfold.hpp): arenas and lists of the last call, grow-only, the arenas from the pool when there is
// one; built per call, not part of bytes_needed, behind no product (labels arrive per call, nothing is cached: no row in
// ctx_state.hpp); falls in free_kfold: with the plan, and with whatever moves the pool's stack below it.
struct KfoldStore {
    DevArena arenaKP;               // the packed panels of one label round: mpad x npad per block, the largest round's total
    DevArena arenaKF;               // G_FF, then its factor, mpad^2 per block
    DevArena arenaKD;               // the inverted diagonal blocks, mpad x 128 per block | -I | the panel solves' scratch tiles
    DevArena arenaKX;               // C^-T, mpad^2 per block: only a call that returns variances asks for it
    DevBuf<int32_t> d_kpos;         // the positions of every block
    DevBuf<int> d_kinfo;            // one flag per block
    DevBuf<double> d_kwork;         // w | v of every (leaf, label) task
    DevBuf<double> d_kout;          // mu | var (obs_ptr[L] each) | lpd (L x K)
    DevBuf<KfoldPackTask> kpack;
    DevBuf<KfoldGffTask> kgff;
    DevBuf<KfoldMomTask> kmom;
    DevBuf<TileTask> kupd, ktrsm, kres, ktrsm2, kadd;   // the block steps of the factorisation (chol_blocks)
    DevBuf<DiagTask> kdiag;
    DevBuf<TransTask> kxtrans;      // C^-T: the diagonal tiles, then the sweep's steps
    DevBuf<TileTask> kxupd, kxtrsm;
    double kfold_seconds[4] = {0.0, 0.0, 0.0, 0.0};     // device seconds of the last successful call: L^-T, pack + G_FF, factorisation, moments
};
static_assert(std::is_nothrow_move_assignable_v<KfoldStore>, "KfoldStore falls by assignment (reset)");

// RouteTreeStore.  The model's tree as flat arrays in HBM: the routing of predict runs on the device (dsmgp_set_test_routed).
// Built by dsmgp_set_tree; stands behind P_RTREE; falls in free_tree: a new tree, new training data or a new leaf table.
struct RouteTreeStore {
    RouteTree rtree{};              // the kernel's by-value view of the arrays below
    DevBuf<int8_t> rt_kind;
    DevBuf<int32_t> rt_first, rt_nchild, rt_sdim, rt_leaf;
    DevBuf<double> rt_thr;
    int64_t rtree_nodes = 0;
    int rtree_max_leaf = -1;        // largest local leaf index a region names (checked against the leaf table at routing time)
};
static_assert(std::is_nothrow_move_assignable_v<RouteTreeStore>, "RouteTreeStore falls by assignment (reset)");

// A resident aggregation family (kernels_agg.hpp): the family, its number of rBCM groups and the number of its moment sums
struct AggState {
    int family = -1, G = 0, W = 0;
};

// What lives as long as the context, and the plain numbers that describe a group without falling with it
struct dsmgp_ctx : Validity, PlanStore, TestInputs, TestProducts, GradLists, GradStore, TargetsStore, KfoldStore, RouteTreeStore {
    // `valid`: what is current (ctx_state.hpp).  HOW a product was made is a plain member:
    bool vt_from_fit = false;       // P_VT: the rows rode through the fit (else: the standalone sweep of predict_run made it)
    bool last_fit_joint = false;    // P_FIT: it carried the resident test rows
    bool grad_lists_all = false;    // P_GRAD_LISTS: they invert every factor owner (build_grad_plan)
    bool grad_all_owners = false;   // P_GRAD_LISTS while build_grad_plan runs: every owner whatever the mask says (xinv_lists)
    bool use_graph = false;         // P_FIT is replayed from a captured graph: opt-in (DSMGP_OPT_FIT_GRAPH), config 2 2.50 -> 2.47 ms, nothing
                                    // elsewhere; capture does not mix with several contexts driven from concurrent host threads (MultiContext)
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    int profile = 0;                // 0: totals only, 1: events around the update launches (dominant kernel), 2: every category
    bool alt_names = false;         // launches under the instantiation names of profile 0 whatever the level (dsmgp_set_profile 3)

    int64_t N = 0;
    int D = 0;
    DevBuf<double> dX, dy;

    int L = 0;
    std::vector<LeafHost> leaves;
    std::vector<int64_t> obs_ptr, obs_idx;
    DevBuf<int64_t> d_obs_ptr, d_obs_idx;

    std::vector<HyperHost> hyper;
    DevBuf<KParam> d_kp;
    DevBuf<double> d_l2;

    std::vector<LeafDev> h_leaves;  // the host's copy of PlanStore::d_leaves
    size_t bytes_needed = 0;

    int fuse_gram = 1;              // update tasks of fit! evaluate the Gram values of their tile themselves (TileTask.gram)
    int fuse_steps = 1;             // block steps with more diagonal blocks than CUs run as two fused launches (kernels_fused.hpp)
    int diag_in_update = 1;         // classic steps: the diagonal tile's update runs one step ahead and its factorisation rides in
                                    // the update launch (DiagFinishTask, kernels_fused.hpp)
    // per phase and block step (PlanStore::fused_step, decided by build_plan):
    //   STEP_CLASSIC    update (all tiles, split-K) / reduce / diagonal block / panel solve launches, one after the other
    //   STEP_FUSED      many leaves: diag_fused_reg_kernel, then tile_fused8_kernel, from the kernel function (kernels_fused.hpp)
    // (A third, lookahead schedule -- the update of step k cut at its last block column, the bulk on this stream, the rank-128
    // finish + diagonal block + solve on a second, high-priority stream beside the bulk of step k + 1 -- was built in round 3
    // and measured in every regime it was meant for: headline 0.4037 / 0.4055 s against 0.3906 / 0.3992, config 2 3.51 against
    // 3.35 ms, 8-rank shards 0.0571 / 0.0569 / 0.0568 / 0.0572 against 0.0577 / 0.0575 / 0.0574 / 0.0575, a 4-rank shard 0.1089 /
    // 0.1082 against 0.1054 / 0.1053.  Removed in round 4; the numbers are in DESIGN.md section 8d.)
    // (Round 4 also built the whole classic step as ONE launch -- diagonal blocks ahead and first in the grid, tile tasks that
    // update from the kernel function, wait inside the launch for their leaf's flag, solve from their registers and write once,
    // K-pieces of split tiles meeting at a ticket -- commit 9fc7be2, parity-green, and measured slower everywhere: headline
    // 0.3947 -> 0.4096 s, 8-rank shard 0.0562 -> 0.0645, config 2 2.51 -> 4.40 ms (profiles/r04_one_launch_ab.log): the last
    // piece to arrive sums up to 46 slabs alone where the reduce launch spreads a tile over 8 workgroups, and the row-split
    // main loop the in-register solve needs runs 5-10 % behind the 2 x 2 one at K >= 2000.  Removed again.)
    // Leaf lanes (round 5, DSMGP_OPT_LANES): the leaves of a table are dealt to one or two LANES (longest-processing-time on n^3,
    // sharing groups together); every lane has step lists and a split-K workspace of its own and runs them on a stream of its
    // own, joined at the end of fit!.  One lane's latency-bound launches (diagonal blocks, panel solves, split-K reduces) then
    // run under the other's update launches -- what several contexts per GPU bought (hipabi.MultiContext: headline -1.4 %, depth
    // 4 -3..-4 %) without a second copy of X, a second plan or host threads.  Per-leaf results do not depend on the lane.
    int lanes_opt = 0;              // 0 = automatic, 1 .. MAX_LANES
    int nlanes = 1;                 // lanes of the current plan
    hipStream_t lane_stream[MAX_LANES] = {};           // [0] = stream
    hipEvent_t ev_fork = nullptr, ev_join[MAX_LANES] = {};
    // Optional device pool (dsmgp_reserve): the large arenas are carved out of one allocation made once, in stack
    // order plan < test < gradients, instead of hipMalloc/hipFree per leaf table -- the driver clears memory on
    // allocation (5 s per 230 GB group measured), which dominated the streaming mode's wall time.
    DevPool pool;
    double alg_flops_joint = 0.0;
    bool joint = true;              // fit advances the resident test rows too
    int ncu = 256;
    bool xcd_order = true;          // XCD-aware task order (speed only)
    int tail_split = DSMGP_TAIL_SPLIT_DEFAULT, tail_rounds = DSMGP_TAIL_ROUNDS_DEFAULT;          // plans with one lane
    int tail_split_lanes = DSMGP_TAIL_SPLIT_LANES, tail_rounds_lanes = DSMGP_TAIL_ROUNDS_LANES;  // plans with two or more
    int ragged_rounds = 2, ragged_div = 4;   // UpdateSplitter::add_step_ragged (launches of the gradient pass)
    // The launch sequence of fit! as a captured hipGraph (one per variant: fit alone / with the resident test rows), replayed
    // while per-launch timing is off (dsmgp_set_profile 0): every kernel argument is a pointer into the plan's task lists or
    // arenas, which live as long as the plan, and the hyper-parameters go through d_kp's CONTENTS -- so a graph stays valid
    // until the plan, the test set or the KParam table's allocation changes (drop_graphs).  What it buys is the host-side
    // launch cost between dependent kernels of a latency-bound chain (config 2: 32 steps x 3 launches).
    hipGraphExec_t fit_graph[2] = {nullptr, nullptr};
    int graph_launches[2][2] = {{0, 0}, {0, 0}};

    // prediction: the counts of the registered test set (TestInputs, TestProducts).  They stay when free_test_products(c, true)
    // empties what was made from the set: dsmgp_add_rows_keep_test registers the same set again on the grown plan
    int64_t n_t = 0;
    std::vector<int64_t> route_ptr;
    int64_t route_total = 0;
    size_t acc_off = 0, acc_count = 0;      // the accumulators' part of arenaPV (register_test)
    AggState agg;       // P_PARTIAL: what d_agg_part holds (dsmgp_aggregate_partial)
    AggState col;       // P_CDONE: the family of the last dsmgp_aggregate_columns
    // pinned host staging for the uploads of a registration (stage_upload): the lists of a test set are ~10 MB at the headline
    // model; through hipMemcpy from pageable vectors they took 9 ms of a 25 ms registration and left the runtime busy behind them
    char* stage = nullptr;
    size_t stage_cap = 0, stage_top = 0;

    // gradients: the inputs, and what build_grad_plan writes for other readers than its own pass (dsmgp_loo, dsmgp_loo_gradients and
    // the column passes read both as well: they do not fall with GradLists)
    std::vector<char> grad_active;  // dsmgp_set_gradient_leaves: leaves whose gradients are wanted (empty = all)
    bool ard_true_gradient = false; // DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT
    std::vector<int> grad_src;      // per leaf: the leaf whose contraction it shares (COPY leaf with the same mean), or -1
    std::vector<size_t> gxoff;      // per owner leaf: its offset in arenaX (build_grad_plan)

    // multi-GPU exchange over RCCL (dsmgp_comm_*, dsmgp_allgather): librccl.so is loaded on first use
    void* comm = nullptr;           // ncclComm_t
    int comm_rank = 0, comm_world = 1;
    DevBuf<double> d_xchg;          // send | recv staging
    // routing workspace, kept across registrations: row counts | leaf counts | outside flag, bitmap, word prefixes
    DevBuf<int32_t> rws_counts;
    DevBuf<uint32_t> rws_bits;
    hipStream_t side = nullptr;     // clock sampler (dsmgp_clock_sample_*): a one-wave kernel beside the context's own launches
    DevBuf<unsigned long long> d_clock;
    bool clock_pending = false;
    double timings[DSMGP_N_TIMINGS] = {0};
    std::vector<hipEvent_t> event_pool;   // PhaseTimer's events, reused across calls
    double alg_flops_update = 0.0;  // algorithmic flops of the Cholesky update launches
    int64_t append_stats[DSMGP_N_APPEND_STATS] = {0, 0, 0, 0, 0, 0};
    bool have_append_stats = false;
    // dsmgp_add_rows_keep_test: plain per-leaf data beside the validity table.  vt_first[l] leading block columns of leaf l's part of
    // arenaVt hold K_tn L^-T of the CURRENT fit although P_VT is not current: it means something only while P_TEST is current,
    // P_VT is not and TestProducts::resume_armed says that the fit is still the one the call made (dsmgp_fit and the predict_run
    // that uses it clear it; so does whatever drops or replaces the test set)
    std::vector<int> vt_first;
    int64_t resume_stats[DSMGP_N_RESUME_STATS] = {0, 0, 0, -1, 0, 0};
    bool have_resume_stats = false;
    double alg_flops_fused = 0.0, alg_flops_fused_joint = 0.0;   // ... of the fused tile launches (update + solve), fit alone / joint
    int n_fused_launches = 0;
    int n_update_launches = 0;
};

namespace {

#define HIPCHK(ctx, call)                                                                        \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return (e_ == hipErrorOutOfMemory) ? DSMGP_E_NOMEM : DSMGP_E_HIP;                    \
        }                                                                                        \
    } while (0)

int fail(dsmgp_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_error = msg;
    return code;
}

template <class T>
int DevBuf<T>::grow(dsmgp_ctx* c, size_t need, size_t want) {
    count = 0;
    if (!p || need > cap) {
        const hipError_t e = p ? hipFree(p) : hipSuccess;
        p = nullptr;
        cap = 0;
        HIPCHK(c, e);
        HIPCHK(c, hipMalloc(&p, want * sizeof(T)));
        cap = want;
    }
    count = need;
    return 0;
}
// `count` entries for a task list: the allocation is kept while the new list fits (a test set that replaces another, a
// gradient mask that changes: hipFree + hipMalloc per list and registration were 3-4 ms of a 16 ms predict at depth 4)
template <class T>
int dev_reserve(dsmgp_ctx* ctx, DevBuf<T>& buf, size_t count) {
    buf.clear();
    return count ? buf.grow(ctx, count) : 0;
}
int copy_upload(dsmgp_ctx* ctx, void* dst, const void* src, size_t bytes) {     // synchronous, from pageable memory
    if (bytes) HIPCHK(ctx, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    return 0;
}
template <class T>
int dev_upload(dsmgp_ctx* ctx, DevBuf<T>& buf, const std::vector<T>& host) {
    if (int rc = dev_reserve(ctx, buf, host.size())) return rc;
    return copy_upload(ctx, buf.p, host.data(), host.size() * sizeof(T));
}

// `bytes` from host memory to the device through the context's PINNED staging buffer, asynchronously on the context's stream: the
// caller's memory is free again on return, the copy is done once the stream is synchronised (stage_done, which every user calls
// before it returns).  Grows on demand; growing waits for the copies in flight.
int stage_upload(dsmgp_ctx* c, void* dst, const void* src, size_t bytes) {
    if (bytes == 0) return 0;
    const size_t at = (c->stage_top + 63) & ~size_t(63);
    if (at + bytes > c->stage_cap) {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->stage) (void)hipHostFree(c->stage);
        c->stage = nullptr;
        c->stage_cap = 0;
        c->stage_top = 0;
        const size_t want = std::max<size_t>(size_t(8) << 20, 2 * (at + bytes));
        HIPCHK(c, hipHostMalloc(reinterpret_cast<void**>(&c->stage), want, hipHostMallocDefault));
        c->stage_cap = want;
        return stage_upload(c, dst, src, bytes);
    }
    std::memcpy(c->stage + at, src, bytes);
    c->stage_top = at + bytes;
    HIPCHK(c, hipMemcpyAsync(dst, c->stage + at, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}
int stage_done(dsmgp_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->stage_top = 0;
    return 0;
}
template <class T>
int stage_upload_list(dsmgp_ctx* c, DevBuf<T>& buf, const std::vector<T>& host) {     // dev_upload through the staging buffer
    if (int rc = dev_reserve(c, buf, host.size())) return rc;
    return stage_upload(c, buf.p, host.data(), host.size() * sizeof(T));
}

// Where the large arenas come from: the reserved pool when there is one, else (null) allocations of their own
DevPool* arena_pool(dsmgp_ctx* c) { return c->pool.active() ? &c->pool : nullptr; }
// What DevArena::get / grow / fit / exact answered, as the library's error code with the text in c->err
int arena_status(dsmgp_ctx* c, int status) {
    if (status == 0) return 0;
    if (status == dev_owner::POOL_FULL)
        return fail(c, DSMGP_E_NOMEM, "reserved device pool too small: need " + std::to_string(c->pool.need >> 20) +
                                          " MiB, pool has " + std::to_string(c->pool.cap >> 20) + " MiB");
    const hipError_t e = (hipError_t)status;
    return fail(c, e == hipErrorOutOfMemory ? DSMGP_E_NOMEM : DSMGP_E_HIP, std::string("hipMalloc of an arena: ") + hipGetErrorString(e));
}

// An UpdateSplitter with the context's scheduling settings for a plan of `nl` lanes
UpdateSplitter make_splitter(const dsmgp_ctx* c, int nl) {
    UpdateSplitter U;
    U.ncu = c->ncu;
    U.xcd = c->xcd_order;
    U.tail_split = nl > 1 ? c->tail_split_lanes : c->tail_split;
    U.tail_rounds = nl > 1 ? c->tail_rounds_lanes : c->tail_rounds;
    U.ragged_rounds = c->ragged_rounds;      // (0 / 1 / 2 rounds cut under lanes: no difference, profiles/r05_grad_lanes_ab.log)
    U.ragged_div = c->ragged_div;
    return U;
}

std::vector<SweepLane> sweep_lanes(const dsmgp_ctx* c, int nl, int nsteps) {
    std::vector<SweepLane> lanes((size_t)nl);
    for (SweepLane& q : lanes) {
        q.U = make_splitter(c, nl);
        q.upd_at.assign((size_t)nsteps, 0);
        q.red_at.assign((size_t)nsteps, 0);
        q.trsm_at.assign((size_t)nsteps, 0);
    }
    return lanes;
}

// The lanes' lists into S, lane after lane through `put` (stage_upload, or copy_upload): the split-K workspace grows to hold the
// slabs of every lane, each lane's splitter is bound to its part of it, and the offset tables are filled
int pack_sweep(dsmgp_ctx* c, SweepLists& S, std::vector<SweepLane>& lanes, int (*put)(dsmgp_ctx*, void*, const void*, size_t)) {
    const int nl = (int)lanes.size(), nsteps = (int)lanes[0].upd_at.size(), nv = nl * nsteps;
    size_t slabs = 0, nu = 0, nr = 0, nt = 0;
    for (const SweepLane& q : lanes) {
        slabs += q.U.max_slabs;
        nu += q.U.upd.size();
        nr += q.U.red.size();
        nt += q.trsm.size();
    }
    if (int rc = arena_status(c, S.slab.grow(arena_pool(c), slabs * TB * TB))) return rc;
    if (int rc = dev_reserve(c, S.upd, nu)) return rc;
    if (int rc = dev_reserve(c, S.red, nr)) return rc;
    if (int rc = dev_reserve(c, S.trsm, nt)) return rc;
    S.nsteps = nsteps;
    S.nlanes = nl;
    S.upd_off.assign((size_t)nv + 1, 0);
    S.red_off.assign((size_t)nv + 1, 0);
    S.trsm_off.assign((size_t)nv + 1, 0);
    size_t bs = 0;
    int bu = 0, br = 0, bt = 0;
    for (int q = 0; q < nl; ++q) {
        SweepLane& ln = lanes[(size_t)q];
        ln.U.bind(S.slab.p + bs * TB * TB);
        for (int k = 0; k < nsteps; ++k) {
            const size_t v = (size_t)q * (size_t)nsteps + (size_t)k;
            S.upd_off[v] = bu + ln.upd_at[(size_t)k];
            S.red_off[v] = br + ln.red_at[(size_t)k];
            S.trsm_off[v] = bt + ln.trsm_at[(size_t)k];
        }
        if (int rc = put(c, S.upd.p + bu, ln.U.upd.data(), ln.U.upd.size() * sizeof(TileTask))) return rc;
        if (int rc = put(c, S.red.p + br, ln.U.red.data(), ln.U.red.size() * sizeof(ReduceTask))) return rc;
        if (int rc = put(c, S.trsm.p + bt, ln.trsm.data(), ln.trsm.size() * sizeof(TileTask))) return rc;
        bs += ln.U.max_slabs;
        bu += (int)ln.U.upd.size();
        br += (int)ln.U.red.size();
        bt += (int)ln.trsm.size();
    }
    S.upd_off[(size_t)nv] = bu;
    S.red_off[(size_t)nv] = br;
    S.trsm_off[(size_t)nv] = bt;
    return 0;
}

void drop_graphs(dsmgp_ctx* c) {
    for (auto& g : c->fit_graph)
        if (g) {
            (void)hipGraphExecDestroy(g);
            g = nullptr;
        }
}

// The named transitions: each lets its lifetime groups fall (reset<G>, or the group's drop), invalidates the products that stood
// for them and, under a reserved pool, keeps the stack order.  Under a pool put() on a carved arena only forgets it: the stack's
// top moves by pool.reset / reset_to_mark, after everything carved above the new top has been forgotten.
template <class G>
void reset(dsmgp_ctx* c) { static_cast<G&>(*c) = G{}; }

// the task lists of the gradient pass (they depend on the set of active leaves): emptied, their allocations and the L^-T arena stay
void free_grad_lists(dsmgp_ctx* c) {
    c->GradLists::drop(true);
    c->invalidate(P_GRAD_LISTS);
}

void free_grad(dsmgp_ctx* c) {
    c->GradLists::drop(false);
    reset<GradStore>(c);
    c->invalidate(P_GRAD_LISTS | P_XINV | P_LOO_LISTS | P_LG_LISTS);
}

// the resident target columns (dsmgp_solve_targets): they go with the plan -- a new leaf table, new training data, dsmgp_release --
// and, under a reserved pool, with whatever resets the pool's stack below them
void free_targets(dsmgp_ctx* c) {
    reset<TargetsStore>(c);
    c->invalidate(P_TG_LISTS);
    c->tmu.release();       // members of TestProducts, which drops them as well: predict_targets' lists are made from the
    c->d_tmu.release();     // resident columns AND the test set, and go with whichever goes first
}

// the arenas and lists of dsmgp_kfold: they go where the resident target columns go
void free_kfold(dsmgp_ctx* c) { reset<KfoldStore>(c); }

void free_tree(dsmgp_ctx* c) {
    reset<RouteTreeStore>(c);
    c->invalidate(P_RTREE);
}

void free_test(dsmgp_ctx* c, bool keep = false);
void free_plan(dsmgp_ctx* c) {
    drop_graphs(c);
    if (c->pool.active()) {  // stack order: everything above the plan goes with it
        free_test(c);
        c->pool.reset();
    }
    reset<PlanStore>(c);
    free_grad(c);
    free_targets(c);
    free_kfold(c);
    c->invalidate(P_PLAN);
}

// What was made from a registered test set -- its arenas, the sweep's, the joint fit's and the prediction's lists, the aggregation
// buffers -- without the set's inputs (free_test).  keep: every buffer stays allocated for what replaces it (emptied, not freed).
// With a device pool the arenas are carved out of the pool's stack and go with its top, so nothing is kept: the answer is the
// `keep` that held.
bool free_test_products(dsmgp_ctx* c, bool keep) {
    drop_graphs(c);
    if (c->pool.active()) {  // the gradient arenas sit above (or would be clobbered below) the test arenas
        free_grad(c);
        free_targets(c);
        free_kfold(c);
        c->pool.reset_to_mark();
        keep = false;
    }
    c->TestProducts::drop(keep);
    c->invalidate(P_TEST);
    return keep;
}

// The registered test set: what was made from it, and its inputs -- the rows, the route CSR, the row / entry index.  keep: a
// registration that replaces another.
void free_test(dsmgp_ctx* c, bool keep) {
    keep = free_test_products(c, keep);
    c->TestInputs::drop(keep);
}

void free_plan_and_test(dsmgp_ctx* c) {       // new training data, leaf table, sharing schedule, plan option or pool
    free_plan(c);
    free_test(c);     // the task lists of a resident test set point into the plan's arenas: they go with it
}

inline int round_up(int x, int m) { return (x + m - 1) / m * m; }
// TileTask.mrows of a row tile with `valid` data rows: rounded up to the MFMA tile height; 0 = the whole tile
inline int tile_mrows(int valid) {
    const int m = round_up(std::max(0, std::min(TB, valid)), 16);
    return m >= TB ? 0 : std::max(16, m);
}

// What the host needs to know about a kernel kind: one row per DSMGP_KIND_*, indexed by the kind (dsmgp_set_hyper admits no
// other value; a kernel id never set has kind -1 and no row).
struct KindInfo {
    const char* name;
    bool ard;           // one length-scale per input dimension (else one)
    bool iso_matern;    // Matern with one length-scale: D equal per-dimension slots of it
    bool matern;        // device KIND 5
    bool rq;            // device KIND 6 (rational quadratic): per-dimension factors 1 / (2 alpha l_d^2), D slots for the iso kind too
    int n_shape;        // shape parameters between the length-scales and logs in the hyper-vector (rational quadratic: loga)
    bool linear;        // no signal variance: KParam.sigma2 = sigma = 1
    double nh_num;      // numerator of the per-dimension factor KParam.nh = nh_num / l^2: -0.5, 1 (ArdLinear) or 2 nu (Matern)
    bool per_dim_grad;  // length-scale gradients from the per-dimension contraction sums Sd (ArdSE: with ard_true_gradient only)
    bool contraction;   // the gradient always contracts (alpha alpha^T - K_y^-1) with dK on the device (tile_graddot*); ArdSE
                        //   with ard_true_gradient only
    bool set_checked;   // dsmgp_set_hyper refuses a wrong number of length-scales itself (the reference kinds: check_hyper, at fit)
    int dot_pass;       // the contraction kernel of the kind's tiles (launch_graddot): 0 tile_graddot_kernel, 1 _prod, 2 _matern, 3 _rq
};
constexpr KindInfo KINDS[] = {
    //  name           ard    iso_m  matern rq     n_shape linear nh_num per_dim contr. set_checked dot_pass
    {"IsoSE",          false, false, false, false, 0,      false, -0.5,  false,  true,  false, 0},
    {"ArdSE",          true,  false, false, false, 0,      false, -0.5,  true,   false, false, 0},
    {"IsoLinear",      false, false, false, false, 0,      true,  -0.5,  false,  false, false, 0},
    {"ArdLinear",      true,  false, false, false, 0,      true,  1.0,   false,  false, false, 0},
    {"ArdSEProduct",   true,  false, false, false, 0,      false, -0.5,  true,   true,  true,  1},
    {"IsoMatern32",    false, true,  true,  false, 0,      false, 3.0,   true,   true,  true,  2},
    {"IsoMatern52",    false, true,  true,  false, 0,      false, 5.0,   true,   true,  true,  2},
    {"ArdMatern32",    true,  false, true,  false, 0,      false, 3.0,   true,   true,  true,  2},
    {"ArdMatern52",    true,  false, true,  false, 0,      false, 5.0,   true,   true,  true,  2},
    // rational quadratic: iso_m = D equal slots for the iso kind; nh_num is 0.5 / alpha, made in upload_hyper
    {"IsoRQ",          false, true,  false, true,  1,      false, 0.0,   true,   true,  true,  3},
    {"ArdRQ",          true,  false, false, true,  1,      false, 0.0,   true,   true,  true,  3},
};
static_assert(sizeof(KINDS) / sizeof(KINDS[0]) == DSMGP_KIND_ARD_RQ + 1, "one row per DSMGP_KIND_*");
// length-scales of a hyper-vector of n values: [logl..., shape..., logs, logNoise]
inline int n_lengthscales(int kind, size_t n) { return (int)n - 2 - KINDS[kind].n_shape; }

// some kernel id has a Matern kind: the fused steps launch diag_fused_reg_matern_kernel as well
inline bool any_matern(const dsmgp_ctx* c) {
    for (const HyperHost& h : c->hyper)
        if (h.kind >= 0 && KINDS[h.kind].matern) return true;
    return false;
}
// some kernel id has a rational quadratic kind: the fused steps launch diag_fused_reg_rq_kernel as well, and a contraction task
// has one more sum (dK / dlog alpha)
inline bool any_rq(const dsmgp_ctx* c) {
    for (const HyperHost& h : c->hyper)
        if (h.kind >= 0 && KINDS[h.kind].rq) return true;
    return false;
}

// Upload the KParam table from the host hyper-parameters.
int upload_hyper(dsmgp_ctx* c) {
    const int nk = (int)c->hyper.size();
    std::vector<double> l2pool, slot_num;
    std::vector<KParam> kp(nk);
    std::vector<size_t> off(nk);
    for (int k = 0; k < nk; ++k) {
        const HyperHost& h = c->hyper[k];
        off[k] = l2pool.size();
        if (h.kind < 0) {   // id never set: no leaf may use it (check_hyper)
            kp[k] = KParam{0, 0, 1.0, 1.0, 1.0, nullptr, nullptr, 0.0, 1.0};
            continue;
        }
        const int nl = n_lengthscales(h.kind, h.loghyp.size());
        off[k] = l2pool.size();
        for (int i = 0; i < nl; ++i) {
            const double l = std::exp(h.loghyp[i]);
            l2pool.push_back(l * l);
        }
        const KindInfo& ki = KINDS[h.kind];
        // an iso Matern / rational quadratic id reads D per-dimension factors like its ARD kind: D slots of its one length-scale
        if (ki.iso_matern)
            for (int i = 1; i < c->D; ++i) l2pool.push_back(l2pool[off[k]]);
        // rational quadratic: nh = 1 / (2 alpha l^2), alpha = exp(loga) from the shape slot behind the length-scales
        const double alpha = ki.rq ? std::exp(h.loghyp[nl]) : 0.0;
        slot_num.resize(l2pool.size(), ki.rq ? 0.5 / alpha : ki.nh_num);
        kp[k].kind = h.kind;
        kp[k].nl = nl;
        kp[k].il2 = alpha;      // (every other kind: 1 / l2[0], below)
        const double logs = h.loghyp[nl + ki.n_shape];
        const double logn = h.loghyp[nl + ki.n_shape + 1];
        kp[k].sigma2 = ki.linear ? 1.0 : std::exp(2.0 * logs);
        kp[k].sigma = ki.linear ? 1.0 : std::exp(logs);
        kp[k].noise = std::exp(2.0 * logn);
    }
    const size_t nslots = l2pool.size();
    // second half (KParam.nh): the per-dimension factor -- of the exponent, -0.5 / l^2, of ArdLinear's product, 1 / l_d^2, or
    // of a Matern kernel's s^2, 2 nu / l_d^2, or of a rational quadratic kernel's w, 1 / (2 alpha l_d^2)
    for (size_t i = 0; i < nslots; ++i) l2pool.push_back(slot_num[i] / l2pool[i]);
    if (l2pool.size() > c->d_l2.cap || !c->d_l2.p) {   // (re)allocate only when the table grows: fit is called in loops
        drop_graphs(c);
        if (int rc = c->d_l2.grow(c, l2pool.size(), std::max<size_t>(16, 2 * l2pool.size()))) return rc;
    }
    if ((size_t)nk > c->d_kp.cap || !c->d_kp.p) {
        drop_graphs(c);
        if (int rc = c->d_kp.grow(c, (size_t)nk, std::max<size_t>(4, 2 * (size_t)nk))) return rc;
    }
    HIPCHK(c, hipMemcpyAsync(c->d_l2.p, l2pool.data(), l2pool.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int k = 0; k < nk; ++k) {
        kp[k].l2 = c->d_l2.p + off[k];
        kp[k].nh = c->d_l2.p + nslots + off[k];
        if (c->hyper[k].kind >= 0) {
            kp[k].nh0 = l2pool[nslots + off[k]];
            if (!KINDS[c->hyper[k].kind].rq) kp[k].il2 = 1.0 / l2pool[off[k]];
        }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_kp.p, kp.data(), nk * sizeof(KParam), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // l2pool / kp are stack storage
    return 0;
}

// an ARD kernel id reads D per-dimension factors wherever its kernel function is evaluated (the additive ArdSE is left to
// check_hyper here, as it has been since this check came in with ArdLinear)
bool ard_linear_short(const dsmgp_ctx* c, int kid) {
    const HyperHost& h = c->hyper[kid];
    return KINDS[h.kind].ard && h.kind != DSMGP_KIND_ARD_SE && n_lengthscales(h.kind, h.loghyp.size()) != c->D;
}

int check_hyper(dsmgp_ctx* c) {
    for (int l = 0; l < c->L; ++l) {
        const int kid = c->leaves[l].kid;
        if (kid < 0 || kid >= (int)c->hyper.size() || c->hyper[kid].kind < 0)
            return fail(c, DSMGP_E_STATE, "leaf " + std::to_string(l) + " uses kernel id " + std::to_string(kid) +
                                              " without hyper-parameters");
        const HyperHost& h = c->hyper[kid];
        const int nl = n_lengthscales(h.kind, h.loghyp.size());
        const bool ard = KINDS[h.kind].ard;
        if (ard && nl != c->D)
            return fail(c, DSMGP_E_ARG, std::string(KINDS[h.kind].name) + " needs one lengthscale per input dimension");
        if (!ard && nl != 1) return fail(c, DSMGP_E_ARG, "Iso kernels take one lengthscale");
    }
    return 0;
}

// Algorithmic flops of the left-looking update of a leaf of (unpadded) size n: for every block column k,
// 2*K flops (K = 128k) per lower-triangle element of that block column.
// A PREFIX leaf keeps the leading kb x kb blocks of its source: in block columns k < kb only the rows >= 128 kb are
// updated (they are the launches of build_factor_steps), the copied part costs nothing.
template <class Depth>
double update_flops(int n, int kb, Depth depth /* block step -> blocks of K the timed launch covers */) {
    double f = 0.0;
    for (int k = 1; k * TB < n; ++k) {
        const int c0 = k * TB, c1 = std::min(n, c0 + TB);
        double elems = 0.0;
        if (k < kb) elems = (double)(c1 - c0) * (double)std::max(0, n - kb * TB);
        else
            for (int c = c0; c < c1; ++c) elems += (double)(n - c);
        f += 2.0 * (double)(depth(k) * TB) * elems;
    }
    return f;
}

// Per-leaf algorithmic flops of the test rows riding through the sweep: 2*K per (test row, column) element.
template <class Depth>
double predict_update_flops(int n, int nt, Depth depth) {
    double f = 0.0;
    for (int k = 1; k * TB < n; ++k) f += 2.0 * (double)(depth(k) * TB) * (double)nt * (double)std::min(TB, n - k * TB);
    return f;
}

// Gram values evaluated by the update tasks themselves (TileTask.gram) instead of written by the Gram launch and read
// back: needs the coordinate image of a tile to fit the kernel's LDS ring.
bool gram_fused(const dsmgp_ctx* c) { return c->fuse_gram && c->D <= GRAM_FUSE_MAX_D; }

// The 16-row blocks of one leaf below the diagonal block of step k -> fused tile tasks of eight (tile_fused8_kernel): all of
// them read the leaf's B panel F[k, 0:K], L_kk behind it and the coordinates of the block's columns.  Empties `blocks`.
void push_fused8_tasks(std::vector<FusedTask8>& out, std::vector<RowBlock>& blocks, const LeafDev& d, const LeafHost& lf, int k) {
    for (size_t b0 = 0; b0 < blocks.size(); b0 += 8) {
        FusedTask8 f{};
        f.B = d.F + (size_t)k * TB;
        f.Dinv = d.Dinv + (size_t)k * TB * TB;
        f.gxb = d.Xg + (size_t)k * TB;
        f.ldb = f.gldb = lf.npad;
        f.gnb = std::max(0, std::min(TB, lf.n - k * TB));
        f.k1 = k * TB;
        f.kid = lf.kid;
        f.nblk = (int)std::min<size_t>(8, blocks.size() - b0);
        for (int q = 0; q < f.nblk; ++q) {
            f.rb[q] = blocks[b0 + q];
            if (f.rb[q].wi != nullptr) f.zk = d.z + (size_t)k * TB;     // riders read z_k
        }
        out.push_back(f);
    }
    blocks.clear();
}

// Step lists of the batched left-looking factorisation.  phase[0]: leaves factorised in full (and, with
// `with_test`, the test rows of those leaves and of the COPY leaves that alias them); phase[1]: PREFIX leaves.
// with_test: the rows of K_tn (Vt) of every leaf are appended below its factor and advance through the same
// update / panel-solve launches -- prediction's triangular solves (src/gaussianprocess.jl:120) cost no launches
// of their own when the test set is resident at fit time.
int build_factor_steps(dsmgp_ctx* c, int lane, bool with_test, StepLists (&phase)[2], DevArena& slab_ws, double& alg_flops,
                       double& alg_flops_fused, bool slab_outside_pool = false) {
    const int L = c->L;
    alg_flops = 0.0;
    const bool fused = gram_fused(c);
    UpdateSplitter split[2] = {make_splitter(c, c->nlanes), make_splitter(c, c->nlanes)};
    for (int ph = 0; ph < 2; ++ph) {
        StepLists& S = phase[ph];
        UpdateSplitter& U = split[ph];
        auto in_phase = [&](const LeafHost& lf) {
            const size_t l = (size_t)(&lf - c->leaves.data());
            return c->leaf_group[l] == ph && c->leaf_lane[l] == lane;
        };
        int nsteps = 0;
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (!in_phase(lf)) continue;
            if (lf.owner == l || (with_test && lf.nt > 0)) nsteps = std::max(nsteps, lf.nb);
        }
        S.nsteps = nsteps;
        std::vector<TileTask> trsm;
        std::vector<DiagTask> diag;
        std::vector<FusedTask8> ftile8;
        std::vector<RowBlock> blocks8;      // 16-row blocks of one leaf below the step's diagonal block: factor rows, then test rows
        std::vector<DiagFusedTask> fdiag;
        std::vector<DiagFinishTask> dfin;
        S.dpos.assign(nsteps, 0);
        S.dfin_off.assign(nsteps + 1, 0);
        S.upd_off.assign(nsteps + 1, 0);
        S.red_off.assign(nsteps + 1, 0);
        S.trsm_off.assign(nsteps + 1, 0);
        S.diag_off.assign(nsteps + 1, 0);
        S.fdiag_off.assign(nsteps + 1, 0);
        S.ftile8_off.assign(nsteps + 1, 0);
        S.step_tiles.assign(nsteps, 0);
        S.pad.assign(nsteps, 0);
        S.mode.assign(nsteps, STEP_CLASSIC);
        for (int k = 0; k < nsteps; ++k) {
            S.upd_off[k] = (int)U.upd.size();
            S.red_off[k] = (int)U.red.size();
            S.trsm_off[k] = (int)trsm.size();
            S.diag_off[k] = (int)diag.size();
            S.fdiag_off[k] = (int)fdiag.size();
            S.ftile8_off[k] = (int)ftile8.size();
            S.dfin_off[k] = (int)dfin.size();
            const int mode = k < (int)c->fused_step[ph].size() ? c->fused_step[ph][k] : STEP_CLASSIC;
            S.mode[k] = (char)mode;
            const bool fstep = mode != STEP_CLASSIC;               // diagonal blocks and tiles below go through the fused kernels
            std::vector<TileTask> tiles;
            // One-step lookahead of the diagonal blocks (DiagFinishTask): where steps k-1 and k are both classic, the update
            // launch of step k-1 has left tile (k,k) = K(k,k) - F[k,0:K-128] F[k,0:K-128]^T (`ahead` below, one step on), and
            // the diagonal-block task of step k -- rank-128 finish + factorisation -- rides in the update launch of step k.
            auto classic_at = [&](int q) {
                return q >= 0 && q < nsteps && (q >= (int)c->fused_step[ph].size() || c->fused_step[ph][q] == STEP_CLASSIC);
            };
            const bool finish_here = c->diag_in_update && gram_fused(c) && !fstep && k >= 2 && classic_at(k - 1);
            const bool ahead = c->diag_in_update && gram_fused(c) && !fstep && k >= 1 && classic_at(k + 1);
            size_t nsym = 0;
            for (int l = 0; l < L; ++l) {
                const LeafHost& lf = c->leaves[l];
                if (lf.nb <= k || !in_phase(lf)) continue;
                const LeafDev& d = c->h_leaves[l];
                const int ld = lf.npad;
                if (lf.owner == l) {
                    // a PREFIX leaf keeps the copied leading kb x kb blocks: for k < kb only rows >= kb are new
                    const int i_first = (k < lf.kb) ? lf.kb : k;
                    const bool own_diag = (k >= lf.kb);
                    const bool fin = finish_here && own_diag;    // tile (k,k) got all but its last block column one step ago
                    for (int i = i_first; i < lf.nb; ++i) {
                        if (fstep) {      // fused step: the diagonal tile belongs to the diagonal-block task; of the tiles below
                                          // the 16-row blocks that hold data are updated and solved, eight to a task (the rows
                                          // beyond stay zero: zero_pad_rows_kernel)
                            if (i == k) continue;
                            const int rows = std::max(0, std::min(TB, lf.n - i * TB));
                            for (int r = 0; r < rows; r += 16) {
                                RowBlock b{};
                                b.A = d.F + (size_t)i * TB + r;
                                b.C = d.F + (size_t)i * TB + r + (size_t)k * TB * ld;
                                b.gx = d.Xg + (size_t)i * TB + r;
                                b.lda = b.ldc = b.glda = ld;
                                b.nvalid = std::min(16, rows - r);
                                if (ph != 1) b.wi = d.w + (size_t)i * TB + r;     // fused forward substitution
                                blocks8.push_back(b);
                            }
                            continue;
                        }
                        if (k > 0 && !(i == k && fin)) {
                            TileTask u{};
                            u.A = d.F + (size_t)i * TB;
                            u.B = d.F + (size_t)k * TB;
                            u.C = d.F + (size_t)i * TB + (size_t)k * TB * ld;
                            u.lda = u.ldb = u.ldc = ld;
                            u.k0 = 0;
                            u.k1 = k * TB;
                            u.update = 1;
                            u.mrows = tile_mrows(lf.n - i * TB);
                            u.sym = (i == k) ? 1 : 0;   // diagonal tile: A == B, lower blocks only
                            nsym += (size_t)u.sym;
                            if (fused) {
                                u.gram = 1 | (i == k ? 2 : 0) | 4;   // bit 2: a tile of the factor is first written here, padding rows too
                                u.kid = lf.kid;
                                u.gxa = d.Xg + (size_t)i * TB;
                                u.gxb = d.Xg + (size_t)k * TB;
                                u.glda = u.gldb = ld;
                                u.gna = std::max(0, std::min(TB, lf.n - i * TB));
                                u.gnb = std::max(0, std::min(TB, lf.n - k * TB));
                            }
                            tiles.push_back(u);
                        }
                        if (i == k + 1 && ahead && k + 1 >= lf.kb) {
                            // the NEXT step's diagonal tile over the columns this step's tiles cover: same depth, the A panel
                            // of the tile (k+1, k) beside it; its last block column and its factorisation follow in the
                            // DiagFinishTask of the next update launch
                            TileTask u{};
                            u.A = u.B = d.F + (size_t)i * TB;
                            u.C = d.F + (size_t)i * TB + (size_t)i * TB * ld;
                            u.lda = u.ldb = u.ldc = ld;
                            u.k0 = 0;
                            u.k1 = k * TB;
                            u.update = 1;
                            u.mrows = tile_mrows(lf.n - i * TB);
                            u.sym = 1;
                            nsym += 1;
                            u.gram = 1 | 2 | 4;
                            u.kid = lf.kid;
                            u.gxa = u.gxb = d.Xg + (size_t)i * TB;
                            u.glda = u.gldb = ld;
                            u.gna = u.gnb = std::max(0, std::min(TB, lf.n - i * TB));
                            tiles.push_back(u);
                        }
                        if (i > k) {
                            TileTask s{};
                            s.A = d.F + (size_t)i * TB + (size_t)k * TB * ld;
                            s.B = d.Dinv + (size_t)k * TB * TB;
                            s.C = const_cast<double*>(s.A);
                            s.lda = ld;
                            s.ldb = TB;
                            s.ldc = ld;
                            s.k0 = 0;
                            s.k1 = TB;
                            s.update = 0;
                            s.mrows = tile_mrows(lf.n - i * TB);
                            if (ph != 1) {   // fused forward substitution for leaves factorised in full
                                s.zk = d.z + (size_t)k * TB;
                                s.wi = d.w + (size_t)i * TB;
                            }
                            trsm.push_back(s);
                        }
                    }
                    if (own_diag) {
                        DiagTask g{};
                        g.T = d.F + (size_t)k * TB + (size_t)k * TB * ld;
                        g.Dinv = d.Dinv + (size_t)k * TB * TB;
                        if (ph != 1) {
                            g.wk = d.w + (size_t)k * TB;
                            g.zk = d.z + (size_t)k * TB;
                        }
                        g.info = d.info;
                        g.ld = ld;
                        g.nvalid = std::max(0, std::min(TB, lf.n - k * TB));
                        g.row0 = k * TB;
                        if (fstep) {
                            DiagFusedTask fg{};
                            fg.d = g;
                            fg.A = d.F + (size_t)k * TB;
                            fg.gx = d.Xg + (size_t)k * TB;
                            fg.k1 = k * TB;
                            fg.glda = ld;
                            fg.kid = lf.kid;
                            fdiag.push_back(fg);
                        } else if (fin) {
                            DiagFinishTask ft{};
                            ft.d = g;
                            ft.A = d.F + (size_t)k * TB + (size_t)(k - 1) * TB * ld;
                            dfin.push_back(ft);
                        } else {
                            diag.push_back(g);
                        }
                    }
                }
                if (with_test && lf.nt > 0) {
                    for (int ti = 0; ti < lf.ntpad / TB; ++ti) {
                        double* tile = d.Vt + (size_t)ti * TB + (size_t)k * TB * lf.ntpad;
                        if (fstep) {
                            const int rows = std::max(0, std::min(TB, lf.nt - ti * TB));
                            for (int r = 0; r < rows; r += 16) {
                                RowBlock b{};
                                b.A = d.Vt + (size_t)ti * TB + r;
                                b.C = tile + r;
                                b.gx = d.Xtg + (size_t)ti * TB + r;
                                b.lda = b.ldc = b.glda = lf.ntpad;
                                b.nvalid = std::min(16, rows - r);
                                if (d.zfused) {
                                    b.wi = d.macc + (size_t)ti * TB + r;
                                    b.sq = d.sacc + (size_t)ti * TB + r;
                                }
                                blocks8.push_back(b);
                            }
                            continue;
                        }
                        if (k > 0) {
                            TileTask u{};
                            u.A = d.Vt + (size_t)ti * TB;
                            u.B = d.F + (size_t)k * TB;
                            u.C = tile;
                            u.lda = lf.ntpad;
                            u.ldb = ld;
                            u.ldc = lf.ntpad;
                            u.k0 = 0;
                            u.k1 = k * TB;
                            u.update = 1;
                            u.mrows = tile_mrows(lf.nt - ti * TB);
                            if (fused) {
                                u.gram = 1;
                                u.kid = lf.kid;
                                u.gxa = d.Xtg + (size_t)ti * TB;
                                u.gxb = d.Xg + (size_t)k * TB;
                                u.glda = lf.ntpad;
                                u.gldb = ld;
                                u.gna = std::max(0, std::min(TB, lf.nt - ti * TB));
                                u.gnb = std::max(0, std::min(TB, lf.n - k * TB));
                            }
                            tiles.push_back(u);
                        }
                        TileTask s{};
                        s.A = tile;
                        s.B = d.Dinv + (size_t)k * TB * TB;
                        s.C = tile;
                        s.lda = lf.ntpad;
                        s.ldb = TB;
                        s.ldc = lf.ntpad;
                        s.k0 = 0;
                        s.k1 = TB;
                        s.update = 0;
                        s.mrows = tile_mrows(lf.nt - ti * TB);
                        if (d.zfused) {   // z_k exists by the time this launch runs: accumulate mu and the variance term
                            s.zk = d.z + (size_t)k * TB;
                            s.wi = d.macc + (size_t)ti * TB;
                            s.sq = d.sacc + (size_t)ti * TB;
                        }
                        trsm.push_back(s);
                    }
                }
                // fused tile tasks: the leaf's 16-row blocks of this step, eight to a task (the last factor rows and the test
                // rows share tasks)
                push_fused8_tasks(ftile8, blocks8, d, lf, k);
            }
            // The lower-blocks-only form of a diagonal tile takes ~0.6 of a full tile (tools/bench_tile_sym.py), the column-split
            // form of a short tile (padding rows below: tile_rows_body) its share of rows: together 3.4 % of the headline
            // model's executed flops (full diagonal tiles 1.5 %, the last row tile of every leaf and of its test rows 1.9 %).
            // Until round 5 both forms were kept for launches in which such tiles are a large share (1/5, 1/10: depth 4, -6 %
            // there) -- in launches dominated by full tiles a few shorter tasks measured +1.2 % (round 3, +0.4 % when
            // issued last).  With the schedule as it is now they pay everywhere: headline, same box, four alternating runs,
            // 0.3819 -> 0.3792 s with both (two lanes), 0.3981 -> 0.3951 with one lane; depth 4, configs 2 and 3, the shards of 4- and 8-rank
            // jobs unchanged (profiles/r05_sym_pad_ab.log).
            if (DSMGP_SYM_SHARE > 0 && nsym * DSMGP_SYM_SHARE < tiles.size())
                for (auto& u : tiles) u.sym = 0;
            {   // short tiles: the PAD instantiations of the kernels (step 0 has no update launch: its panel solves decide)
                size_t npad = 0, ntot = tiles.size();
                for (const auto& u : tiles) npad += (u.mrows != 0 && u.mrows <= 96) ? 1 : 0;
                if (tiles.empty()) {
                    ntot = trsm.size() - (size_t)S.trsm_off[k];
                    for (size_t q = (size_t)S.trsm_off[k]; q < trsm.size(); ++q) npad += (trsm[q].mrows != 0 && trsm[q].mrows <= 64) ? 1 : 0;
                }
                const bool share = DSMGP_PAD_SHARE == 0 || npad * (size_t)DSMGP_PAD_SHARE >= ntot;
                // big launches only: the PAD instantiation in EVERY launch leaves the headline, its shards and depth 4 where
                // they are, costs a single GP of 32 blocks 2 % (2.28 -> 2.33 ms) and gives the PoE of 128 experts 2.4 % (4.50 ->
                // 4.39 ms): profiles/r05_sym_pad_ab.log
                S.pad[k] = (npad > 0 && share && ntot >= (size_t)(2 * c->ncu)) ? 1 : 0;
            }
            // (The shorter tasks stay with the tiles of their leaf, whose B panel they share through L2: moved behind the whole
            // tiles of the launch the headline step measures 0.3853 -> 0.3883 s, four alternating runs: profiles/r05_sym_pad_ab.log.)
            U.add_step(tiles, k * TB);
            S.step_tiles[k] = (int)tiles.size();
            // Where the step's diagonal-block tasks sit in its update launch.  They are ~45 us each, and a slot that runs one
            // finishes its share of the launch that much later: in a launch that keeps every workgroup slot busy from start
            // to end (rounds of equal tiles) the launch ends that much later wherever they sit (measured: at the front the
            // update launches of the headline model and of an 8-rank shard grew by 37 and 30 us a step, the diagonal-block
            // launch they replace was 38).  So: a launch that leaves slots idle anyway (fewer tasks than the chip's 2 x CUs
            // workgroup slots) takes them first; a fuller one takes them LAST, behind its tail pieces, where they land in the
            // slots that drain first while the last pieces are still running.
            {
                const int nu_k = (int)U.upd.size() - S.upd_off[k], nd_k = (int)dfin.size() - S.dfin_off[k];
                if (nu_k + nd_k <= 2 * c->ncu) S.dpos[k] = 0;
                else if (DSMGP_DFIN_BACK < 0) S.dpos[k] = nu_k;
                else S.dpos[k] = std::max(0, (int)U.tail_begin - S.upd_off[k] - DSMGP_DFIN_BACK * c->ncu);
            }
            {   // panel solves of a leaf read the same Dinv_k: keep them on one XCD (small leaves have 3-4 of them per
                // step; dealt round-robin every one of them fetched the 128 KB block from HBM on its own: the depth-4
                // model's panel-solve launches fetched 2.6x their tile bytes)
                std::vector<int> unused(trsm.size());
                xcd_permute(trsm, unused, (size_t)S.trsm_off[k], trsm.size(), c->xcd_order);
                std::vector<int> unused3(ftile8.size());     // the fused tile tasks of a leaf share its B panel and L_kk
                xcd_permute(ftile8, unused3, (size_t)S.ftile8_off[k], ftile8.size(), c->xcd_order);
            }
        }
        S.upd_off[nsteps] = (int)U.upd.size();
        S.red_off[nsteps] = (int)U.red.size();
        S.trsm_off[nsteps] = (int)trsm.size();
        S.diag_off[nsteps] = (int)diag.size();
        S.fdiag_off[nsteps] = (int)fdiag.size();
        S.ftile8_off[nsteps] = (int)ftile8.size();
        S.dfin_off[nsteps] = (int)dfin.size();
        if (int rc = dev_upload(c, S.dfin, dfin)) return rc;
        if (int rc = dev_upload(c, S.trsm, trsm)) return rc;
        if (int rc = dev_upload(c, S.diag, diag)) return rc;
        if (int rc = dev_upload(c, S.fdiag, fdiag)) return rc;
        if (int rc = dev_upload(c, S.ftile8, ftile8)) return rc;
    }
    {
        const size_t slabs = std::max(split[0].max_slabs, split[1].max_slabs);
        slab_ws.put();
        if (slabs)
            if (int rc = arena_status(c, slab_ws.get(slab_outside_pool ? nullptr : arena_pool(c), slabs * TB * TB))) return rc;
        for (int ph = 0; ph < 2; ++ph) {
            split[ph].bind(slab_ws.p);
            if (int rc = dev_upload(c, phase[ph].upd, split[ph].upd)) return rc;
            if (int rc = dev_upload(c, phase[ph].red, split[ph].red)) return rc;
        }
        if (std::getenv("DSMGP_HOSTLOG")) {      // how many tiles of the factorisation pass through a split-K reduce before their panel solve
            size_t tiles = 0, panel = 0;
            for (int ph = 0; ph < 2; ++ph) {
                for (int v : phase[ph].step_tiles) tiles += (size_t)v;
                panel += (size_t)phase[ph].trsm_off[phase[ph].nsteps];
            }
            std::fprintf(stderr, "hostlog lane %d: %zu update tiles, %zu of them cut along K (reduce tasks), %zu panel-solve tiles\n", lane, tiles,
                         split[0].red.size() + split[1].red.size(), panel);
        }
    }
    // algorithmic flops of the launches timed as "update" (slot 1: tile_gemm_kernel_v2): 2 K per element of block column k with
    // K = 128 k, nothing where it runs fused.  Fused tile launches (slot 18: tile_fused8_kernel) are counted apart: their update flops
    // plus the triangular solve of the tiles below the diagonal block (c_k^2 per row, c_k = columns of block k).
    alg_flops_fused = 0.0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (c->leaf_lane[l] != lane) continue;
        const std::vector<char>& md = c->fused_step[(int)c->leaf_group[l]];
        auto mode = [&](int k) { return k < (int)md.size() ? (int)md[k] : (int)STEP_CLASSIC; };
        auto depth = [&](int k) { return mode(k) == STEP_FUSED ? 0 : k; };
        auto depth_fused = [&](int k) { return mode(k) == STEP_FUSED ? k : 0; };
        if (lf.owner == l) {
            alg_flops += update_flops(lf.n, lf.kb, depth);
            alg_flops_fused += update_flops(lf.n, lf.kb, depth_fused);
        }
        if (with_test && lf.nt > 0) {
            alg_flops += predict_update_flops(lf.n, lf.nt, depth);
            alg_flops_fused += predict_update_flops(lf.n, lf.nt, depth_fused);
        }
        for (int k = 0; k * TB < lf.n; ++k) {
            if (mode(k) != STEP_FUSED) continue;
            const double ck = (double)std::min(TB, lf.n - k * TB);
            if (lf.owner == l) alg_flops_fused += (double)std::max(0, lf.n - std::max(k + 1, lf.kb) * TB) * ck * ck;
            if (with_test && lf.nt > 0) alg_flops_fused += (double)lf.nt * ck * ck;
        }
    }
    return 0;
}

int build_schedule(dsmgp_ctx* c);
int register_test(dsmgp_ctx* c, HostLog& hl, const std::vector<int>* first = nullptr);
int full_sweep_lists(dsmgp_ctx* c);
// Who owns which factor, how many leading blocks a PREFIX leaf keeps, and where every leaf's buffers sit in the plan's arenas
void plan_layout(dsmgp_ctx* c, size_t& fTot, size_t& dTot, size_t& vTot, size_t& xTot) {
    const int L = c->L;
    fTot = dTot = vTot = xTot = 0;
    for (int l = 0; l < L; ++l) {
        LeafHost& lf = c->leaves[l];
        lf.owner = (lf.op == DSMGP_SHARE_COPY) ? lf.src : l;
        lf.kb = (lf.op == DSMGP_SHARE_PREFIX) ? (int)(lf.prefix / TB) : 0;
        if (lf.op == DSMGP_SHARE_PREFIX && lf.kb == 0) {
            lf.op = DSMGP_SHARE_FULL;   // nothing worth copying
            lf.src = -1;
        }
    }
    for (int l = 0; l < L; ++l) {
        LeafHost& lf = c->leaves[l];
        if (lf.owner == l) {
            lf.f_off = fTot;
            fTot += (size_t)lf.npad * lf.npad;
            lf.dinv_off = dTot;
            dTot += (size_t)lf.nb * TB * TB;
        }
        lf.vec_off = vTot;
        vTot += (size_t)4 * lf.npad;
        lf.xg_off = xTot;
        xTot += (size_t)lf.npad * c->D;
    }
    for (int l = 0; l < L; ++l) {
        LeafHost& lf = c->leaves[l];
        if (lf.owner != l) {
            lf.f_off = c->leaves[lf.owner].f_off;
            lf.dinv_off = c->leaves[lf.owner].dinv_off;
        }
    }
}

// Build arenas, the LeafDev table and every task list for the current leaf table + sharing schedule, unless they are current.
// adoptF / adoptDinv (dsmgp_append_rows in place): the factor and Dinv arenas of the previous plan, whose layout is this plan's; they
// are moved into c->arenaF / c->arenaDinv instead of new allocations -- the caller's are empty from then on, and its own until then.
int build_plan(dsmgp_ctx* c, DevArena&& adoptF = DevArena(), DevArena&& adoptDinv = DevArena()) {
    if (c->has(P_PLAN)) return 0;
    HostLog hl_total("build_plan");
    {
        HostLog hl("build_plan: free_plan");
        free_plan(c);
    }
    const int L = c->L;
    if (L == 0) return fail(c, DSMGP_E_STATE, "no leaves set");
    size_t fTot = 0, dTot = 0, vTot = 0, xTot = 0;
    plan_layout(c, fTot, dTot, vTot, xTot);
    c->bytes_needed = (fTot + dTot + vTot + xTot) * sizeof(double);
    size_t freeB = 0, totalB = 0;
    HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
    // (dsmgp_append_rows in place: the factor and Dinv arenas of the previous plan are taken over, they are allocated already)
    const bool adopt = adoptF.p != nullptr && adoptDinv.p != nullptr;
    if (!c->pool.active() && c->bytes_needed - (adopt ? (fTot + dTot) * sizeof(double) : 0) + (size_t(1) << 30) > freeB)
        return fail(c, DSMGP_E_NOMEM, "leaf table needs " + std::to_string(c->bytes_needed >> 20) + " MiB, device has " +
                                          std::to_string(freeB >> 20) + " MiB free");
    {
        HostLog hl("build_plan: arenas");
        if (adopt) {
            c->arenaF = std::move(adoptF);
            c->arenaDinv = std::move(adoptDinv);
        } else {
            if (int rc = arena_status(c, c->arenaF.get(arena_pool(c), fTot))) return rc;
            if (int rc = arena_status(c, c->arenaDinv.get(arena_pool(c), dTot))) return rc;
            // the diagonal-block kernel writes the lower blocks of Dinv_k only: the blocks above the diagonal are zero from here on
            HIPCHK(c, hipMemsetAsync(c->arenaDinv.p, 0, std::max<size_t>(1, dTot) * sizeof(double), c->stream));
        }
        if (int rc = arena_status(c, c->arenaVec.get(arena_pool(c), vTot))) return rc;
        if (int rc = arena_status(c, c->arenaXg.get(arena_pool(c), xTot))) return rc;
    }
    if (int rc = c->d_info.alloc(c, L)) return rc;
    if (int rc = c->d_owner.alloc(c, L)) return rc;
    {   // the owner table changes with the leaf table / sharing schedule only: uploaded here, once
        std::vector<int> owner(L);
        for (int l = 0; l < L; ++l) owner[l] = c->leaves[l].owner;
        HIPCHK(c, hipMemcpy(c->d_owner.p, owner.data(), (size_t)L * sizeof(int), hipMemcpyHostToDevice));
    }
    if (int rc = c->d_mll.alloc(c, L)) return rc;
    if (int rc = c->d_leaves.alloc(c, L)) return rc;

    c->h_leaves.assign(L, LeafDev{});
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        LeafDev& d = c->h_leaves[l];
        d.F = c->arenaF.p + lf.f_off;
        d.Dinv = c->arenaDinv.p + lf.dinv_off;
        d.Xg = c->arenaXg.p + lf.xg_off;
        d.yc = c->arenaVec.p + lf.vec_off;
        d.w = d.yc + lf.npad;
        d.z = d.w + lf.npad;
        d.alpha = d.z + lf.npad;
        d.info = c->d_info.p + lf.owner;
        d.mean = lf.mean;
        d.n = lf.n;
        d.npad = lf.npad;
        d.nb = lf.nb;
        d.kid = lf.kid;
    }
    HIPCHK(c, hipMemcpy(c->d_leaves.p, c->h_leaves.data(), L * sizeof(LeafDev), hipMemcpyHostToDevice));

    // gather X rows and centred y of every leaf (replaces the per-leaf views + apply_subtract!,
    // src/gaussianprocess.jl:72-74, src/treeStructure.jl:271-273)
    {
        int maxpad = 0;
        for (auto& lf : c->leaves) maxpad = std::max(maxpad, lf.npad);
        for_leaf_chunks((size_t)L, [&](size_t leaf0, size_t cnt) {
            dim3 grid((maxpad + 255) / 256, (unsigned)cnt);
            gather_leaf_kernel<<<grid, 256, 0, c->stream>>>(c->d_leaves.p, c->d_obs_ptr.p, c->d_obs_idx.p, c->dX.p, c->dy.p,
                                                            c->N, c->D, (int)leaf0);
        });
        HIPCHK(c, hipGetLastError());
    }
    // The eight-wave fused tile tasks write the 16-row blocks of a factor that hold data and nothing else: the rows below them
    // in a leaf's last row tile -- padding, which the classic steps and every sweep over the factor expect to be zero -- are
    // zeroed here, once per plan (nothing writes anything else there afterwards)
    std::vector<ZeroRowsTask> zr;
    if (gram_fused(c)) {
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            const int last = lf.n - (lf.nb - 1) * TB;
            if (lf.owner != l || lf.nb < 2 || last >= TB) continue;
            ZeroRowsTask z{};
            z.p = c->h_leaves[l].F + (size_t)(lf.nb - 1) * TB;
            z.ld = lf.npad;
            z.r0 = (std::max(0, last) + 15) / 16 * 16;
            z.ncols = (lf.nb - 1) * TB;
            if (z.r0 < TB) zr.push_back(z);
        }
    }
    // the upper 16x16 blocks of every diagonal tile: zero once per plan, written by nobody afterwards (zero_upper_blocks_kernel)
    std::vector<ZeroUpperTask> zu;
    int maxnb = 1;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.owner != l) continue;
        zu.push_back(ZeroUpperTask{c->h_leaves[l].F, lf.npad, lf.nb});
        maxnb = std::max(maxnb, lf.nb);
    }
    {   // both lists are on the device before the first launch: nothing returns between a launch and its synchronise
        DevBuf<ZeroRowsTask> zrows;
        DevBuf<ZeroUpperTask> zupper;
        if (int rc = dev_upload(c, zrows, zr)) return rc;
        if (int rc = dev_upload(c, zupper, zu)) return rc;
        if (!zr.empty()) zero_pad_rows_kernel<<<(int)zr.size(), 256, 0, c->stream>>>(zrows.p);
        for_leaf_chunks(zu.size(), [&](size_t b0, size_t cnt) {
            zero_upper_blocks_kernel<<<dim3((unsigned)cnt, (unsigned)std::min(maxnb, 64)), 256, 0, c->stream>>>(zupper.p + b0);
        });
        const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
        HIPCHK(c, e1);
        HIPCHK(c, e2);
    }

    if (int rc = build_schedule(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_PLAN);
    c->pool.mark();
    return 0;
}

// The part of the plan that depends on the sharing schedule alone, not on where the arenas are: phases, lanes, how every block step
// runs, the Gram list, the Dinv completions and the solve sweeps.  dsmgp_append_rows builds it twice over the same arenas: once with
// its one-shot continuation marks, once with the schedule it leaves behind.
int build_schedule(dsmgp_ctx* c) {
    const int L = c->L;
    // Phases: PREFIX leaves run after their sources (phase 1), everything else in phase 0 (COPY leaves ride with their source).
    // (Round 3 also built a split of the phase-0 leaves into two groups whose fused steps ran merged -- one launch carrying the
    // diagonal blocks of one group next to the tiles of the other, so that a CU mostly holds one latency-bound and one
    // pipe-bound workgroup: correct, and no faster -- depth 4 0.0601 s against 0.0586-0.0604 s -- so it is not in the tree.)
    c->leaf_group.assign(L, 0);
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].op == DSMGP_SHARE_PREFIX) c->leaf_group[l] = 1;
    // Lanes: sharing groups (a source with its COPY and PREFIX leaves) dealt longest-processing-time first on n^3.
    {
        std::vector<int> unit(L);
        std::vector<double> cost(L, 0.0);
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            unit[l] = lf.op == DSMGP_SHARE_FULL ? l : lf.src;
            const double n = (double)lf.n;
            cost[unit[l]] += lf.op == DSMGP_SHARE_COPY ? n * n : n * n * n;
        }
        int nunits = 0;
        for (int l = 0; l < L; ++l) nunits += unit[l] == l ? 1 : 0;
        // (also under a reserved pool -- the streaming context -- since round 6: every lane's split-K workspace is one more
        // arena carved from the pool's stack, lane after lane; config 5 at full size 111.4 -> 110.3 s with two lanes in every group)
        c->nlanes = c->lanes_opt > 0 ? c->lanes_opt : (nunits >= LANES_AUTO_MIN_LEAVES ? 2 : 1);
        c->nlanes = std::max(1, std::min(c->nlanes, nunits));
        c->leaf_lane.assign(L, 0);
        if (c->nlanes > 1) {
            std::vector<int> order;
            for (int l = 0; l < L; ++l)
                if (unit[l] == l) order.push_back(l);
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
            // (Weighing in the chain of a lane's largest leaf -- in the shard of an 8-rank job the lane that holds it ends at 52.3 ms,
            // the other, of equal flops and 77 steps instead of 103, at 47.5 -- by a cost per block step moves no end time that
            // matters: shards 0.0520 / 0.0513 / 0.0975 s without, 0.0519 / 0.0514 / 0.0971 with 0.13 ms a step, slower beyond;
            // tools/lane_timeline.py, profiles/r05_tail_ab.log.  What the early lane leaves behind runs on the whole chip.)
            double load[MAX_LANES] = {};
            std::vector<char> of_unit(L, 0);
            for (int u : order) {
                int lane = 0;
                for (int q = 1; q < c->nlanes; ++q)
                    if (load[q] < load[lane]) lane = q;
                of_unit[u] = (char)lane;
                load[lane] += cost[u];
            }
            for (int l = 0; l < L; ++l) c->leaf_lane[l] = of_unit[unit[l]];
        }
    }
    // How every block step runs (STEP_*).  Fused: the steps whose diagonal blocks alone fill the chip (or shallow ones).
    for (int ph = 0; ph < 2; ++ph) {
        int ns = 0;
        for (int l = 0; l < L; ++l)
            if (c->leaf_group[l] == ph) ns = std::max(ns, c->leaves[l].nb);
        c->fused_step[ph].assign(ns, STEP_CLASSIC);
        if (!gram_fused(c)) continue;
        for (int k = 0; k < ns; ++k) {
            int nd = 0;
            for (int l = 0; l < L; ++l) {
                const LeafHost& lf = c->leaves[l];
                if (c->leaf_group[l] == ph && lf.owner == l && lf.nb > k && k >= lf.kb) ++nd;
            }
            // (a depth limit on the first rule -- classic steps from block step 6 / 10 / 14 on even where the diagonal blocks fill
            // the chip -- gives the depth-3 model, whose fused steps reach K = 2304, 1.2 % at every limit and leaves depth 4
            // where it is: profiles/r05_tail_ab.log)
            // fused: the diagonal blocks alone fill the chip -- or the step is shallow (K <= 512: the one workgroup that
            // updates a diagonal tile before factorising it is done in a few microseconds; deeper, that update belongs in
            // the many-workgroup update launch, split along K)
            // (round 4: the shallow rule only where the step has leaves enough to give the two fused launches something to
            // do -- with the diagonal blocks one step ahead the classic steps of a handful of leaves are the shorter chain:
            // single GP 2.49 -> 2.25-2.31 ms, 8-rank shards 0.0560-0.0568 -> 0.0553-0.0560 s with no shallow step fused; the
            // headline model's 144 leaves and a PoE's 128 experts keep it)
            if (c->fuse_steps && (nd > c->ncu || (k <= FUSED_SHALLOW_STEPS && nd >= FUSED_SHALLOW_MIN_LEAVES))) c->fused_step[ph][k] = STEP_FUSED;
        }
    }
    // Gram tasks: lower tiles of every owner; with the Gram fused into the update tasks only the tiles that have none --
    // block column 0 (a PREFIX leaf: below the blocks it copies from its source; the copied blocks need no Gram at all),
    // and none at all where step 0 runs fused (its tasks start from the kernel function)
    std::vector<GramTask> gram;
    const bool fused = gram_fused(c);
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.owner != l) continue;
        {
            const std::vector<char>& fs = c->fused_step[(int)c->leaf_group[l]];
            if (fused && !fs.empty() && fs[0] != STEP_CLASSIC) continue;
        }
        const LeafDev& d = c->h_leaves[l];
        // (a leaf that continues from its OWN kept blocks -- dsmgp_append_rows, src == l -- may hold them in place: no tile of the
        // kept square is written; a PREFIX leaf proper gets its copy after this launch)
        const bool keeps_own = lf.op == DSMGP_SHARE_PREFIX && lf.src == l;
        for (int j = 0; j < (fused ? 1 : lf.nb); ++j)
            for (int i = ((fused || keeps_own) ? std::max(j, lf.kb) : j); i < lf.nb; ++i) {
                GramTask g{};
                g.xa = d.Xg + (size_t)i * TB;
                g.xb = d.Xg + (size_t)j * TB;
                g.out = d.F + (size_t)i * TB + (size_t)j * TB * lf.npad;
                g.lda = g.ldb = g.ldo = lf.npad;
                g.na = std::max(0, std::min(TB, lf.n - i * TB));
                g.nb = std::max(0, std::min(TB, lf.n - j * TB));
                g.sym = 1;
                g.diag = (i == j);
                g.kid = lf.kid;
                gram.push_back(g);
            }
    }
    if (int rc = dev_upload(c, c->gram, gram)) return rc;

    // Selective completions of Dinv_k inside fit! (the fused steps leave the 16x16 diagonal inverses only, kernels.hpp):
    {
        auto fused_in = [&](int ph, int k) { return k < (int)c->fused_step[ph].size() && c->fused_step[ph][k] == STEP_FUSED; };
        auto block_task = [&](int l, int k) {
            const LeafHost& lf = c->leaves[l];
            const LeafDev& d = c->h_leaves[l];
            DiagTask g{};
            g.T = d.F + (size_t)k * TB + (size_t)k * TB * lf.npad;
            g.Dinv = d.Dinv + (size_t)k * TB * TB;
            g.info = d.info;
            g.ld = lf.npad;
            g.nvalid = std::max(0, std::min(TB, lf.n - k * TB));
            g.row0 = k * TB;
            return g;
        };
        std::vector<DiagTask> pre, fw;
        std::vector<char> done(L, 0);
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.op == DSMGP_SHARE_PREFIX)      // its copied blocks: produced by the source's phase-0 steps
                for (int k = 0; k < lf.kb; ++k)
                    if (fused_in(0, k)) pre.push_back(block_task(l, k));
            if (lf.op == DSMGP_SHARE_FULL) continue;
            const int o = lf.owner;               // COPY: the source's buffers; PREFIX: its own
            if (done[o]) continue;
            done[o] = 1;
            const LeafHost& lo = c->leaves[o];
            const int pho = (int)c->leaf_group[o];
            for (int k = lo.kb; k < lo.nb; ++k)
                if (fused_in(pho, k)) fw.push_back(block_task(o, k));
        }
        if (int rc = dev_upload(c, c->dinvc_prefix, pre)) return rc;
        if (int rc = dev_upload(c, c->dinvc_fwd, fw)) return rc;
        // ... and on first use after it (ensure_dinv): every block an owner's fused step factorises (the copied blocks of a
        // PREFIX leaf are in `pre`: completed inside every fit)
        std::vector<DiagTask> all;
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.owner != l) continue;
            for (int k = lf.kb; k < lf.nb; ++k)
                if (fused_in((int)c->leaf_group[l], k)) all.push_back(block_task(l, k));
        }
        if (int rc = dev_upload(c, c->dinvc_all, all)) return rc;
    }
    // The step lists of the factorisation are built on first use: those for the train rows alone by the first fit! without a
    // resident test set (ensure_phase), those with the test rows riding along by dsmgp_set_test -- a context that only ever
    // fits with its test set resident (the streaming mode: 20 million tile tasks over the groups of config 5) builds one set.

    // solve sweeps.  Forward: only leaves whose factor came from elsewhere (COPY, PREFIX) -- leaves factorised
    // in full get z = L^-1 y from the factorisation itself (chol_diag_packed_kernel + the panel-solve epilogue).
    // Backward: every leaf.
    {
        int nsteps = 0;
        for (auto& lf : c->leaves) nsteps = std::max(nsteps, lf.nb);
        c->solve_steps = nsteps;
        std::vector<SolveTask> fwd, bwd;
        c->fwd_off.assign(nsteps + 1, 0);
        c->bwd_off.assign(nsteps + 1, 0);
        for (int k = 0; k < nsteps; ++k) {
            c->fwd_off[k] = (int)fwd.size();
            for (int l = 0; l < L; ++l) {
                const LeafHost& lf = c->leaves[l];
                if (lf.nb <= k) continue;
                if (lf.owner == l && lf.op == DSMGP_SHARE_FULL) continue;   // fused
                const LeafDev& d = c->h_leaves[l];
                for (int i = k; i < lf.nb; ++i) {
                    SolveTask s{};
                    s.Dk = d.Dinv + (size_t)k * TB * TB;
                    s.vk = d.w + (size_t)k * TB;
                    s.ldt = lf.npad;
                    if (i == k) {
                        s.self = 1;
                        s.out_k = d.z + (size_t)k * TB;
                    } else {
                        s.T = d.F + (size_t)i * TB + (size_t)k * TB * lf.npad;
                        s.vi = d.w + (size_t)i * TB;
                    }
                    fwd.push_back(s);
                }
            }
        }
        c->fwd_off[nsteps] = (int)fwd.size();
        // backward sweep on w = copy of z (z itself is kept: the predictive mean is m + (K_tn L^-T) z).
        // launch 0: alpha of every leaf's last block; launch s >= 1: block kb = nb-s updates the blocks left of
        // it with alpha_kb, and the task of block kb-1 finishes alpha_{kb-1} in the same workgroup.
        for (int s_ = 0; s_ < nsteps; ++s_) {
            c->bwd_off[s_] = (int)bwd.size();
            for (int l = 0; l < L; ++l) {
                const LeafHost& lf = c->leaves[l];
                const LeafDev& d = c->h_leaves[l];
                if (s_ == 0) {
                    SolveTask s{};
                    s.self = 1;
                    s.Dk = d.Dinv + (size_t)(lf.nb - 1) * TB * TB;
                    s.vk = d.w + (size_t)(lf.nb - 1) * TB;
                    s.out_k = d.alpha + (size_t)(lf.nb - 1) * TB;
                    s.ldt = lf.npad;
                    bwd.push_back(s);
                    continue;
                }
                const int kb = lf.nb - s_;
                if (kb < 1) continue;
                for (int j = 0; j < kb; ++j) {
                    SolveTask s{};
                    s.T = d.F + (size_t)kb * TB + (size_t)j * TB * lf.npad;
                    s.ldt = lf.npad;
                    s.vk = d.alpha + (size_t)kb * TB;
                    s.vi = d.w + (size_t)j * TB;
                    if (j == kb - 1) {
                        s.Dk = d.Dinv + (size_t)j * TB * TB;
                        s.out_k = d.alpha + (size_t)j * TB;
                    }
                    bwd.push_back(s);
                }
            }
        }
        c->bwd_off[nsteps] = (int)bwd.size();
        if (int rc = dev_upload(c, c->fwd, fwd)) return rc;
        if (int rc = dev_upload(c, c->bwd, bwd)) return rc;
    }
    return 0;
}

// Step lists of a fit! without resident test rows.  Built after the plan, possibly after the test arenas: with a device pool
// its split-K workspace is allocated outside the pool (the pool is a stack: plan < test < gradients).
int ensure_phase(dsmgp_ctx* c) {
    if (c->has(P_PHASE)) return 0;
    HostLog hl("ensure_phase: factor steps");
    c->alg_flops_update = c->alg_flops_fused = 0.0;
    for (int lane = 0; lane < c->nlanes; ++lane) {
        double fu = 0.0, ff = 0.0;
        if (int rc = build_factor_steps(c, lane, false, c->phase[lane], c->slabF[lane], fu, ff, true)) return rc;
        c->alg_flops_update += fu;
        c->alg_flops_fused += ff;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_PHASE);
    return 0;
}

// Step lists of a fit! with the registered test rows riding along: built on first use (see dsmgp_set_test).
int ensure_joint(dsmgp_ctx* c) {
    if (c->has(P_JOINT)) return 0;
    HostLog hl("ensure_joint: joint factor steps");
    c->alg_flops_joint = c->alg_flops_fused_joint = 0.0;
    for (int lane = 0; lane < c->nlanes; ++lane) {
        double fu = 0.0, ff = 0.0;
        if (int rc = build_factor_steps(c, lane, true, c->phaseJ[lane], c->slabJ[lane], fu, ff)) return rc;
        c->alg_flops_joint += fu;
        c->alg_flops_fused_joint += ff;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_JOINT);
    return 0;
}

// dpos / dfin / ndfin: an update launch that carries its step's diagonal-block tasks (tile_gemm_kernel_v2's grid layout)
void launch_tiles(dsmgp_ctx* c, const TileTask* tasks, int n, int role = 0 /* 0 update, 1 panel solve */, bool pad = false,
                  int dpos = 0, const DiagFinishTask* dfin = nullptr, int ndfin = 0, hipStream_t st = nullptr) {
    const int g = n + ndfin;
    if (!st) st = c->stream;
    if (pad) {   // launches with many padding-row tiles (small leaves): waves without data rows stay off the matrix pipe
        if (role == 1) tile_trsm_kernel<true><<<n, 256, 0, st>>>(tasks);
        else if (c->profile == 0 || c->alt_names) tile_gemm_kernel_v2<false, 2, true><<<g, 256, 0, st>>>(tasks, nullptr, c->d_kp.p, c->D, dpos, dfin, ndfin);
        else tile_gemm_kernel_v2<false, 0, true><<<g, 256, 0, st>>>(tasks, nullptr, c->d_kp.p, c->D, dpos, dfin, ndfin);
        return;
    }
    // ROLE only names the instantiation: with per-launch timing switched off (dsmgp_set_profile(ctx, 0)) the same code
    // runs as <false, 2>, so that a profiler's per-kernel average of <false, 0> covers exactly the launches bench.py times
    if (role == 1) tile_trsm_kernel<false><<<n, 256, 0, st>>>(tasks);   // B = inverse of a diagonal block, K = 128
    else if (c->profile == 0 || c->alt_names) tile_gemm_kernel_v2<false, 2><<<g, 256, 0, st>>>(tasks, nullptr, c->d_kp.p, c->D, dpos, dfin, ndfin);
    else tile_gemm_kernel_v2<false, 0><<<g, 256, 0, st>>>(tasks, nullptr, c->d_kp.p, c->D, dpos, dfin, ndfin);
}

// Two events bracketing a call on the context's stream; destroyed on every exit path.
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    hipError_t init() {
        hipError_t e = hipEventCreate(&a);
        return e != hipSuccess ? e : hipEventCreate(&b);
    }
    // init, then `launch()` between the two events on `st`; a launch error is returned
    template <class Launch>
    hipError_t timed(hipStream_t st, Launch&& launch) {
        hipError_t e = init();
        if (e == hipSuccess) e = hipEventRecord(a, st);
        if (e != hipSuccess) return e;
        launch();
        e = hipGetLastError();
        return e != hipSuccess ? e : hipEventRecord(b, st);
    }
    // after a synchronisation: the seconds between the two events, added to `seconds`
    hipError_t add_seconds(double& seconds) const {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, a, b);
        seconds += ms * 1e-3;
        return e;
    }
    ~EventPair() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

// hipEvent spans per kernel category.  The events come from a pool owned by the context (created once, reused by
// every fit/predict), so the timed region neither creates nor destroys events.
struct PhaseTimer {
    dsmgp_ctx* c;
    struct Span { int slot; int e0, e1; int step, tasks, red; };
    std::vector<Span> spans;
    size_t used = 0;
    explicit PhaseTimer(dsmgp_ctx* c_) : c(c_) {}
    bool on = false;
    int take() {
        if (used == c->event_pool.size()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return -1;
            c->event_pool.push_back(e);
        }
        return (int)used++;
    }
    void begin(int slot, hipStream_t st = nullptr) {
        on = c->profile >= 2 || (c->profile == 1 && (slot == 1 || slot == 18));
        if (!on) return;
        const int a = take(), b = take();
        if (a < 0 || b < 0) {
            on = false;
            return;
        }
        (void)hipEventRecord(c->event_pool[a], st ? st : c->stream);
        spans.push_back({slot, a, b, -1, 0, 0});
    }
    void note(int step, int ntasks, int nred) {
        if (on) {
            spans.back().step = step;
            spans.back().tasks = ntasks;
            spans.back().red = nred;
        }
    }
    void end(hipStream_t st = nullptr) {
        if (!on) return;
        (void)hipEventRecord(c->event_pool[spans.back().e1], st ? st : c->stream);
    }
    // ref: an event recorded before every span (the start of the call).  With two lanes the launches of a slot overlap in time:
    // next to the SUM of their durations (timings[slot]: what a profiler's per-kernel total is) the time during which ANY of
    // them ran -- the union of the intervals -- goes to timings[19] (update launches) and [20] (fused tile launches).
    void collect(hipEvent_t ref = nullptr) {
        const bool log = std::getenv("DSMGP_STEPLOG") != nullptr;
        std::vector<std::pair<float, float>> iv[2];
        for (const Span& s : spans) {
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, c->event_pool[s.e0], c->event_pool[s.e1]);
            c->timings[s.slot] += ms * 1e-3;
            float a = -1.f;
            if (ref && (log || s.slot == 1 || s.slot == 18)) (void)hipEventElapsedTime(&a, ref, c->event_pool[s.e0]);
            if (ref && (s.slot == 1 || s.slot == 18)) iv[s.slot == 1 ? 0 : 1].push_back({a, a + ms});
            if (log && s.step >= 0)
                std::fprintf(stderr, "steplog slot %d step %d tasks %d tiles %d ms %.4f at %.4f\n", s.slot, s.step, s.tasks, s.red, ms, a);
        }
        for (int q = 0; q < 2; ++q) {
            std::sort(iv[q].begin(), iv[q].end());
            double tot = 0.0;
            float lo = 0.f, hi = -1.f;
            for (const auto& p : iv[q]) {
                if (hi < 0.f || p.first > hi) {
                    if (hi >= 0.f) tot += hi - lo;
                    lo = p.first;
                    hi = p.second;
                } else if (p.second > hi) {
                    hi = p.second;
                }
            }
            if (hi >= 0.f) tot += hi - lo;
            c->timings[19 + q] += tot * 1e-3;
        }
        spans.clear();
        used = 0;
    }
};

// One block step of one lane's factorisation phase, on that lane's stream.  Classic step: update (-> split-K reduce) -> diagonal
// block -> panel solve.  Fused step (many leaves, or shallow): diag_fused_reg_kernel -> tile_fused8_kernel.
void run_step(dsmgp_ctx* c, StepLists& S, int k, PhaseTimer& pt, hipStream_t st, bool count_launches) {
    if (k >= S.nsteps) return;
    const int nfd = S.fdiag_off[k + 1] - S.fdiag_off[k], nft8 = S.ftile8_off[k + 1] - S.ftile8_off[k];
    const int nu = S.upd_off[k + 1] - S.upd_off[k];
    if (nfd > 0 || nft8 > 0) {     // fused step: diagonal blocks (their tile's update included), then the tiles below them
        if (nfd > 0) {
            pt.begin(2, st);
            diag_fused_reg_kernel<<<nfd, 256, DIAGR_LDS_BYTES, st>>>(S.fdiag.p + S.fdiag_off[k], c->d_kp.p, c->D);
            // Matern leaves: their diagonal blocks in a launch of their own over the same list (each kernel skips the other's)
            if (any_matern(c))
                diag_fused_reg_matern_kernel<<<nfd, 256, DIAGR_LDS_BYTES, st>>>(S.fdiag.p + S.fdiag_off[k], c->d_kp.p, c->D);
            if (any_rq(c))      // rational quadratic leaves likewise
                diag_fused_reg_rq_kernel<<<nfd, 256, DIAGR_LDS_BYTES, st>>>(S.fdiag.p + S.fdiag_off[k], c->d_kp.p, c->D);
            pt.note(k, nfd, 0);
            pt.end(st);
        }
        if (nft8 > 0) {
            pt.begin(18, st);
            if (c->profile == 0 || c->alt_names) tile_fused8_kernel<2><<<nft8, 512, 0, st>>>(S.ftile8.p + S.ftile8_off[k], c->d_kp.p, c->D);
            else tile_fused8_kernel<0><<<nft8, 512, 0, st>>>(S.ftile8.p + S.ftile8_off[k], c->d_kp.p, c->D);
            pt.note(k, nft8, nft8);
            pt.end(st);
            if (count_launches) c->n_fused_launches++;
        }
        return;
    }
    const int ndf = S.dfin_off[k + 1] - S.dfin_off[k];
    if (nu > 0 || ndf > 0) {
        pt.begin(1, st);
        launch_tiles(c, S.upd.p + S.upd_off[k], nu, 0, S.pad[k] != 0, S.dpos[k], S.dfin.p + S.dfin_off[k], ndf, st);
        pt.note(k, nu, S.step_tiles[k]);
        pt.end(st);
        const int nr = S.red_off[k + 1] - S.red_off[k];
        if (nr > 0) {
            pt.begin(13, st);
            tile_reduce_kernel<<<nr * REDUCE_WGS, 256, 0, st>>>(S.red.p + S.red_off[k]);
            pt.end(st);
        }
        if (count_launches) c->n_update_launches++;
    }
    const int nd = S.diag_off[k + 1] - S.diag_off[k];
    if (nd > 0) {
        pt.begin(2, st);
        chol_diag_packed_kernel<<<nd, 256, DIAGP_LDS_BYTES, st>>>(S.diag.p + S.diag_off[k]);
        pt.note(k, nd, 0);
        pt.end(st);
    }
    const int ns = S.trsm_off[k + 1] - S.trsm_off[k];
    if (ns > 0) {
        pt.begin(3, st);
        launch_tiles(c, S.trsm.p + S.trsm_off[k], ns, 1, S.pad[k] != 0, 0, nullptr, 0, st);
        pt.note(k, ns, 0);
        pt.end(st);
    }
}

// Lanes 1 .. nl-1 wait for what the context's stream has queued so far (fork); the context's stream waits for them (join).
// Lane 0 is the context's stream.
int fork_lanes(dsmgp_ctx* c, int nl) {
    if (nl > 1) {
        HIPCHK(c, hipEventRecord(c->ev_fork, c->stream));
        for (int lane = 1; lane < nl; ++lane) HIPCHK(c, hipStreamWaitEvent(c->lane_stream[lane], c->ev_fork, 0));
    }
    return 0;
}
int join_lanes(dsmgp_ctx* c, int nl) {
    for (int lane = 1; lane < nl; ++lane) {
        HIPCHK(c, hipEventRecord(c->ev_join[lane], c->lane_stream[lane]));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_join[lane], 0));
    }
    return 0;
}

// Phase `ph` of every lane: the lanes fork, take their block steps -- enqueued step by step, lane after lane, so that both queues
// stay fed -- and join.
int run_lanes(dsmgp_ctx* c, StepLists (*lists)[2], int ph, PhaseTimer& pt, bool count_launches) {
    int nsteps = 0;
    for (int lane = 0; lane < c->nlanes; ++lane) nsteps = std::max(nsteps, lists[lane][ph].nsteps);
    if (nsteps == 0) return 0;
    if (int rc = fork_lanes(c, c->nlanes)) return rc;
    // (Starting the second lane half a step late -- after the first launch of the first lane's step 0, so that the latency-bound
    // launches of one lane meet the pipe-bound ones of the other from the start -- measured nothing: headline 0.3870 / 0.3865 /
    // 0.3928 plain, 0.3870 / 0.3878 / 0.3922 staggered; depth 4 0.0495 / 0.0500 / 0.0495 against 0.0501 / 0.0498 / 0.0500
    // (profiles/r05_lane_stagger_ab.log): the lanes drift apart by themselves within a few steps.)
    for (int k = 0; k < nsteps; ++k)
        for (int lane = 0; lane < c->nlanes; ++lane) run_step(c, lists[lane][ph], k, pt, c->lane_stream[lane], count_launches);
    HIPCHK(c, hipGetLastError());
    return join_lanes(c, c->nlanes);
}

// The whole inverse of every diagonal block (the fused steps of a fit leave L_kk and its 16x16 diagonal inverses only): what the
// standalone prediction sweep, the gradients and the sweeps for alpha multiply with.  Queued on the context's stream.
int ensure_dinv(dsmgp_ctx* c) {
    if (c->has(P_DINV)) return 0;
    if (c->dinvc_all.count)
        dinv_complete_kernel<<<(int)c->dinvc_all.count, 256, DIAGP_LDS_BYTES, c->stream>>>(c->dinvc_all.p);
    HIPCHK(c, hipGetLastError());
    c->mark(P_DINV);
    return 0;
}

// alpha = L^-T z by the backward block sweep on w = copy of z (z stays: the predictive mean is m + V^T z).
int ensure_alpha(dsmgp_ctx* c) {
    if (c->has(P_ALPHA)) return 0;
    if (int rc = ensure_dinv(c)) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    int maxpad = 0;
    for (auto& lf : c->leaves) maxpad = std::max(maxpad, lf.npad);
    for_leaf_chunks((size_t)c->L, [&](size_t leaf0, size_t cnt) {
        copy_z_kernel<<<dim3((maxpad + 255) / 256, (unsigned)cnt), 256, 0, c->stream>>>(c->d_leaves.p, (int)leaf0);
    });
    for (int s = 0; s < c->solve_steps; ++s) {
        const int n = c->bwd_off[s + 1] - c->bwd_off[s];
        if (n > 0) solve_bwd_kernel<<<n, 256, 0, c->stream>>>(c->bwd.p + c->bwd_off[s]);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    c->timings[14] = ms * 1e-3;
    c->mark(P_ALPHA);
    return 0;
}

// The timing slots and launch counters that the launches of a fit fill
void reset_fit_timings(dsmgp_ctx* c) {
    for (int i = 0; i < 6; ++i) c->timings[i] = 0.0;
    c->timings[11] = c->timings[13] = c->timings[14] = 0.0;
    c->timings[18] = c->timings[19] = c->timings[20] = 0.0;
    c->n_update_launches = 0;
    c->n_fused_launches = 0;
}

// The launches of a fit over the step lists `phases` (c->phase, or c->phaseJ with the resident test rows riding along: joint), on
// the context's stream and the lanes'.  between(): what the caller queues between the two phases -- dsmgp_fit the copies of the
// PREFIX leaves' leading blocks, dsmgp_append_rows the relocation of the kept blocks.  Nothing here synchronises or records the
// call's own events: dsmgp_fit captures this sequence into a graph.
template <class Between>
int enqueue_fit(dsmgp_ctx* c, StepLists (*phases)[2], bool joint, PhaseTimer& pt, Between&& between) {
    const int L = c->L;
    HIPCHK(c, hipMemsetAsync(c->d_info.p, 0, (size_t)L * sizeof(int), c->stream));
    if (joint && c->acc_count) HIPCHK(c, hipMemsetAsync(c->arenaPV.p + c->acc_off, 0, c->acc_count * sizeof(double), c->stream));
    // 1. kernel matrices K + (noise + eps) I, lower tiles   (src/gaussianprocess.jl:83-98) [+ K_tn tiles]
    //    (fused into the update tasks: only the tiles of block column 0 are written here)
    {
        const DevBuf<GramTask>& tg = (joint && gram_fused(c)) ? c->pgram0 : c->pgram;
        pt.begin(0);
        if (c->gram.count) gram_tile_kernel<<<2 * (int)c->gram.count, 256, 0, c->stream>>>(c->gram.p, c->d_kp.p, c->D);
        if (joint && tg.count) gram_tile_kernel<<<2 * (int)tg.count, 256, 0, c->stream>>>(tg.p, c->d_kp.p, c->D);
        pt.end();
    }
    // 2. factorisation, full leaves first                    (src/gaussianprocess.jl:101); w = y - m rides along
    {
        int maxpad = 0;
        for (auto& lf : c->leaves) maxpad = std::max(maxpad, lf.npad);
        for_leaf_chunks((size_t)L, [&](size_t leaf0, size_t cnt) {
            copy_vec_kernel<<<dim3((maxpad + 255) / 256, (unsigned)cnt), 256, 0, c->stream>>>(c->d_leaves.p, (int)leaf0);
        });
    }
    if (int rc = run_lanes(c, phases, 0, pt, true)) return rc;
    // 3. prefix leaves: their leading blocks from where they are, continue (src/fit.jl:276-278).  (A table without a PREFIX
    //    leaf has no step in phase 1: run_lanes queues nothing, not even the fork.)
    if (int rc = between()) return rc;
    if (int rc = run_lanes(c, phases, 1, pt, true)) return rc;
    // 4. z = L^-1 (y - m) for the leaves whose factor came from another leaf (COPY, PREFIX); leaves factorised in
    //    full produced z during the factorisation.  alpha = L^-T z (src/gaussianprocess.jl:105) is NOT computed here:
    //    neither the log-marginal (z.z) nor the prediction (V^T z) needs it -- ensure_alpha() runs the backward sweep
    //    on first use (gradients, dsmgp_download_factor).
    {
        pt.begin(4);
        if (c->dinvc_fwd.count)
            dinv_complete_kernel<<<(int)c->dinvc_fwd.count, 256, DIAGP_LDS_BYTES, c->stream>>>(c->dinvc_fwd.p);
        for (int k = 0; k < c->solve_steps; ++k) {
            const int n = c->fwd_off[k + 1] - c->fwd_off[k];
            if (n > 0) solve_fwd_kernel<<<n, 256, 0, c->stream>>>(c->fwd.p + c->fwd_off[k]);
        }
        pt.end();
    }
    // 5. log marginal likelihood                              (src/gaussianprocess.jl:163)
    pt.begin(5);
    mll_kernel<<<L, 256, 0, c->stream>>>(c->d_leaves.p, c->d_mll.p);
    pt.end();
    return 0;
}

// mll and info of the fit that has just run, per leaf (either may be null).  info lives per factor owner.
int fetch_fit_results(dsmgp_ctx* c, double* mll_out, int32_t* info_out) {
    const int L = c->L;
    if (mll_out) HIPCHK(c, hipMemcpy(mll_out, c->d_mll.p, (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
    if (!info_out) return 0;
    std::vector<int> owner_info((size_t)L);
    HIPCHK(c, hipMemcpy(owner_info.data(), c->d_info.p, (size_t)L * sizeof(int), hipMemcpyDeviceToHost));
    for (int l = 0; l < L; ++l) info_out[l] = owner_info[(size_t)c->leaves[l].owner];
    // A PREFIX leaf whose source failed inside the rows it copied meets the damage at its first own pivot (row kb * TB + 1);
    // its first bad leading minor is the source's, and that is what LAPACK would report for the leaf
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.op != DSMGP_SHARE_PREFIX) continue;
        const int si = owner_info[(size_t)lf.src];
        if (si != 0 && si <= lf.kb * TB && info_out[l] != 0) info_out[l] = si;
    }
    return 0;
}

}  // namespace

// =================================================================================================
extern "C" {

int dsmgp_create(int32_t device_id, dsmgp_ctx** out) {
    if (!out) return fail(nullptr, DSMGP_E_ARG, "out is NULL");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, DSMGP_E_NODEVICE, "no HIP device visible: the GP-expert path has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, DSMGP_E_ARG, "device id out of range");
    dsmgp_ctx* c = new dsmgp_ctx();
    c->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&c->stream, DSMGP_STREAM_FLAGS) != hipSuccess) {
        delete c;
        return fail(nullptr, DSMGP_E_HIP, "cannot initialise device");
    }
    c->lane_stream[0] = c->stream;
    bool lanes_ok = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming) == hipSuccess;
    for (int lane = 1; lane < MAX_LANES && lanes_ok; ++lane)
        lanes_ok = hipStreamCreateWithFlags(&c->lane_stream[lane], DSMGP_STREAM_FLAGS) == hipSuccess &&
                   hipEventCreateWithFlags(&c->ev_join[lane], hipEventDisableTiming) == hipSuccess;
    if (!lanes_ok) {
        (void)hipStreamDestroy(c->stream);
        delete c;
        return fail(nullptr, DSMGP_E_HIP, "cannot create the lanes' streams");
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(chol_diag_packed_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, DIAGP_LDS_BYTES);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(dinv_complete_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, DIAGP_LDS_BYTES);
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device_id) == hipSuccess && prop.multiProcessorCount > 0)
            c->ncu = prop.multiProcessorCount;
    }
#ifdef DSMGP_DIAG   // scheduling knobs of the diagnostic build (DSMGP_XCD, DSMGP_TAIL_SPLIT, DSMGP_TAIL_ROUNDS); the product build reads no tuning variables
    if (const char* s = std::getenv("DSMGP_XCD")) c->xcd_order = std::atoi(s) != 0;
    if (const char* s = std::getenv("DSMGP_TAIL_SPLIT")) c->tail_split = c->tail_split_lanes = std::max(1, std::atoi(s));
    if (const char* s = std::getenv("DSMGP_TAIL_ROUNDS")) c->tail_rounds = c->tail_rounds_lanes = std::max(0, std::atoi(s));
    if (const char* s = std::getenv("DSMGP_RAGGED_ROUNDS")) c->ragged_rounds = std::max(1, std::atoi(s));
    if (const char* s = std::getenv("DSMGP_RAGGED_DIV")) c->ragged_div = std::max(1, std::atoi(s));
#endif
    const char* p = std::getenv("DSMGP_PROFILE");
    c->profile = p ? std::atoi(p) * 2 : 0;   // DSMGP_PROFILE=1 -> every category
    *out = c;
    return 0;
}

int dsmgp_destroy(dsmgp_ctx* c) {
    if (!c) return DSMGP_E_ARG;
    (void)hipSetDevice(c->device);
    free_plan_and_test(c);
    c->pool.release();
    (void)dsmgp_comm_destroy(c);
    drop_graphs(c);
    if (c->side) {
        (void)hipStreamSynchronize(c->side);
        (void)hipStreamDestroy(c->side);
    }
    if (c->stage) (void)hipHostFree(c->stage);
    c->stage = nullptr;
    for (hipEvent_t e : c->event_pool) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (int lane = 1; lane < MAX_LANES; ++lane) {
        if (c->ev_join[lane]) (void)hipEventDestroy(c->ev_join[lane]);
        if (c->lane_stream[lane]) (void)hipStreamDestroy(c->lane_stream[lane]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;               // the context's device arrays go with their owners
    return 0;
}

const char* dsmgp_last_error(dsmgp_ctx* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int dsmgp_device_name(dsmgp_ctx* c, char* buf, int32_t len) {
    if (!c || !buf || len <= 0) return DSMGP_E_ARG;
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, c->device));
    std::snprintf(buf, len, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return 0;
}

int dsmgp_set_joint(dsmgp_ctx* c, int32_t on) {
    if (!c) return DSMGP_E_ARG;
    c->joint = on != 0;
    return 0;
}

int dsmgp_set_option(dsmgp_ctx* c, int32_t option, int32_t value) {
    if (!c) return DSMGP_E_ARG;
    if (option == DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT) {
        if ((value != 0) != c->ard_true_gradient) {
            HIPCHK(c, hipSetDevice(c->device));
            free_grad(c);     // the contraction tile list depends on it
        }
        c->ard_true_gradient = value != 0;
        return 0;
    }
    if (option == DSMGP_OPT_FIT_GRAPH) {
        if (value == 0) drop_graphs(c);
        c->use_graph = value != 0;
        return 0;
    }
    // PLAN_OPTIONS: the task lists of fit! (and, through the plan, of the resident test set) depend on them
    int* const opt = option == DSMGP_OPT_FUSED_GRAM ? &c->fuse_gram : option == DSMGP_OPT_FUSED_STEPS ? &c->fuse_steps :
                     option == DSMGP_OPT_DIAG_IN_UPDATE ? &c->diag_in_update : option == DSMGP_OPT_LANES ? &c->lanes_opt : nullptr;
    if (!opt) return fail(c, DSMGP_E_ARG, "set_option: unknown option");
    if (opt == &c->lanes_opt) {
        if (value < 0 || value > MAX_LANES) return fail(c, DSMGP_E_ARG, "set_option: lanes must be 0 (automatic) or 1 .. 4");
    } else {
        value = value != 0;
    }
    if (value != *opt) {
        HIPCHK(c, hipSetDevice(c->device));
        free_plan_and_test(c);
    }
    *opt = value;
    return 0;
}

int dsmgp_set_profile(dsmgp_ctx* c, int32_t on) {
    if (!c) return DSMGP_E_ARG;
    c->alt_names = on == 3;         // level 3 = level 1 under the kernel names of level 0 (bench.py's single-lane extra)
    c->profile = on < 0 ? 0 : (on == 3 ? 1 : (on > 2 ? 2 : on));
    return 0;
}

int dsmgp_set_train(dsmgp_ctx* c, const double* X, const double* y, int64_t N, int32_t D) {
    if (!c) return DSMGP_E_ARG;
    if (!X || !y || N <= 0 || D <= 0) return fail(c, DSMGP_E_ARG, "set_train: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    free_plan_and_test(c);
    free_tree(c);
    c->dX.release();
    c->dy.release();
    c->N = N;
    c->D = D;
    if (int rc = c->dX.alloc(c, (size_t)N * D)) return rc;
    if (int rc = c->dy.alloc(c, (size_t)N)) return rc;
    HIPCHK(c, hipMemcpy(c->dX.p, X, (size_t)N * D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->dy.p, y, (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    c->L = 0;
    c->leaves.clear();
    return 0;
}

int dsmgp_set_leaves(dsmgp_ctx* c, int32_t L, const int64_t* obs_ptr, const int64_t* obs_idx,
                     const int32_t* kernel_id, const double* mean) {
    if (!c) return DSMGP_E_ARG;
    if (!c->dX.p) return fail(c, DSMGP_E_STATE, "set_leaves before set_train");
    if (L <= 0 || !obs_ptr || !obs_idx || !kernel_id || !mean) return fail(c, DSMGP_E_ARG, "set_leaves: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    free_plan_and_test(c);
    free_tree(c);           // its regions name indices of the OLD leaf table
    if (obs_ptr[0] != 0) return fail(c, DSMGP_E_ARG, "obs_ptr[0] must be 0");
    c->leaves.assign(L, LeafHost{});
    c->grad_active.clear();         // a new leaf table: gradients of every leaf again
    for (int l = 0; l < L; ++l) {
        const int64_t a = obs_ptr[l], b = obs_ptr[l + 1];
        if (b <= a) return fail(c, DSMGP_E_ARG, "leaf " + std::to_string(l) + " has no observations");
        if (b - a > (int64_t)1 << 20) return fail(c, DSMGP_E_ARG, "leaf too large");
        for (int64_t i = a; i < b; ++i) {
            if (obs_idx[i] < 0 || obs_idx[i] >= c->N) return fail(c, DSMGP_E_ARG, "observation index out of range");
            if (i > a && obs_idx[i] <= obs_idx[i - 1]) return fail(c, DSMGP_E_ARG, "obs lists must be strictly ascending");
        }
        if (kernel_id[l] < 0 || kernel_id[l] >= DSMGP_MAX_KERNEL_IDS) return fail(c, DSMGP_E_ARG, "kernel id out of range");
        LeafHost& lf = c->leaves[l];
        lf.n = (int)(b - a);
        lf.npad = round_up(lf.n, TB);
        lf.nb = lf.npad / TB;
        lf.kid = kernel_id[l];
        lf.mean = mean[l];
        lf.obs_off = a;
    }
    c->L = L;
    c->obs_ptr.assign(obs_ptr, obs_ptr + L + 1);
    c->obs_idx.assign(obs_idx, obs_idx + obs_ptr[L]);
    c->d_obs_ptr.release();
    c->d_obs_idx.release();
    if (int rc = c->d_obs_ptr.alloc(c, (size_t)L + 1)) return rc;
    if (int rc = c->d_obs_idx.grow(c, c->obs_idx.size(), std::max<size_t>(1, c->obs_idx.size()))) return rc;
    HIPCHK(c, hipMemcpy(c->d_obs_ptr.p, obs_ptr, (L + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->d_obs_idx.p, obs_idx, c->obs_idx.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    return 0;
}

int dsmgp_set_sharing(dsmgp_ctx* c, const int32_t* op, const int32_t* src, const int64_t* prefix_len) {
    if (!c) return DSMGP_E_ARG;
    if (c->L == 0) return fail(c, DSMGP_E_STATE, "set_sharing before set_leaves");
    const int L = c->L;
    // the whole schedule is validated into temporaries and committed at the end: a rejected schedule leaves the
    // context (leaf table, task lists of the previous schedule) exactly as it was
    struct Share { int op; int src; int64_t prefix; };
    std::vector<Share> sh(L, Share{DSMGP_SHARE_FULL, -1, 0});
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const int o = op ? op[l] : DSMGP_SHARE_FULL;
        if (o == DSMGP_SHARE_FULL) continue;
        if (!src || src[l] < 0 || src[l] >= L || src[l] == l) return fail(c, DSMGP_E_ARG, "sharing: bad source leaf");
        const LeafHost& s = c->leaves[src[l]];
        const int so = op[src[l]];
        if (so != DSMGP_SHARE_FULL) return fail(c, DSMGP_E_ARG, "sharing: source leaf must be factorised in full");
        if (s.kid != lf.kid) return fail(c, DSMGP_E_ARG, "sharing: kernel ids differ");
        const int64_t* a = c->obs_idx.data() + lf.obs_off;
        const int64_t* b = c->obs_idx.data() + s.obs_off;
        if (o == DSMGP_SHARE_COPY) {
            if (s.n != lf.n || std::memcmp(a, b, sizeof(int64_t) * lf.n) != 0)
                return fail(c, DSMGP_E_ARG, "sharing: COPY needs identical observation lists");
            sh[l] = Share{o, src[l], 0};
        } else if (o == DSMGP_SHARE_PREFIX) {
            if (!prefix_len || prefix_len[l] != s.n || s.n >= lf.n || std::memcmp(a, b, sizeof(int64_t) * s.n) != 0)
                return fail(c, DSMGP_E_ARG, "sharing: PREFIX needs the source's list as a strict prefix");
            sh[l] = Share{o, src[l], prefix_len[l]};
        } else {
            return fail(c, DSMGP_E_ARG, "sharing: unknown op");
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    free_plan_and_test(c);
    for (int l = 0; l < L; ++l) {
        c->leaves[l].op = sh[l].op;
        c->leaves[l].src = sh[l].src;
        c->leaves[l].prefix = sh[l].prefix;
    }
    return 0;
}

int dsmgp_set_hyper(dsmgp_ctx* c, int32_t kernel_id, int32_t kind, const double* loghyp, int32_t n) {
    if (!c) return DSMGP_E_ARG;
    if (kernel_id < 0 || kernel_id >= DSMGP_MAX_KERNEL_IDS || !loghyp || n < 3) return fail(c, DSMGP_E_ARG, "set_hyper: bad arguments");
    if (kind < 0 || kind > DSMGP_KIND_ARD_RQ) return fail(c, DSMGP_E_ARG, "set_hyper: unknown kernel kind");
    const KindInfo& ki = KINDS[kind];
    if (ki.set_checked && ki.ard && c->D > 0 && n != c->D + 2 + ki.n_shape)
        return fail(c, DSMGP_E_ARG, std::string("set_hyper: ") + ki.name + " needs one lengthscale per input dimension");
    if (ki.set_checked && ki.ard && n < 3 + ki.n_shape)      // before set_train has fixed D: at least one length-scale
        return fail(c, DSMGP_E_ARG, std::string("set_hyper: ") + ki.name + " needs one lengthscale per input dimension");
    if (ki.set_checked && !ki.ard && n != 3 + ki.n_shape)
        return fail(c, DSMGP_E_ARG, std::string("set_hyper: ") + ki.name +
                                        (ki.n_shape ? " takes [logl, loga, logs, logNoise]" : " takes [logl, logs, logNoise]"));
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(loghyp[i])) return fail(c, DSMGP_E_ARG, "set_hyper: non-finite hyper-parameter");
    if ((int)c->hyper.size() <= kernel_id) c->hyper.resize(kernel_id + 1);
    const bool had_matern = any_matern(c), had_rq = any_rq(c);
    if (c->hyper[kernel_id].kind != kind) free_grad(c);   // the contraction tiles / ArdLinear tasks depend on the kernel kind
    c->hyper[kernel_id].kind = kind;
    c->hyper[kernel_id].loghyp.assign(loghyp, loghyp + n);
    // a captured fit launches diag_fused_reg_matern_kernel / diag_fused_reg_rq_kernel or not
    if (any_matern(c) != had_matern || any_rq(c) != had_rq) drop_graphs(c);
    c->invalidate(P_FIT);   // (the aggregation's sums fall too: the rBCM finish would read its prior variance from the NEXT KParam table)
    return 0;
}

int dsmgp_fit(dsmgp_ctx* c, double* mll_out, int32_t* info_out, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (c->L == 0) return fail(c, DSMGP_E_STATE, "fit before set_leaves");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = check_hyper(c)) return rc;
    if (int rc = build_plan(c)) return rc;
    if (int rc = upload_hyper(c)) return rc;
    // With a resident test set the rows of K_tn ride through the same launches (build_factor_steps).
    const bool joint = c->joint && c->has(P_TEST);
    c->resume_armed = false;        // the factor changes: what dsmgp_add_rows_keep_test kept of K_tn L^-T is stale from here on
    if (joint) {
        if (int rc = full_sweep_lists(c)) return rc;      // (the joint fit launches pgram where the Gram is not fused)
        if (int rc = ensure_joint(c)) return rc;
    } else if (int rc = ensure_phase(c)) {
        return rc;
    }
    const int L = c->L;
    reset_fit_timings(c);
    PhaseTimer pt(c);
    EventPair ev;
    HIPCHK(c, ev.init());
    const hipEvent_t t0 = ev.a, t1 = ev.b;
    HIPCHK(c, hipEventRecord(t0, c->stream));

    // between the phases: the leading blocks of every PREFIX leaf, copied from its source's factor
    auto prefix_copies = [&]() -> int {
        bool any_prefix = false;
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.op != DSMGP_SHARE_PREFIX) continue;
            any_prefix = true;
            const LeafDev& d = c->h_leaves[l];
            const LeafDev& s = c->h_leaves[lf.src];
            const size_t rows = (size_t)lf.kb * TB;
            HIPCHK(c, hipMemcpy2DAsync(d.F, (size_t)d.npad * sizeof(double), s.F, (size_t)s.npad * sizeof(double),
                                       rows * sizeof(double), rows, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(d.Dinv, s.Dinv, rows * TB * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        }
        if (any_prefix && c->dinvc_prefix.count)    // copied blocks that a fused step factorised: their whole inverse, for the classic steps of phase 1
            dinv_complete_kernel<<<(int)c->dinvc_prefix.count, 256, DIAGP_LDS_BYTES, c->stream>>>(c->dinvc_prefix.p);
        return 0;
    };
    auto enqueue = [&]() -> int { return enqueue_fit(c, joint ? c->phaseJ : c->phase, joint, pt, prefix_copies); };
    c->invalidate(P_FIT);           // the factors are rewritten from here on
    // Replay the sequence as a graph while nothing inside it records events (profile 0); capture it on first use
    const int gk = joint ? 1 : 0;
    if (c->use_graph && c->profile == 0) {
        if (!c->fit_graph[gk]) {
            hipGraph_t g = nullptr;
            HIPCHK(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue();
            const hipError_t ce = hipStreamEndCapture(c->stream, &g);
            if (rc != 0 || ce != hipSuccess || !g) {
                if (g) (void)hipGraphDestroy(g);
                (void)hipGetLastError();
                c->use_graph = false;               // this runtime cannot capture the sequence: plain launches from here on
                if (rc != 0) return rc;
            } else {
                const hipError_t ie = hipGraphInstantiate(&c->fit_graph[gk], g, nullptr, nullptr, 0);
                (void)hipGraphDestroy(g);
                if (ie != hipSuccess) {
                    c->fit_graph[gk] = nullptr;
                    (void)hipGetLastError();
                    c->use_graph = false;
                }
                c->graph_launches[gk][0] = c->n_update_launches;      // counted by the capture pass: the same on every replay
                c->graph_launches[gk][1] = c->n_fused_launches;
            }
        }
        if (c->fit_graph[gk]) {
            HIPCHK(c, hipGraphLaunch(c->fit_graph[gk], c->stream));
            c->n_update_launches = c->graph_launches[gk][0];
            c->n_fused_launches = c->graph_launches[gk][1];
        } else if (int rc = enqueue()) {
            return rc;
        }
    } else {
        if (int rc = enqueue()) return rc;
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(t1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
    pt.collect(t0);
    c->timings[11] = ms * 1e-3;
    if (seconds) *seconds = ms * 1e-3;
    if (int rc = fetch_fit_results(c, mll_out, info_out)) return rc;
    c->mark(P_FIT);
    if (joint) c->mark(P_VT);
    c->vt_from_fit = joint;
    c->last_fit_joint = joint;
    return 0;
}

// Append training rows to the fitted model: every factor owner keeps the leading blocks of the factor it had and continues
// from them, through the PREFIX phase of the fit with the leaf's OWN old factor as the source (include/dsmgp_hip.h).
// What dsmgp_add_rows_keep_test carries of the resident test set across the rebuild of the plan
struct KeptTest {
    struct Leaf {
        size_t vt_off;
        int ntpad, npad;
        int have;                   // leading block columns of the leaf's K_tn L^-T that were current when the call began
    };
    bool resident = false;
    std::vector<Leaf> old;
    DevArena arena;                 // the previous arenaVt: owned here until the context takes it back or it is put
};

// The test set again on the grown plan (the fit is done, the old factors are gone).  A leaf keeps the block columns that were
// current and belong to kept blocks of the factor it reads -- its owner's, so a COPY leaf its source's.  IN PLACE where no leaf's
// offset or size in the arena moves; else RELOCATE: a new arena beside the old, the kept column runs (contiguous: 128 x 128
// tiles with lds = ldd = ntpad) in one launch, then the old one is put -- never a move inside one arena, whose source and
// destination would overlap.  rs: dsmgp_resume_stats.  An error leaves the set half built: the caller drops it.
static int keep_test_set(dsmgp_ctx* c, KeptTest& kt, const std::vector<int>& factor_keep, int64_t* rs) {
    const int L = c->L;
    std::vector<int> first((size_t)L, 0);
    std::vector<size_t> off((size_t)L, 0);
    size_t vTot = 0;
    bool same = true, any = false;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const KeptTest::Leaf& o = kt.old[(size_t)l];
        off[(size_t)l] = vTot;
        vTot += (size_t)o.ntpad * lf.npad;      // (register_test's layout: the routes, and with them ntpad, are what they were)
        if (off[(size_t)l] != o.vt_off || lf.npad != o.npad) same = false;
        if (c->route_ptr[(size_t)l + 1] == c->route_ptr[(size_t)l]) continue;
        first[(size_t)l] = std::min(std::min(o.have, factor_keep[(size_t)lf.owner]), lf.nb);
        if (first[(size_t)l] > 0) {
            any = true;
            rs[0]++;
            rs[1] += first[(size_t)l];
        } else {
            rs[4]++;
        }
    }
    if (same || !any) {     // in place -- or nothing to keep: register_test takes the arena over while it fits
        c->arenaVt = std::move(kt.arena);
    } else {
        const size_t want = vTot + vTot / 8;
        size_t freeB = 0, totalB = 0;
        HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
        if (want * sizeof(double) + (size_t(1) << 30) > freeB)
            return fail(c, DSMGP_E_NOMEM, "add_rows_keep_test: no room for the new K_tn arena beside the old one");
        if (int rc = arena_status(c, c->arenaVt.get(arena_pool(c), want))) return rc;
        std::vector<RelocTask> rt;
        for (int l = 0; l < L; ++l) {
            const KeptTest::Leaf& o = kt.old[(size_t)l];
            for (int j = 0; j < first[(size_t)l]; ++j)
                for (int i = 0; i < o.ntpad / TB; ++i) {
                    const size_t at = (size_t)i * TB + (size_t)j * TB * (size_t)o.ntpad;
                    rt.push_back(RelocTask{kt.arena.p + o.vt_off + at, c->arenaVt.p + off[(size_t)l] + at, o.ntpad, o.ntpad});
                }
        }
        DevBuf<RelocTask> reloc;
        if (int rc = dev_upload(c, reloc, rt)) return rc;
        relocate_tiles_kernel<<<(unsigned)rt.size(), 256, 0, c->stream>>>(reloc.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        kt.arena.put();
        rs[2] = (int64_t)rt.size() * TB * TB * (int64_t)sizeof(double);
    }
    const double* const arena = c->arenaVt.p;
    c->stage_top = 0;       // (the stream is idle)
    HostLog hl("add_rows_keep_test: sizes");
    if (int rc = register_test(c, hl, &first)) return rc;
    if (any && c->arenaVt.p != arena) return fail(c, DSMGP_E_STATE, "add_rows_keep_test: the K_tn arena was replaced");
    c->vt_first = first;
    c->resume_armed = true;
    return 0;
}

// The argument checks of grow_rows that read nothing but the arguments and the leaf table's sizes
static int check_added_rows(dsmgp_ctx* c, const double* X_new, const double* y_new, int64_t m, int32_t D, const int64_t* add_ptr,
                            const int64_t* add_idx, const double* mean) {
    const int L = c->L;
    if (add_ptr[0] != 0) return fail(c, DSMGP_E_ARG, "append_rows: add_ptr[0] must be 0");
    for (int l = 0; l < L; ++l) {
        const int64_t a = add_ptr[l], b = add_ptr[l + 1];
        if (b < a) return fail(c, DSMGP_E_ARG, "append_rows: add_ptr must not descend");
        if (b - a > m) return fail(c, DSMGP_E_ARG, "append_rows: a list that is not strictly ascending");
        if ((int64_t)c->leaves[l].n + (b - a) > (int64_t)1 << 20) return fail(c, DSMGP_E_ARG, "append_rows: leaf too large");
        for (int64_t i = a; i < b; ++i) {
            if (add_idx[i] < 0 || add_idx[i] >= m) return fail(c, DSMGP_E_ARG, "append_rows: position out of range");
            if (i > a && add_idx[i] <= add_idx[i - 1]) return fail(c, DSMGP_E_ARG, "append_rows: lists must be strictly ascending");
        }
    }
    for (int64_t i = 0; i < m * (int64_t)D; ++i)
        if (!std::isfinite(X_new[i])) return fail(c, DSMGP_E_ARG, "append_rows: non-finite value in X_new");
    for (int64_t i = 0; i < m; ++i)
        if (!std::isfinite(y_new[i])) return fail(c, DSMGP_E_ARG, "append_rows: non-finite value in y_new");
    if (mean)
        for (int l = 0; l < L; ++l)
            if (!std::isfinite(mean[l])) return fail(c, DSMGP_E_ARG, "append_rows: non-finite mean");
    return 0;
}

// keep_test (dsmgp_add_rows_keep_test): a resident test set stays resident -- its rows, routes and entry index as they are, the second
// half of its registration again on the grown plan -- and, where dsmgp_predict_run had run on the fit the call finds, every leaf
// keeps the leading block columns of K_tn L^-T that belong to the kept blocks of the factor it reads (keep_test_set, above).
static int grow_rows(dsmgp_ctx* c, const double* X_new, const double* y_new, int64_t m, int32_t D, const int64_t* add_ptr,
                     const int64_t* add_idx, const double* mean, double* mll_out, int32_t* info_out, double* seconds, bool keep_test) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "append_rows needs a current fit");
    if (c->pool.active()) return fail(c, DSMGP_E_STATE, "append_rows under a reserved pool");
    if (!X_new || !y_new || !add_ptr || !add_idx || m < 1) return fail(c, DSMGP_E_ARG, "append_rows: bad arguments");
    if (D != c->D) return fail(c, DSMGP_E_ARG, "append_rows: D is not the D of set_train");
    if (int rc = check_added_rows(c, X_new, y_new, m, D, add_ptr, add_idx, mean)) return rc;
    const int L = c->L;
    const int64_t N0 = c->N;
    HIPCHK(c, hipSetDevice(c->device));

    // 1. what the kept blocks need before they are read again: every Dinv_k whole (the fused steps of the fit left the 16x16
    //    inverses only), and who failed (their kept blocks are damaged: factorised from block 0)
    if (int rc = ensure_dinv(c)) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::vector<int> old_info((size_t)L);
    HIPCHK(c, hipMemcpy(old_info.data(), c->d_info.p, (size_t)L * sizeof(int), hipMemcpyDeviceToHost));

    // 2. the grown data beside the old: nothing of the context has changed if it does not fit
    DevBuf<double> nX, ny;
    {
        DevBuf<double> aX, ay;
        // (the message says so: a caller that mirrors the table's sizes -- hipabi.Context -- tells this DSMGP_E_NOMEM from the later one)
        auto unchanged = [&](int rc) { return fail(c, rc, "append_rows: the grown data do not fit, the context is unchanged (" + c->err + ")"); };
        if (int rc = aX.alloc(c, (size_t)m * D)) return unchanged(rc);
        if (int rc = ay.alloc(c, (size_t)m)) return unchanged(rc);
        if (int rc = nX.alloc(c, (size_t)(N0 + m) * D)) return unchanged(rc);
        if (int rc = ny.alloc(c, (size_t)(N0 + m))) return unchanged(rc);
        HIPCHK(c, hipMemcpy(aX.p, X_new, (size_t)m * D * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(ay.p, y_new, (size_t)m * sizeof(double), hipMemcpyHostToDevice));
        const long long total = (long long)(N0 + m) * D;
        const int grid = (int)std::min<long long>((total + 255) / 256, 65536);
        append_rows_kernel<<<grid, 256, 0, c->stream>>>(c->dX.p, aX.p, nX.p, (long long)N0, (long long)m, D);
        append_rows_kernel<<<grid, 256, 0, c->stream>>>(c->dy.p, ay.p, ny.p, (long long)N0, (long long)m, 1);
        const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
        HIPCHK(c, e1);
        HIPCHK(c, e2);
    }

    // 3. the previous plan: where every factor sits, and the arenas themselves, moved out of the context -- free_plan finds nothing
    //    there, and whatever this call does not hand back (build_plan in place, keep_test_set) goes when the call returns
    struct Old { size_t f_off, dinv_off; int n, npad, nb, owner, op, src; double mean; };
    std::vector<Old> old((size_t)L);
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        old[(size_t)l] = Old{lf.f_off, lf.dinv_off, lf.n, lf.npad, lf.nb, lf.owner, lf.op, lf.src, lf.mean};
    }
    DevArena oldF = std::move(c->arenaF), oldDinv = std::move(c->arenaDinv);
    // ... and, for a test set that stays, where every leaf's K_tn L^-T sits, how much of it is current, and the arena itself
    KeptTest kt;
    kt.resident = keep_test && c->has(P_TEST);
    if (kt.resident) {
        const bool swept = c->has(P_PRED), pending = !c->has(P_VT) && c->resume_armed;
        kt.old.resize((size_t)L);
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            kt.old[(size_t)l] = KeptTest::Leaf{lf.vt_off, lf.ntpad, lf.npad, swept ? lf.nb : (pending ? c->vt_first[(size_t)l] : 0)};
        }
        kt.arena = std::move(c->arenaVt);
        free_plan(c);
        free_test_products(c, true);    // the rows, the CSR and the entry index stay as they are
    } else {
        free_plan_and_test(c);      // (the routing tree stays: leaf indices do not change)
    }
    c->grad_active.clear();

    // 4. the grown leaf table and the schedule it keeps: COPY where source and leaf got the same rows, FULL elsewhere
    auto adds_of = [&](int l) { return add_ptr[l + 1] - add_ptr[l]; };
    auto same_adds = [&](int a, int b) {
        return adds_of(a) == adds_of(b) &&
               (adds_of(a) == 0 || std::memcmp(add_idx + add_ptr[a], add_idx + add_ptr[b], sizeof(int64_t) * (size_t)adds_of(a)) == 0);
    };
    {
        std::vector<int64_t> ptr((size_t)L + 1, 0), idx;
        idx.reserve(c->obs_idx.size() + (size_t)add_ptr[L]);
        for (int l = 0; l < L; ++l) {
            LeafHost& lf = c->leaves[l];
            idx.insert(idx.end(), c->obs_idx.begin() + lf.obs_off, c->obs_idx.begin() + lf.obs_off + lf.n);
            for (int64_t i = add_ptr[l]; i < add_ptr[l + 1]; ++i) idx.push_back(N0 + add_idx[i]);
            ptr[(size_t)l + 1] = (int64_t)idx.size();
        }
        for (int l = 0; l < L; ++l) {
            LeafHost& lf = c->leaves[l];
            lf.obs_off = ptr[(size_t)l];
            lf.n = (int)(ptr[(size_t)l + 1] - ptr[(size_t)l]);
            lf.npad = round_up(lf.n, TB);
            lf.nb = lf.npad / TB;
            if (mean) lf.mean = mean[l];
        }
        c->obs_ptr.swap(ptr);
        c->obs_idx.swap(idx);
    }
    c->dX = std::move(nX);
    c->dy = std::move(ny);
    c->N = N0 + m;
    int64_t st[DSMGP_N_APPEND_STATS] = {0, 0, 0, 0, 0, 0};
    std::vector<char> stays_copy((size_t)L, 0);
    for (int l = 0; l < L; ++l)
        if (old[(size_t)l].op == DSMGP_SHARE_COPY) {
            stays_copy[(size_t)l] = same_adds(l, old[(size_t)l].src) ? 1 : 0;
            if (!stays_copy[(size_t)l]) st[5]++;
        }
    auto final_schedule = [&]() {       // what later fits run under
        for (int l = 0; l < (int)c->leaves.size(); ++l) {
            LeafHost& lf = c->leaves[l];
            lf.op = stays_copy[(size_t)l] ? DSMGP_SHARE_COPY : DSMGP_SHARE_FULL;
            lf.src = stays_copy[(size_t)l] ? old[(size_t)l].src : -1;
            lf.prefix = 0;
        }
    };
    // whatever goes wrong from here on: the grown data and leaf table, no plan, no fit -- as after dsmgp_set_leaves.  (The old
    // arenas go with their owners: the context's with free_plan_and_test, those still held here when the call returns.)
    auto give_up = [&](int rc) {
        const std::string msg = c->err;
        (void)hipStreamSynchronize(c->stream);
        free_plan_and_test(c);
        final_schedule();
        c->err = msg;
        return rc;
    };
    // ... except where the device copy of the grown leaf table itself cannot be made: a plan must never gather through a missing
    // or stale copy, so the leaf table goes (the grown data stay; dsmgp_set_leaves is the next call, anything else: DSMGP_E_STATE)
    auto without_table = [&](int rc) {
        give_up(rc);
        c->L = 0;
        c->leaves.clear();
        c->obs_ptr.clear();
        c->obs_idx.clear();
        c->d_obs_ptr.release();
        c->d_obs_idx.release();
        return rc;
    };
    c->d_obs_ptr.release();
    c->d_obs_idx.release();
    if (int rc = c->d_obs_ptr.alloc(c, (size_t)L + 1)) return without_table(rc);
    if (int rc = c->d_obs_idx.grow(c, c->obs_idx.size(), std::max<size_t>(1, c->obs_idx.size()))) return without_table(rc);
    if (hipMemcpy(c->d_obs_ptr.p, c->obs_ptr.data(), ((size_t)L + 1) * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_obs_idx.p, c->obs_idx.data(), c->obs_idx.size() * sizeof(int64_t), hipMemcpyHostToDevice) != hipSuccess)
        return without_table(fail(c, DSMGP_E_HIP, "append_rows: upload of the leaf table failed"));

    // 5. this call's one-shot marks: an owner that keeps blocks is a PREFIX leaf whose source is its own old factor (phase 1, z
    //    from the forward sweep); kb = every block for a leaf without additions, floor(n_old / 128) otherwise
    final_schedule();
    std::vector<int> factor_keep((size_t)L, 0);         // per factor owner: the leading blocks it keeps
    for (int l = 0; l < L; ++l) {
        LeafHost& lf = c->leaves[l];
        if (lf.op != DSMGP_SHARE_FULL) continue;
        const Old& mine = old[(size_t)l];
        const Old& from = old[(size_t)mine.owner];
        const int keep = old_info[(size_t)mine.owner] != 0 ? 0 : (adds_of(l) == 0 ? from.nb : from.n / TB);
        if (keep > 0) {
            lf.op = DSMGP_SHARE_PREFIX;
            lf.src = l;
            lf.prefix = (int64_t)keep * TB;
        }
        factor_keep[(size_t)l] = keep;
        if (keep == 0) st[4]++;
        else if (keep < lf.nb) st[0]++;
        st[3] += lf.nb - keep;
    }
    bool in_place = true;
    {
        size_t a = 0, b = 0, v = 0, x = 0;
        plan_layout(c, a, b, v, x);
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            const Old& o = old[(size_t)l];
            if (lf.owner != o.owner || lf.npad != o.npad || lf.f_off != o.f_off || lf.dinv_off != o.dinv_off) in_place = false;
        }
    }
    // (the lane deal of this plan weighs every owner by n^3 as a fit would, although a continuing owner costs O(n 128 n) and an
    // untouched one nothing: the lanes of this one call may be unevenly loaded -- speed only, and the lists are rebuilt below)
    if (int rc = in_place ? build_plan(c, std::move(oldF), std::move(oldDinv)) : build_plan(c)) return give_up(rc);
    if (int rc = upload_hyper(c)) return give_up(rc);
    if (int rc = ensure_phase(c)) return give_up(rc);      // this call's step lists: dropped below

    // 6. the kept blocks of every continuing owner, old arenas -> new ones: one task list, one launch
    DevBuf<RelocTask> reloc;
    if (!in_place) {
        std::vector<RelocTask> rt;
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.op != DSMGP_SHARE_PREFIX) continue;
            const Old& from = old[(size_t)old[(size_t)l].owner];
            const LeafDev& d = c->h_leaves[l];
            for (int j = 0; j < lf.kb; ++j) {
                for (int i = 0; i < lf.kb; ++i)
                    rt.push_back(RelocTask{oldF.p + from.f_off + (size_t)i * TB + (size_t)j * TB * from.npad,
                                           d.F + (size_t)i * TB + (size_t)j * TB * lf.npad, from.npad, lf.npad});
                rt.push_back(RelocTask{oldDinv.p + from.dinv_off + (size_t)j * TB * TB, d.Dinv + (size_t)j * TB * TB, TB, TB});
            }
        }
        st[2] = (int64_t)rt.size() * TB * TB * (int64_t)sizeof(double);
        if (int rc = dev_upload(c, reloc, rt)) return give_up(rc);
    } else {
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            const int o = lf.owner;
            if (adds_of(l) == 0 && adds_of(o) == 0 && lf.mean == old[(size_t)l].mean && old_info[(size_t)old[(size_t)l].owner] == 0) st[1]++;
        }
    }

    // 7. the launches of a fit, the relocation between its phases: the owners without kept blocks (there may be none) in phase
    //    0, the continuations in phase 1
    reset_fit_timings(c);
    PhaseTimer pt(c);
    EventPair ev;
    if (ev.init() != hipSuccess) return give_up(fail(c, DSMGP_E_HIP, "append_rows: hipEventCreate failed"));
    auto relocate = [&]() -> int {
        if (reloc.count) relocate_tiles_kernel<<<(unsigned)reloc.count, 256, 0, c->stream>>>(reloc.p);
        return 0;
    };
    auto run_fit = [&]() -> int {
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        if (int rc = enqueue_fit(c, c->phase, false, pt, relocate)) return rc;
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return 0;
    };
    if (int rc = run_fit()) {
        pt.collect();
        return give_up(rc);
    }
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, ev.a, ev.b);
    pt.collect(ev.a);
    c->timings[11] = ms * 1e-3;
    if (seconds) *seconds = ms * 1e-3;
    oldF.put();             // the old factors have been read for the last time (in place: the context has them)
    oldDinv.put();
    // (a failure from here on still goes through give_up: the one-shot marks never outlive the call.)  The read-back comes before
    // final_schedule() takes the marks away; its PREFIX correction changes nothing here, where a PREFIX leaf's source is itself.
    if (int rc = fetch_fit_results(c, mll_out, info_out)) return give_up(rc);
    c->mark(P_FIT);
    c->vt_from_fit = false;
    c->last_fit_joint = false;
    // 8. the marks go: the blocks this call's fused steps left without their whole inverse are completed under ITS lists, then
    //    the schedule lists are rebuilt as the next fit needs them (COPY where kept, FULL elsewhere) and the step lists dropped
    if (int rc = ensure_dinv(c)) return give_up(rc);
    if (hipStreamSynchronize(c->stream) != hipSuccess) return give_up(fail(c, DSMGP_E_HIP, "append_rows: hipStreamSynchronize failed"));
    final_schedule();
    {
        size_t a = 0, b = 0, v = 0, x = 0;
        plan_layout(c, a, b, v, x);
    }
    if (int rc = build_schedule(c)) return give_up(rc);
    c->invalidate(P_PHASE);
    for (int i = 0; i < DSMGP_N_APPEND_STATS; ++i) c->append_stats[i] = st[i];
    c->have_append_stats = true;
    // 9. the test set that stays: after the old factors have gone, so that the call's peak is the larger of "old + new factors +
    //    old K_tn L^-T" and "new factors + old + new K_tn L^-T".  The fit is good whatever happens here: a set that cannot be
    //    kept is dropped, as dsmgp_append_rows drops it, and the stats say so.
    if (keep_test) {
        int64_t rs[DSMGP_N_RESUME_STATS] = {0, 0, 0, -1, 0, 0};
        if (kt.resident && keep_test_set(c, kt, factor_keep, rs) != 0) {
            (void)hipStreamSynchronize(c->stream);
            free_test(c);
            const int64_t dropped[DSMGP_N_RESUME_STATS] = {0, 0, 0, -1, 0, 1};
            for (int i = 0; i < DSMGP_N_RESUME_STATS; ++i) rs[i] = dropped[i];
        }
        kt.arena.put();
        for (int i = 0; i < DSMGP_N_RESUME_STATS; ++i) c->resume_stats[i] = rs[i];
        c->have_resume_stats = true;
    }
    return 0;
}

int dsmgp_append_rows(dsmgp_ctx* c, const double* X_new, const double* y_new, int64_t m, int32_t D, const int64_t* add_ptr,
                      const int64_t* add_idx, const double* mean, double* mll_out, int32_t* info_out, double* seconds) {
    return grow_rows(c, X_new, y_new, m, D, add_ptr, add_idx, mean, mll_out, info_out, seconds, false);
}

int dsmgp_add_rows_keep_test(dsmgp_ctx* c, const double* X_new, const double* y_new, int64_t m, int32_t D, const int64_t* add_ptr,
                             const int64_t* add_idx, const double* mean, double* mll_out, int32_t* info_out, double* seconds) {
    return grow_rows(c, X_new, y_new, m, D, add_ptr, add_idx, mean, mll_out, info_out, seconds, true);
}

int dsmgp_resume_stats(dsmgp_ctx* c, int64_t* out) {
    if (!c || !out) return DSMGP_E_ARG;
    if (!c->have_resume_stats) return fail(c, DSMGP_E_STATE, "resume_stats before add_rows_keep_test");
    for (int i = 0; i < DSMGP_N_RESUME_STATS; ++i) out[i] = c->resume_stats[i];
    return 0;
}

int dsmgp_append_stats(dsmgp_ctx* c, int64_t* out) {
    if (!c || !out) return DSMGP_E_ARG;
    if (!c->have_append_stats) return fail(c, DSMGP_E_STATE, "append_stats before append_rows");
    for (int i = 0; i < DSMGP_N_APPEND_STATS; ++i) out[i] = c->append_stats[i];
    return 0;
}

// -------------------------------------------------------------------------------------------------
}  // extern "C"

namespace {
// Second half of a test-set registration, common to dsmgp_set_test (routes from the host) and dsmgp_set_test_routed (routes
// made on the device): per-leaf sizes from c->route_ptr, the K_tn arena, the gathered test rows, the task lists of the sweep.
// The first half has put the rows (dXt), the CSR (d_route_ptr / d_route_idx) and the per-row entry index (d_row_ptr / d_row_ent /
// d_ent_leaf) into HBM and the per-leaf row offsets into c->route_ptr.
int build_sweep_lists(dsmgp_ctx* c, HostLog& hl, const std::vector<int>& first);
int register_test(dsmgp_ctx* c, HostLog& hl, const std::vector<int>* first) {
    const int L = c->L;
    const int64_t n_t = c->n_t, total = c->route_total;
    const int64_t* rp = c->route_ptr.data();
    hl.lap("set_test: sizes");
    size_t vTot = 0, xTot = 0;
    size_t accTot = 0;
    for (int l = 0; l < L; ++l) accTot += (size_t)round_up((int)(rp[l + 1] - rp[l]), TB);
    const size_t pTot = 2 * (size_t)total + 2 * accTot + 2 * TB;
    for (int l = 0; l < L; ++l) {
        LeafHost& lf = c->leaves[l];
        lf.nt = (int)(rp[l + 1] - rp[l]);
        lf.ntpad = round_up(lf.nt, TB);
        lf.route_off = rp[l];
        lf.vt_off = vTot;
        vTot += (size_t)lf.ntpad * lf.npad;
        lf.xt_off = xTot;
        xTot += (size_t)lf.ntpad * c->D;
        lf.pv_off = (size_t)rp[l];   // mu / var of all leaves are contiguous in route order (unpadded)
    }
    size_t freeB = 0, totalB = 0;
    HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
    const size_t need = (vTot + xTot + pTot) * sizeof(double) + (size_t)n_t * c->D * sizeof(double);
    if (!c->pool.active()) freeB += (c->arenaVt.cap + c->arenaXt.cap + c->arenaPV.cap) * sizeof(double);   // taken over or released first (DevArena::fit)
    if (!c->pool.active() && need + (size_t(1) << 30) > freeB)
        return fail(c, DSMGP_E_NOMEM, "test set needs " + std::to_string(need >> 20) + " MiB, device has " +
                                          std::to_string(freeB >> 20) + " MiB free");
    hl.lap("set_test: arenas");
    // every arena of the test set this one replaces is taken over while it fits (and is not wastefully large: at most twice what
    // is needed); with a device pool they are carved out of the pool's stack
    if (int rc = arena_status(c, c->arenaVt.fit(arena_pool(c), vTot))) return rc;
    if (int rc = arena_status(c, c->arenaXt.fit(arena_pool(c), xTot))) return rc;
    if (int rc = arena_status(c, c->arenaPV.fit(arena_pool(c), pTot))) return rc;
    int maxpad = 0;
    size_t accOff = 0;
    c->acc_off = 2 * (size_t)total;
    c->acc_count = 2 * accTot;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        LeafDev& d = c->h_leaves[l];
        d.Vt = c->arenaVt.p + lf.vt_off;
        d.Xtg = c->arenaXt.p + lf.xt_off;
        d.mu = c->arenaPV.p + lf.pv_off;
        d.var = c->arenaPV.p + (size_t)total + lf.pv_off;
        d.macc = c->arenaPV.p + 2 * (size_t)total + accOff;
        d.sacc = d.macc + accTot;
        d.zfused = (lf.owner == l && lf.op == DSMGP_SHARE_FULL) ? 1 : 0;
        accOff += (size_t)lf.ntpad;
        d.nt = lf.nt;
        d.ntpad = lf.ntpad;
        maxpad = std::max(maxpad, lf.ntpad);
    }
    if (int rc = stage_upload(c, c->d_leaves.p, c->h_leaves.data(), (size_t)L * sizeof(LeafDev))) return rc;
    if (maxpad > 0) {
        for_leaf_chunks((size_t)L, [&](size_t leaf0, size_t cnt) {
            gather_test_kernel<<<dim3((maxpad + 255) / 256, (unsigned)cnt), 256, 0, c->stream>>>(
                c->d_leaves.p, c->d_route_ptr.p, c->d_route_idx.p, c->dXt.p, n_t, c->D, (int)leaf0);
        });
        HIPCHK(c, hipGetLastError());
    }
    {
        const std::vector<int> zero((size_t)L, 0);
        if (int rc = build_sweep_lists(c, hl, first ? *first : zero)) return rc;
    }
    // The same test rows as riders of the factorisation launches (used by fit while this test set is resident).  With a device
    // pool (the streaming context: the pool is a stack, plan < test < gradients, and a fit follows at once) the lists are built
    // here; otherwise by the first fit that wants them (ensure_joint) -- predict(model, x) on rows the model has not seen
    // registers them and runs its own sweep, and should not wait for task lists only a later fit! would use (0.067 s of the
    // 0.088 s this call took at the headline model).
    c->mark(P_TEST);
    int rc = c->pool.active() ? ensure_joint(c) : 0;
    hl.lap("set_test: final sync");
    if (rc == 0) rc = stage_done(c);
    if (rc != 0) c->invalidate(P_TEST);
    return rc;
}

// The task lists of the standalone sweep over the registered rows.  first[l]: the block step leaf l's sweep begins at -- zeros for
// a registration; what dsmgp_add_rows_keep_test kept of the leaf's K_tn L^-T otherwise: steps k < first[l] have no task of any
// kind (no K_tn tile either: block columns below first[l] are never written), block column first[l] is written whole like every
// later one, and the moment sums over the columns the sweep does not visit come from kept_sums_kernel (dsmgp_predict_run).
int build_sweep_lists(dsmgp_ctx* c, HostLog& hl, const std::vector<int>& first) {
    const int L = c->L;
    hl.lap("set_test: task lists (host)");
    // task lists
    // In the block steps that a fit runs fused (many leaves, or shallow: build_plan) the sweep does too: one tile_fused8_kernel
    // launch whose tasks evaluate K_tn themselves, update and solve eight 16-row blocks of test rows each and write them once
    // -- the routed rows of a small leaf are a fraction of a 128-row tile (44 of 128 at depth 4), which the update / panel
    // solve launches of the other steps execute in full.  A COPY leaf goes with its source's group, as in the factorisation.
    auto fused_at = [&](int l, int k) {
        const std::vector<char>& fs = c->fused_step[(int)c->leaf_group[l]];
        return gram_fused(c) && k < (int)fs.size() && fs[(size_t)k] == STEP_FUSED;
    };
    std::vector<GramTask> pg, pg0;  // K_tn tiles the sweep reads from memory (block column 0 of the classic steps; every column where the
                                    // update tasks cannot evaluate them: D > 32); those of block column 0 for the joint fit
    std::vector<PredTask> ptk, ptk_slow;
    int nsteps = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        nsteps = std::max(nsteps, lf.nb);
        const LeafDev& d = c->h_leaves[l];
        for (int ti = 0; ti < lf.ntpad / TB; ++ti) {
            ptk.push_back(PredTask{l, ti * TB});
            if (!d.zfused) ptk_slow.push_back(PredTask{l, ti * TB});
            for (int j = 0; j < lf.nb; ++j) {
                if (fused_at(l, j)) continue;       // evaluated inside the fused tasks (sweep and joint fit alike)
                if (j > 0 && gram_fused(c)) continue;   // ... and inside the update tasks of the classic steps (TileTask.gram)
                GramTask g{};
                g.xa = d.Xtg + (size_t)ti * TB;
                g.xb = d.Xg + (size_t)j * TB;
                g.out = d.Vt + (size_t)ti * TB + (size_t)j * TB * lf.ntpad;
                g.lda = lf.ntpad;
                g.ldb = lf.npad;
                g.ldo = lf.ntpad;
                g.na = std::max(0, std::min(TB, lf.nt - ti * TB));
                g.nb = std::max(0, std::min(TB, lf.n - j * TB));
                g.sym = 0;
                g.diag = 0;
                g.kid = lf.kid;
                if (j >= first[(size_t)l]) pg.push_back(g);
                if (j == 0) pg0.push_back(g);
            }
        }
    }
    // the sweep runs lane by lane like the factorisation (SweepLists)
    const int nl = c->nlanes, nv = nl * nsteps;
    std::vector<SweepLane> lanes = sweep_lanes(c, nl, nsteps);
    std::vector<int>& f8_off = c->psweep.f8_off;
    f8_off.assign((size_t)nv + 1, 0);
    // Fused steps: the tasks are made on the device (build_sweep8_kernel) from one SweepSeg per (leaf, step); the host counts them
    // per step -- a leaf of nt routed rows has ceil(ceil(nt / 16) / 8) tasks in each of its fused steps -- and says where each
    // pair's tasks start.  Classic steps: the leaves that have them, per step (few: the largest leaves of a many-leaf model,
    // all leaves beyond the shallow steps of a model with few).
    std::vector<SweepSeg> segs;
    std::vector<std::vector<int>> classic((size_t)nv);
    {
        std::vector<int> cnt8((size_t)nv, 0);
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.nt == 0) continue;
            const int nt8 = ((lf.nt + 15) / 16 + 7) / 8;
            const size_t v0 = (size_t)c->leaf_lane[l] * (size_t)nsteps;
            for (int k = first[(size_t)l]; k < lf.nb; ++k) {
                if (fused_at(l, k)) cnt8[v0 + (size_t)k] += nt8;
                else classic[v0 + (size_t)k].push_back(l);
            }
        }
        // (The K_tn arena is NOT cleared.  Rounds 1-4 zeroed it at every registration because the update / panel-solve tiles of
        // the classic steps read and write whole 128-row tiles while the Gram kernel writes data rows only -- but a row of a tile
        // product depends on its own row of the first operand alone, every rider sums per row, and nothing reads a row beyond a
        // leaf's routed ones (pred_finish / pred_mu / pred_var stop at nt): what sits in the padding rows never reaches a result.
        // Clearing cost more than its own time: 9.6 GB per registration at depth 4.)
        for (int v = 0; v < nv; ++v) f8_off[(size_t)v + 1] = f8_off[(size_t)v] + cnt8[(size_t)v];
        std::vector<int> cursor((size_t)nv, 0);
        segs.reserve((size_t)L * 4);
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.nt == 0) continue;
            const int nt8 = ((lf.nt + 15) / 16 + 7) / 8;
            const size_t v0 = (size_t)c->leaf_lane[l] * (size_t)nsteps;
            for (int k = first[(size_t)l]; k < lf.nb; ++k)
                if (fused_at(l, k)) {
                    SweepSeg sg{};
                    sg.leaf = l;
                    sg.k = k;
                    sg.src0 = cursor[v0 + (size_t)k];
                    sg.begin = f8_off[v0 + (size_t)k];
                    sg.n = cnt8[v0 + (size_t)k];
                    segs.push_back(sg);
                    cursor[v0 + (size_t)k] += nt8;
                }
        }
    }
    // (the lanes' lists are independent: one host thread per lane -- 90k tile tasks at the headline model, 10 ms on one thread)
    auto build_lane = [&](int lane) {
      for (int k = 0; k < nsteps; ++k) {
        const int v = lane * nsteps + k;
        SweepLane& ln = lanes[(size_t)lane];
        ln.mark(k);
        std::vector<TileTask> tiles;
        for (int l : classic[(size_t)v]) {
            const LeafHost& lf = c->leaves[l];
            const LeafDev& d = c->h_leaves[l];
            for (int ti = 0; ti < lf.ntpad / TB; ++ti) {
                double* tile = d.Vt + (size_t)ti * TB + (size_t)k * TB * lf.ntpad;
                if (k > 0) {
                    TileTask u{};
                    u.A = d.Vt + (size_t)ti * TB;
                    u.B = d.F + (size_t)k * TB;
                    u.C = tile;
                    u.lda = lf.ntpad;
                    u.ldb = lf.npad;
                    u.ldc = lf.ntpad;
                    u.k0 = 0;
                    u.k1 = k * TB;
                    u.update = 1;
                    u.mrows = tile_mrows(lf.nt - ti * TB);
                    if (gram_fused(c)) {    // the task evaluates its K_tn tile itself, as in the joint fit: only block column 0 of
                        u.gram = 1;         // K_tn ever exists in memory
                        u.kid = lf.kid;
                        u.gxa = d.Xtg + (size_t)ti * TB;
                        u.gxb = d.Xg + (size_t)k * TB;
                        u.glda = lf.ntpad;
                        u.gldb = lf.npad;
                        u.gna = std::max(0, std::min(TB, lf.nt - ti * TB));
                        u.gnb = std::max(0, std::min(TB, lf.n - k * TB));
                    }
                    tiles.push_back(u);
                }
                TileTask s{};
                s.A = tile;
                s.B = d.Dinv + (size_t)k * TB * TB;
                s.C = tile;
                s.lda = lf.ntpad;
                s.ldb = TB;
                s.ldc = lf.ntpad;
                s.k0 = 0;
                s.k1 = TB;
                s.update = 0;
                s.mrows = tile_mrows(lf.nt - ti * TB);
                s.zk = d.z + (size_t)k * TB;           // predictive mean and variance ride along
                s.wi = d.macc + (size_t)ti * TB;
                s.sq = d.sacc + (size_t)ti * TB;
                ln.trsm.push_back(s);
            }
        }
        ln.U.add_step(tiles, k * TB);
      }
    };
    {
        // nothing may throw across the ABI, and nothing may leave a worker thread (std::terminate) or unwind past a joinable one:
        // every lane's build runs inside a catch that records the failure (bad_alloc from the 90k-task vectors of a large
        // registration), the workers are joined first, then the call returns DSMGP_E_NOMEM
        std::atomic<bool> lane_failed{false};
        auto build_lane_safe = [&](int q) {
            try {
                build_lane(q);
            } catch (...) {
                lane_failed.store(true);
            }
        };
        std::vector<std::thread> th;
        int started = 1;                    // lanes [1, started) have a thread of their own
        try {
            for (int q = 1; q < nl; ++q) {
                th.emplace_back(build_lane_safe, q);
                started = q + 1;
            }
        } catch (...) {                     // no thread to be had: the remaining lanes are built here
        }
        build_lane_safe(0);
        for (std::thread& t : th) t.join();
        for (int q = started; q < nl; ++q) build_lane_safe(q);
        if (lane_failed.load()) return fail(c, DSMGP_E_NOMEM, "set_test: out of host memory while building the sweep's task lists");
    }
    hl.lap("set_test: task uploads");
    if (int rc = stage_upload_list(c, c->psegs, segs)) return rc;
    if (int rc = dev_reserve(c, c->psweep.f8, (size_t)f8_off[(size_t)nv])) return rc;
    if (!segs.empty())
        build_sweep8_kernel<<<(unsigned)((segs.size() + 127) / 128), 128, 0, c->stream>>>(c->psegs.p, (int)segs.size(), c->d_leaves.p, c->psweep.f8.p,
                                                                                        c->xcd_order ? 1 : 0);
    HIPCHK(c, hipGetLastError());
    if (int rc = pack_sweep(c, c->psweep, lanes, stage_upload)) return rc;
    if (int rc = stage_upload_list(c, c->pgram, pg)) return rc;
    if (int rc = stage_upload_list(c, c->pgram0, pg0)) return rc;
    if (int rc = stage_upload_list(c, c->ptasks, ptk)) return rc;
    if (int rc = stage_upload_list(c, c->ptasks_slow, ptk_slow)) return rc;
    // the sums over the kept columns: per (leaf, row tile) chunks of KEPT_CHUNK_BLOCKS block columns, real columns only (a leaf
    // without additions keeps its last, partial block column)
    std::vector<KeptSumTask> ks;
    std::vector<KeptFinTask> kf;
    const int chunk = KEPT_CHUNK_BLOCKS * TB;
    auto kept_cols = [&](int l) { return c->leaves[l].nt == 0 ? 0 : std::min(first[(size_t)l] * TB, c->leaves[l].n); };
    size_t nchunk = 0;
    for (int l = 0; l < L; ++l) nchunk += (size_t)(c->leaves[l].ntpad / TB) * (size_t)((kept_cols(l) + chunk - 1) / chunk);
    if (int rc = dev_reserve(c, c->d_kept_part, nchunk * 2 * TB)) return rc;
    bool any = false;
    for (int l = 0; l < L; ++l) {
        const int ncols = kept_cols(l);
        if (ncols == 0) continue;
        any = true;
        const LeafHost& lf = c->leaves[l];
        const LeafDev& d = c->h_leaves[l];
        for (int ti = 0; ti < lf.ntpad / TB; ++ti) {
            double* part = c->d_kept_part.p + ks.size() * 2 * TB;
            kf.push_back(KeptFinTask{part, d.macc + (size_t)ti * TB, d.sacc + (size_t)ti * TB, (ncols + chunk - 1) / chunk, 0});
            for (int c0 = 0; c0 < ncols; c0 += chunk, part += 2 * TB)
                ks.push_back(KeptSumTask{d.Vt + (size_t)ti * TB + (size_t)c0 * (size_t)lf.ntpad, d.z + c0, part, lf.ntpad,
                                         std::min(chunk, ncols - c0), std::max(0, std::min(TB, lf.nt - ti * TB)), 0});
        }
    }
    if (int rc = stage_upload_list(c, c->kept_tasks, ks)) return rc;
    if (int rc = stage_upload_list(c, c->kept_fin, kf)) return rc;
    c->sweep_resumed = any;
    return 0;
}

// The sweep's lists from block 0 again, where the resident ones skip what dsmgp_add_rows_keep_test had kept
int full_sweep_lists(dsmgp_ctx* c) {
    if (!c->sweep_resumed) return 0;
    drop_graphs(c);
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    HostLog hl("sweep lists from block 0");
    const std::vector<int> zero((size_t)c->L, 0);
    if (int rc = build_sweep_lists(c, hl, zero)) return rc;
    return stage_done(c);
}
}  // namespace

extern "C" {

int dsmgp_set_test(dsmgp_ctx* c, const double* Xt, int64_t n_t, int32_t D, const int64_t* route_ptr, const int64_t* route_idx) {
    if (!c) return DSMGP_E_ARG;
    if (c->L == 0) return fail(c, DSMGP_E_STATE, "set_test before set_leaves");
    if (!Xt || n_t <= 0 || !route_ptr) return fail(c, DSMGP_E_ARG, "set_test: bad arguments");
    if (D != c->D) return fail(c, DSMGP_E_ARG, "set_test: the test matrix has " + std::to_string(D) + " columns, the training data " + std::to_string(c->D));
    HIPCHK(c, hipSetDevice(c->device));
    HostLog hl_total("set_test");
    if (int rc = build_plan(c)) return rc;
    HostLog hl("set_test: free old");
    free_test(c, true);     // every buffer of the set this one replaces is kept for it
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    hl.lap("set_test: validate");
    const int L = c->L;
    if (route_ptr[0] != 0) return fail(c, DSMGP_E_ARG, "route_ptr[0] must be 0");
    const int64_t total = route_ptr[L];
    if (total > 0 && !route_idx) return fail(c, DSMGP_E_ARG, "route_idx is NULL");
    for (int l = 0; l < L; ++l)
        if (route_ptr[l + 1] < route_ptr[l]) return fail(c, DSMGP_E_ARG, "route_ptr must be non-decreasing");
    for (int64_t i = 0; i < total; ++i)
        if (route_idx[i] < 0 || route_idx[i] >= n_t) return fail(c, DSMGP_E_ARG, "route index out of range");
    c->n_t = n_t;
    c->route_total = total;
    c->route_ptr.assign(route_ptr, route_ptr + L + 1);
    hl.lap("set_test: uploads + row index");
    if (int rc = c->dXt.grow(c, (size_t)n_t * c->D)) return rc;
    HIPCHK(c, hipMemcpy(c->dXt.p, Xt, (size_t)n_t * c->D * sizeof(double), hipMemcpyHostToDevice));
    if (int rc = c->d_route_ptr.grow(c, (size_t)L + 1)) return rc;
    HIPCHK(c, hipMemcpy(c->d_route_ptr.p, route_ptr, (L + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (int rc = c->d_route_idx.grow(c, (size_t)total)) return rc;
    if (total) HIPCHK(c, hipMemcpy(c->d_route_idx.p, route_idx, total * sizeof(int64_t), hipMemcpyHostToDevice));
    {
        // per test row, the (leaf, row) entries that carry its moments, in ascending entry order (= leaf order):
        // the index agg_partial_kernel walks
        if (total > (int64_t)INT32_MAX) return fail(c, DSMGP_E_ARG, "set_test: more than 2^31 routed rows");
        std::vector<int64_t> rptr((size_t)n_t + 1, 0);
        for (int64_t i = 0; i < total; ++i) rptr[route_idx[i] + 1]++;
        for (int64_t r = 0; r < n_t; ++r) rptr[r + 1] += rptr[r];
        std::vector<int32_t> rent((size_t)std::max<int64_t>(1, total)), eleaf((size_t)std::max<int64_t>(1, total));
        std::vector<int64_t> fill(rptr.begin(), rptr.end() - 1);
        for (int l = 0; l < L; ++l)
            for (int64_t i = route_ptr[l]; i < route_ptr[l + 1]; ++i) {
                rent[fill[route_idx[i]]++] = (int32_t)i;
                eleaf[i] = l;
            }
        if (int rc = c->d_row_ptr.grow(c, (size_t)n_t + 1)) return rc;
        if (int rc = c->d_row_ent.grow(c, rent.size())) return rc;
        if (int rc = c->d_ent_leaf.grow(c, eleaf.size())) return rc;
        HIPCHK(c, hipMemcpy(c->d_row_ptr.p, rptr.data(), rptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_row_ent.p, rent.data(), rent.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(c->d_ent_leaf.p, eleaf.data(), eleaf.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return register_test(c, hl);
}


// ---- routing on the device --------------------------------------------------------------------------------------------------
int dsmgp_set_tree(dsmgp_ctx* c, int64_t n_nodes, const int8_t* kind, const int64_t* first_child, const int64_t* n_child,
                   const int64_t* split_dim, const double* thr, int64_t thr_ld, const int64_t* leaf_id) {
    if (!c) return DSMGP_E_ARG;
    if (c->L == 0) return fail(c, DSMGP_E_STATE, "set_tree before set_leaves");
    if (n_nodes <= 0 || n_nodes > (int64_t)INT32_MAX || !kind || !first_child || !n_child || !split_dim || !thr || !leaf_id || thr_ld <= 0)
        return fail(c, DSMGP_E_ARG, "set_tree: bad arguments");
    std::vector<int32_t> first((size_t)n_nodes), nch((size_t)n_nodes), sdim((size_t)n_nodes), leaf((size_t)n_nodes), need((size_t)n_nodes, 0);
    int max_leaf = -1;
    for (int64_t i = 0; i < n_nodes; ++i) {
        if (kind[i] < 0 || kind[i] > 2) return fail(c, DSMGP_E_ARG, "set_tree: unknown node kind");
        if (kind[i] == 0) {
            if (leaf_id[i] < -1 || leaf_id[i] >= c->L) return fail(c, DSMGP_E_ARG, "set_tree: a region names a leaf outside the leaf table");
            max_leaf = std::max(max_leaf, (int)leaf_id[i]);
        } else if (n_child[i] <= 0 || first_child[i] <= i || first_child[i] + n_child[i] > n_nodes) {
            return fail(c, DSMGP_E_ARG, "set_tree: children must follow their parent, consecutively");
        }
        if (kind[i] == 1 && (n_child[i] > thr_ld || split_dim[i] < 0 || split_dim[i] >= c->D))
            return fail(c, DSMGP_E_ARG, "set_tree: a split node needs a threshold per child and a split dimension below D");
        first[(size_t)i] = (int32_t)first_child[i];
        nch[(size_t)i] = (int32_t)n_child[i];
        sdim[(size_t)i] = (int32_t)split_dim[i];
        leaf[(size_t)i] = kind[i] == 0 ? (int32_t)leaf_id[i] : -1;
    }
    // pending nodes of a row's depth-first walk (route_walk_row's stack)
    const int stack_need = route_stack_need(n_nodes, kind, first.data(), nch.data(), need.data());
    if (stack_need > ROUTE_STACK)
        return fail(c, DSMGP_E_ARG, "set_tree: the tree needs " + std::to_string(stack_need) + " pending nodes per row, the walk holds " +
                                        std::to_string(ROUTE_STACK));
    // The device path keeps one bit per (leaf, row) and writes a row's entries in the order its walk meets them, where the
    // host registration orders them by leaf: the two agree only when the walk (depth-first, children in order) meets the held
    // leaves in strictly ascending order.
    {
        std::vector<char> seen((size_t)c->L, 0);
        std::vector<int32_t> pending(1, 0);
        int last = -1;
        int64_t met = 0;
        while (!pending.empty()) {
            const int32_t i = pending.back();
            pending.pop_back();
            if (++met > n_nodes) return fail(c, DSMGP_E_ARG, "set_tree: a node is the child of two parents");
            if (kind[i] != 0) {
                for (int32_t j = nch[(size_t)i] - 1; j >= 0; --j) pending.push_back(first[(size_t)i] + j);
                continue;
            }
            const int l = leaf[(size_t)i];
            if (l < 0) continue;
            if (seen[(size_t)l]) return fail(c, DSMGP_E_ARG, "set_tree: leaf " + std::to_string(l) + " is named twice; the device routing holds a leaf once per row");
            if (l < last)
                return fail(c, DSMGP_E_ARG, "set_tree: the leaves are not numbered depth-first (leaf " + std::to_string(l) + " follows leaf " +
                                                std::to_string(last) + "); the device routing needs them ascending along the walk");
            seen[(size_t)l] = 1;
            last = l;
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    free_tree(c);
    auto up = [&](auto& buf, const auto* src, size_t n) -> int {
        if (int rc = buf.alloc(c, n)) return rc;
        HIPCHK(c, hipMemcpy(buf.p, src, n * sizeof(*src), hipMemcpyHostToDevice));
        return 0;
    };
    if (int rc = up(c->rt_kind, kind, (size_t)n_nodes)) return rc;
    if (int rc = up(c->rt_first, first.data(), (size_t)n_nodes)) return rc;
    if (int rc = up(c->rt_nchild, nch.data(), (size_t)n_nodes)) return rc;
    if (int rc = up(c->rt_sdim, sdim.data(), (size_t)n_nodes)) return rc;
    if (int rc = up(c->rt_leaf, leaf.data(), (size_t)n_nodes)) return rc;
    if (int rc = up(c->rt_thr, thr, (size_t)n_nodes * (size_t)thr_ld)) return rc;
    c->rtree = RouteTree{c->rt_kind.p, c->rt_first.p, c->rt_nchild.p, c->rt_sdim.p, c->rt_leaf.p, c->rt_thr.p, (int)thr_ld};
    c->rtree_nodes = n_nodes;
    c->rtree_max_leaf = max_leaf;
    c->mark(P_RTREE);
    return 0;
}

int dsmgp_set_test_routed(dsmgp_ctx* c, const double* Xt, int64_t n_t, int32_t D) {
    if (!c) return DSMGP_E_ARG;
    if (c->L == 0) return fail(c, DSMGP_E_STATE, "set_test before set_leaves");
    if (!c->has(P_RTREE)) return fail(c, DSMGP_E_STATE, "set_test_routed before set_tree");
    if (!Xt || n_t <= 0) return fail(c, DSMGP_E_ARG, "set_test_routed: bad arguments");
    if (D != c->D) return fail(c, DSMGP_E_ARG, "set_test_routed: the test matrix has " + std::to_string(D) + " columns, the training data " + std::to_string(c->D));
    HIPCHK(c, hipSetDevice(c->device));
    HostLog hl_total("set_test_routed");
    if (int rc = build_plan(c)) return rc;
    HostLog hl("set_test: free old");
    free_test(c, true);
    c->stage_top = 0;
    hl.lap("set_test: route on the device");
    const int L = c->L;
    const int64_t wpl = (n_t + 31) / 32;
    const size_t nbits = (size_t)L * (size_t)wpl;
    if (nbits * 8 > (size_t(8) << 30)) return fail(c, DSMGP_E_NOMEM, "set_test_routed: routing bitmap above 8 GiB; route on the host (dsmgp_set_test)");
    const size_t ncounts = (size_t)n_t + (size_t)L + 1;
    if (int rc = c->rws_counts.grow(c, ncounts, ncounts + ncounts / 4)) return rc;
    if (int rc = c->rws_bits.grow(c, 2 * nbits, 2 * nbits + nbits / 2)) return rc;
    int32_t* row_cnt = c->rws_counts.p;
    int32_t* leaf_cnt = row_cnt + n_t;
    int* outside = reinterpret_cast<int*>(leaf_cnt + L);
    uint32_t* bitmap = c->rws_bits.p;
    uint32_t* wprefix = bitmap + nbits;
    if (int rc = c->dXt.grow(c, (size_t)n_t * c->D)) return rc;
    if (int rc = stage_upload(c, c->dXt.p, Xt, (size_t)n_t * c->D * sizeof(double))) return rc;
    if (int rc = c->d_route_ptr.grow(c, (size_t)L + 1)) return rc;
    if (int rc = c->d_row_ptr.grow(c, (size_t)n_t + 1)) return rc;
    HIPCHK(c, hipMemsetAsync(bitmap, 0, nbits * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(outside, 0, sizeof(int), c->stream));
    const unsigned gr = (unsigned)((n_t + 255) / 256);
    route_walk_kernel<false><<<gr, 256, 0, c->stream>>>(c->rtree, c->dXt.p, n_t, row_cnt, bitmap, wpl, outside, nullptr, nullptr, nullptr, nullptr);
    scan_counts_kernel<<<1, 1024, 0, c->stream>>>(row_cnt, n_t, c->d_row_ptr.p);
    route_rank_kernel<<<L, 256, 0, c->stream>>>(bitmap, wpl, wprefix, leaf_cnt);
    scan_counts_kernel<<<1, 1024, 0, c->stream>>>(leaf_cnt, (int64_t)L, c->d_route_ptr.p);
    HIPCHK(c, hipGetLastError());
    c->route_ptr.assign((size_t)L + 1, 0);
    int flag = 0;
    HIPCHK(c, hipMemcpyAsync(c->route_ptr.data(), c->d_route_ptr.p, ((size_t)L + 1) * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&flag, outside, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (flag != 0) {
        free_test(c);
        return fail(c, DSMGP_E_DOMAIN, "set_test_routed: a test row lies outside the region of a split node (the reference loops forever there)");
    }
    const int64_t total = c->route_ptr[(size_t)L];
    if (total > (int64_t)INT32_MAX) {
        free_test(c);
        return fail(c, DSMGP_E_ARG, "set_test: more than 2^31 routed rows");
    }
    c->n_t = n_t;
    c->route_total = total;
    if (int rc = c->d_route_idx.grow(c, (size_t)total)) return rc;
    if (int rc = c->d_row_ent.grow(c, (size_t)total)) return rc;
    if (int rc = c->d_ent_leaf.grow(c, (size_t)total)) return rc;
    route_fill_kernel<<<L, 256, 0, c->stream>>>(bitmap, wpl, wprefix, c->d_route_ptr.p, c->d_route_idx.p, c->d_ent_leaf.p);
    route_walk_kernel<true><<<gr, 256, 0, c->stream>>>(c->rtree, c->dXt.p, n_t, nullptr, bitmap, wpl, nullptr, c->d_row_ptr.p, c->d_route_ptr.p, wprefix,
                                                       c->d_row_ent.p);
    HIPCHK(c, hipGetLastError());
    return register_test(c, hl);
}

int dsmgp_routes(dsmgp_ctx* c, int64_t* route_ptr, int64_t* route_idx) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_TEST)) return fail(c, DSMGP_E_STATE, "routes before set_test");
    HIPCHK(c, hipSetDevice(c->device));
    if (route_ptr) std::memcpy(route_ptr, c->route_ptr.data(), ((size_t)c->L + 1) * sizeof(int64_t));
    if (route_idx && c->route_total)
        HIPCHK(c, hipMemcpy(route_idx, c->d_route_idx.p, (size_t)c->route_total * sizeof(int64_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"

namespace {
// A sweep (SweepLists) on the lanes' streams, step by step, lanes inner: per (lane, step) the fused 8-block tasks, the update
// launch with its split-K reduce, the panel solves.  pt: spans in slots 7 (fused tasks, updates) and 8 (panel solves), or none.
int run_sweep(dsmgp_ctx* c, const SweepLists& S, PhaseTimer* pt) {
    if (int rc = fork_lanes(c, S.nlanes)) return rc;
    for (int k = 0; k < S.nsteps; ++k)
        for (int lane = 0; lane < S.nlanes; ++lane) {
            const int v = lane * S.nsteps + k;
            const hipStream_t st = c->lane_stream[lane];
            const int n8 = S.f8_off.empty() ? 0 : S.f8_off[v + 1] - S.f8_off[v];
            if (n8 > 0) {
                if (pt) pt->begin(7, st);
                tile_fused8_kernel<1><<<n8, 512, 0, st>>>(S.f8.p + S.f8_off[v], c->d_kp.p, c->D);
                if (pt) pt->end(st);
            }
            const int nu = S.upd_off[v + 1] - S.upd_off[v];
            if (nu > 0) {
                if (pt) pt->begin(7, st);
                launch_tiles(c, S.upd.p + S.upd_off[v], nu, 0, false, 0, nullptr, 0, st);
                const int nr = S.red_off[v + 1] - S.red_off[v];
                if (nr > 0) tile_reduce_kernel<<<nr * REDUCE_WGS, 256, 0, st>>>(S.red.p + S.red_off[v]);
                if (pt) pt->end(st);
            }
            const int ns = S.trsm_off[v + 1] - S.trsm_off[v];
            if (ns > 0) {
                if (pt) pt->begin(8, st);
                launch_tiles(c, S.trsm.p + S.trsm_off[v], ns, 1, false, 0, nullptr, 0, st);
                if (pt) pt->end(st);
            }
        }
    return join_lanes(c, S.nlanes);
}
}  // namespace

extern "C" {

int dsmgp_predict_run(dsmgp_ctx* c, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "predict before fit");
    if (!c->has(P_TEST)) return fail(c, DSMGP_E_STATE, "predict before set_test");
    HIPCHK(c, hipSetDevice(c->device));
    for (int i = 6; i < 10; ++i) c->timings[i] = 0.0;
    c->timings[12] = 0.0;
    HostLog hl("predict_run: events");
    PhaseTimer pt(c);
    EventPair ev;
    HIPCHK(c, ev.init());
    const hipEvent_t t0 = ev.a, t1 = ev.b;
    HIPCHK(c, hipEventRecord(t0, c->stream));
    hl.lap("predict_run: enqueue");
    if (c->ptasks.count) {
        const bool standalone = !c->has(P_VT);
        if (standalone) {
            // after dsmgp_add_rows_keep_test the sweep resumes where the kept block columns end, once; any other sweep begins at 0
            const bool resume = c->resume_armed;
            if (!resume)
                if (int rc = full_sweep_lists(c)) return rc;
            if (int rc = ensure_dinv(c)) return rc;       // the panel solves of the sweep multiply with Dinv_k
            HIPCHK(c, hipMemsetAsync(c->arenaPV.p + c->acc_off, 0, c->acc_count * sizeof(double), c->stream));
            if (resume && c->kept_tasks.count) {          // ... and the sums of the columns it skips are stored over the zeros
                pt.begin(9);
                kept_sums_kernel<<<(unsigned)c->kept_tasks.count, 256, 0, c->stream>>>(c->kept_tasks.p);
                kept_sums_finish_kernel<<<(unsigned)c->kept_fin.count, 128, 0, c->stream>>>(c->kept_fin.p);
                pt.end();
            }
            if (resume) {
                int64_t swept = 0;
                for (int l = 0; l < c->L; ++l)
                    if (c->leaves[l].nt > 0) swept += c->leaves[l].nb - c->vt_first[(size_t)l];
                c->resume_stats[3] = swept;
                c->resume_armed = false;
            }
            // K_tn tiles of the classic steps                (src/gaussianprocess.jl:133)
            if (c->pgram.count) {
                pt.begin(6);
                gram_tile_kernel<<<2 * (int)c->pgram.count, 256, 0, c->stream>>>(c->pgram.p, c->d_kp.p, c->D);
                pt.end();
            }
            // V^T = K_tn L^-T, block column by block column (src/gaussianprocess.jl:120), lane by lane on the lanes' streams
            if (int rc = run_sweep(c, c->psweep, &pt)) return rc;
            c->mark(P_VT);
            c->vt_from_fit = false;
        }
        // mu = m + V^T z (= m + K_tn alpha), var = diag(Ktt - V'V) + noise   (src/gaussianprocess.jl:117-126):
        // both sums were accumulated by the panel-solve epilogues of the sweep; leaves whose z did not exist yet
        // while their rows rode through the factorisation (COPY / PREFIX) are finished from the stored rows
        pt.begin(9);
        pred_finish_kernel<<<(int)c->ptasks.count, 128, 0, c->stream>>>(c->d_leaves.p, c->ptasks.p, c->d_kp.p, c->D);
        // (only where the rows rode through the fit: a repeated call after the standalone sweep finds the sweep's sums of EVERY
        // leaf in the accumulators, and finishing COPY / PREFIX leaves from the stored rows instead would change their bits)
        if (!standalone && c->vt_from_fit && c->ptasks_slow.count) {
            pred_mu_kernel<<<(int)c->ptasks_slow.count, 256, 0, c->stream>>>(c->d_leaves.p, c->ptasks_slow.p);
            pred_var_kernel<<<(int)c->ptasks_slow.count, 256, 0, c->stream>>>(c->d_leaves.p, c->ptasks_slow.p, c->d_kp.p, c->D);
        }
        pt.end();
    } else {
        c->mark(P_VT);              // no routed rows at all: K_tn L^-T is empty, and current (predict_cov / predict_gradients: nothing written)
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(t1, c->stream));
    hl.lap("predict_run: wait");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    hl.done();
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
    pt.collect();
    c->timings[12] = ms * 1e-3;
    if (seconds) *seconds = ms * 1e-3;
    c->invalidate(P_PRED);
    c->mark(P_PRED);
    return 0;
}

int dsmgp_predict_fetch(dsmgp_ctx* c, double* mu_out, double* var_out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "predict_fetch before predict_run");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->route_total;
    if (n && mu_out) HIPCHK(c, hipMemcpyAsync(mu_out, c->arenaPV.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (n && var_out) HIPCHK(c, hipMemcpyAsync(var_out, c->arenaPV.p + n, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

// Inspection: K_tn L^-T of one leaf over its routed rows and its n real columns, as the sweep left it
int dsmgp_download_vt(dsmgp_ctx* c, int32_t leaf, double* V_out, int64_t ld) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "download_vt before predict_run on the current fit");
    if (leaf < 0 || leaf >= c->L) return fail(c, DSMGP_E_ARG, "download_vt: leaf out of range");
    const LeafHost& lf = c->leaves[leaf];
    if (lf.nt == 0) return 0;
    if (!V_out || ld < lf.nt) return fail(c, DSMGP_E_ARG, "download_vt: V_out is NULL or ld < nt");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2D(V_out, (size_t)ld * sizeof(double), c->h_leaves[leaf].Vt, (size_t)lf.ntpad * sizeof(double),
                          (size_t)lf.nt * sizeof(double), (size_t)lf.n, hipMemcpyDeviceToHost));
    return 0;
}

int dsmgp_predict_leaves(dsmgp_ctx* c, const double* Xt, int64_t n_t, int32_t D, const int64_t* route_ptr,
                         const int64_t* route_idx, double* mu_out, double* var_out) {
    if (int rc = dsmgp_set_test(c, Xt, n_t, D, route_ptr, route_idx)) return rc;
    if (int rc = dsmgp_predict_run(c, nullptr)) return rc;
    return dsmgp_predict_fetch(c, mu_out, var_out);
}

// Sigma = K_tt - V^T V (+ noise I) of one leaf over its routed rows: the lower tiles of Vt Vt^T on the matrix cores with the
// kernel function in the epilogue (tile_predcov_kernel), mirrored by the same kernel.  Reads Vt only: after dsmgp_predict_run
// it holds K_tn L^-T for every leaf and every real column, whether the rows went through the standalone sweep or rode through
// the factorisation -- each block step of either reads all earlier block columns of Vt as its operand, and the leaves whose
// moments are finished late (pred_mu_kernel / pred_var_kernel) are finished from those stored rows.
int dsmgp_predict_cov(dsmgp_ctx* c, int32_t leaf, int32_t with_noise, double* Sigma_out, int64_t ld, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "predict_cov before predict_run on the current fit");
    if (leaf < 0 || leaf >= c->L) return fail(c, DSMGP_E_ARG, "predict_cov: leaf out of range");
    const LeafHost& lf = c->leaves[leaf];
    if (lf.nt == 0) return 0;
    if (!Sigma_out || ld < lf.nt) return fail(c, DSMGP_E_ARG, "predict_cov: Sigma_out is NULL or ld < nt");
    HIPCHK(c, hipSetDevice(c->device));
    const LeafDev& d = c->h_leaves[leaf];
    const int ntp = lf.ntpad, nbt = ntp / TB;
    if (int rc = arena_status(c, c->arenaCov.grow(arena_pool(c), (size_t)ntp * ntp))) return rc;
    std::vector<PredCovTask> tasks;
    tasks.reserve((size_t)nbt * (nbt + 1) / 2);
    // row tile by row tile, the tiles of one row next to each other: they share their A panel
    for (int i = 0; i < nbt; ++i)
        for (int j = 0; j <= i; ++j) {
            PredCovTask g{};
            g.gemm.A = d.Vt + (size_t)i * TB;
            g.gemm.B = d.Vt + (size_t)j * TB;
            g.gemm.C = c->arenaCov.p + (size_t)i * TB + (size_t)j * TB * ntp;
            g.gemm.lda = g.gemm.ldb = g.gemm.ldc = ntp;
            g.gemm.k0 = 0;
            g.gemm.k1 = lf.n - lf.n % KC2;
            g.Ct = c->arenaCov.p + (size_t)j * TB + (size_t)i * TB * ntp;
            g.xa = d.Xtg + (size_t)i * TB;
            g.xb = d.Xtg + (size_t)j * TB;
            g.ldx = ntp;
            g.na = std::min(TB, lf.nt - i * TB);
            g.nb = std::min(TB, lf.nt - j * TB);
            g.diag = (i == j);
            g.kid = lf.kid;
            g.n = lf.n;
            g.with_noise = with_noise ? 1 : 0;
            tasks.push_back(g);
        }
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    if (int rc = stage_upload_list(c, c->pcov, tasks)) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    tile_predcov_kernel<<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->pcov.p, c->d_kp.p, c->D);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(Sigma_out, (size_t)ld * sizeof(double), c->arenaCov.p, (size_t)ntp * sizeof(double),
                               (size_t)lf.nt * sizeof(double), (size_t)lf.nt, hipMemcpyDeviceToHost, c->stream));
    if (int rc = stage_done(c)) return rc;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    return 0;
}

// Joint draws of every leaf over its routed rows (kernels_sample.hpp): out = mu + chol(Sigma_l + jitter I) eps_l.
namespace {
// The blocked Cholesky of a list of symmetric matrices whose lower tiles are in place (mpad x mpad, ld = mpad, identity padding
// behind the m valid rows), one round of launches per 128-column block step for all matrices that still have that step, left
// looking: tile_gemm_kernel_v2 (block column k minus the product of the finished columns, the whole K range in one task: a fixed
// order), chol_diag_packed_kernel with nvalid (the diagonal tile, its inverse into Dinv, the first bad pivot with its absolute
// order into the matrix's flag), tile_trsm_kernel.  Shared by dsmgp_predict_sample and dsmgp_kfold.
struct CholBlock {
    double* F;          // the matrix, overwritten by its factor
    int m, mpad;
    double* Dinv;       // mpad x 128 of its own: the inverted diagonal blocks (zeroed by the caller)
    int* info;          // its flag on the device (zeroed by the caller)
};
struct CholSteps {
    std::vector<TileTask> upd, trsm, res, trsm2, add;
    std::vector<DiagTask> diag;
    std::vector<int> upd_off, trsm_off, diag_off;      // step k's tasks are [*_off[k], *_off[k + 1])
    int nsteps = 0;
};
struct CholLists {
    DevBuf<TileTask>&upd, &trsm, &res, &trsm2, &add;
    DevBuf<DiagTask>& diag;
};
// scratch tiles (128 x 128 doubles each) the panel solves of the widest step need: one per tile below the first diagonal block
size_t chol_blocks_scratch_tiles(const std::vector<CholBlock>& mats) {
    size_t n = 0;
    for (const CholBlock& b : mats) n += (size_t)(b.mpad / TB - 1);
    return n;
}
// negi: 128 x 128 doubles that chol_blocks_negi fills with -I; scratch: chol_blocks_scratch_tiles(mats) tiles
void chol_blocks_plan(const std::vector<CholBlock>& mats, double* negi, double* scratch, CholSteps& S) {
    S = CholSteps{};
    for (const CholBlock& b : mats) S.nsteps = std::max(S.nsteps, b.mpad / TB);
    S.upd_off.assign((size_t)S.nsteps + 1, 0);
    S.trsm_off.assign((size_t)S.nsteps + 1, 0);
    S.diag_off.assign((size_t)S.nsteps + 1, 0);
    for (int k = 0; k < S.nsteps; ++k) {
        for (const CholBlock& b : mats) {
            const int ntp = b.mpad, nbt = ntp / TB;
            if (k >= nbt) continue;
            double* F = b.F;
            double* Dk = b.Dinv + (size_t)k * TB * TB;
            if (k > 0)
                for (int i = k; i < nbt; ++i) {     // F[i, k] -= F[i, 0:k] F[k, 0:k]^T, the whole K range in one task
                    TileTask t{};
                    t.A = F + (size_t)i * TB;
                    t.B = F + (size_t)k * TB;
                    t.C = F + (size_t)i * TB + (size_t)k * TB * ntp;
                    t.lda = t.ldb = t.ldc = ntp;
                    t.k0 = 0;
                    t.k1 = k * TB;
                    t.update = 1;
                    t.sym = (i == k) ? 1 : 0;
                    S.upd.push_back(t);
                }
            DiagTask dt{};
            dt.T = F + (size_t)k * TB + (size_t)k * TB * ntp;
            dt.Dinv = Dk;
            dt.info = b.info;
            dt.ld = ntp;
            dt.nvalid = std::min(TB, b.m - k * TB);
            dt.row0 = k * TB;
            S.diag.push_back(dt);
            // The panel solve X = B L_kk^-T of tile B = F[i, k] multiplies with the explicit inverse, whose error grows with the
            // condition of L_kk (Sigma + 1e-8 I without noise: 4e-15 of ||A|| where a substitution leaves 3e-16), so it takes one
            // step of refinement, each a launch of the existing kernels over the step's tiles:
            //   S = B Dinv_k^T;   B <- B - S L_kk^T (the residual);   B <- B Dinv_k^T (the correction);   B <- B + S (as B - S (-I)^T)
            for (int i = k + 1; i < nbt; ++i) {
                double* tile = F + (size_t)i * TB + (size_t)k * TB * ntp;
                double* Sc = scratch + (S.trsm.size() - (size_t)S.trsm_off[(size_t)k]) * TB * TB;
                TileTask t{};
                t.A = tile;
                t.B = Dk;
                t.C = Sc;
                t.lda = ntp;
                t.ldb = t.ldc = TB;
                t.k0 = 0;
                t.k1 = TB;
                S.trsm.push_back(t);
                TileTask r{};
                r.A = Sc;
                r.B = F + (size_t)k * TB + (size_t)k * TB * ntp;
                r.C = tile;
                r.lda = TB;
                r.ldb = r.ldc = ntp;
                r.k0 = 0;
                r.k1 = TB;
                r.update = 1;
                S.res.push_back(r);
                TileTask t2 = t;
                t2.C = tile;
                t2.ldc = ntp;
                S.trsm2.push_back(t2);
                TileTask a = r;
                a.B = negi;
                a.ldb = TB;
                S.add.push_back(a);
            }
        }
        S.upd_off[(size_t)k + 1] = (int)S.upd.size();
        S.trsm_off[(size_t)k + 1] = (int)S.trsm.size();
        S.diag_off[(size_t)k + 1] = (int)S.diag.size();
    }
}
int chol_blocks_upload(dsmgp_ctx* c, const CholSteps& S, CholLists& Ls) {
    if (int rc = stage_upload_list(c, Ls.upd, S.upd)) return rc;
    if (int rc = stage_upload_list(c, Ls.trsm, S.trsm)) return rc;
    if (int rc = stage_upload_list(c, Ls.res, S.res)) return rc;
    if (int rc = stage_upload_list(c, Ls.trsm2, S.trsm2)) return rc;
    if (int rc = stage_upload_list(c, Ls.add, S.add)) return rc;
    return stage_upload_list(c, Ls.diag, S.diag);
}
int chol_blocks_negi(dsmgp_ctx* c, const CholSteps& S, double* negi) {
    if (S.trsm.empty()) return 0;
    std::vector<double> h((size_t)TB * TB, 0.0);
    for (int i = 0; i < TB; ++i) h[(size_t)i * TB + i] = -1.0;
    return stage_upload(c, negi, h.data(), h.size() * sizeof(double));
}
void chol_blocks_run(dsmgp_ctx* c, const CholSteps& S, CholLists& Ls) {
    for (int k = 0; k < S.nsteps; ++k) {
        const int nu = S.upd_off[(size_t)k + 1] - S.upd_off[(size_t)k], nd = S.diag_off[(size_t)k + 1] - S.diag_off[(size_t)k];
        const int ns = S.trsm_off[(size_t)k + 1] - S.trsm_off[(size_t)k];
        if (nu) launch_tiles(c, Ls.upd.p + S.upd_off[(size_t)k], nu);
        if (nd) chol_diag_packed_kernel<<<nd, 256, DIAGP_LDS_BYTES, c->stream>>>(Ls.diag.p + S.diag_off[(size_t)k]);
        if (ns) {
            launch_tiles(c, Ls.trsm.p + S.trsm_off[(size_t)k], ns, 1);
            launch_tiles(c, Ls.res.p + S.trsm_off[(size_t)k], ns);
            launch_tiles(c, Ls.trsm2.p + S.trsm_off[(size_t)k], ns, 1);
            launch_tiles(c, Ls.add.p + S.trsm_off[(size_t)k], ns);
        }
    }
}

// The factors of every leaf with routed rows for (with_noise, jitter): Sigma in one launch, then one round of launches per block
// step for all leaves that still have it.  Leaves whose fit failed get the flag -1 and no task.  Marks P_SAMPLE.
int sample_factorise(dsmgp_ctx* c, int with_noise, double jitter, hipEvent_t after_sigma) {
    c->invalidate(P_SAMPLE);
    const int L = c->L;
    std::vector<int32_t> finfo((size_t)L);
    if (int rc = fetch_fit_results(c, nullptr, finfo.data())) return rc;
    c->sample_off.assign((size_t)L, 0);
    std::vector<size_t> doff((size_t)L, 0);
    size_t ftot = 0, dtot = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        c->sample_off[(size_t)l] = ftot;
        doff[(size_t)l] = dtot;
        ftot += (size_t)lf.ntpad * lf.ntpad;
        dtot += (size_t)lf.ntpad * TB;
    }
    // behind the inverted diagonal blocks: -I, and one scratch tile per panel solve of the widest step (step 0)
    size_t nsolve0 = 0;
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].nt > 0) nsolve0 += (size_t)(c->leaves[l].ntpad / TB - 1);
    const size_t negi_off = dtot, scratch_off = dtot + (size_t)TB * TB;
    const size_t wtot = scratch_off + nsolve0 * TB * TB;
    if (int rc = arena_status(c, c->arenaSample.grow(arena_pool(c), ftot))) return rc;
    if (int rc = arena_status(c, c->arenaSampleDinv.grow(arena_pool(c), wtot))) return rc;
    if (int rc = c->d_sinfo.grow(c, (size_t)L)) return rc;
    std::vector<int> flags((size_t)L, 0);
    std::vector<PredCovTask> cov;
    std::vector<CholBlock> mats;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        if (finfo[(size_t)l] != 0) {
            flags[(size_t)l] = -1;
            continue;
        }
        const LeafDev& d = c->h_leaves[l];
        const int ntp = lf.ntpad, nbt = ntp / TB;
        double* F = c->arenaSample.p + c->sample_off[(size_t)l];
        for (int i = 0; i < nbt; ++i)
            for (int j = 0; j <= i; ++j) {      // dsmgp_predict_cov's tasks, into the leaf's part of the factor arena
                PredCovTask g{};
                g.gemm.A = d.Vt + (size_t)i * TB;
                g.gemm.B = d.Vt + (size_t)j * TB;
                g.gemm.C = F + (size_t)i * TB + (size_t)j * TB * ntp;
                g.gemm.lda = g.gemm.ldb = g.gemm.ldc = ntp;
                g.gemm.k0 = 0;
                g.gemm.k1 = lf.n - lf.n % KC2;
                g.Ct = g.gemm.C;
                g.xa = d.Xtg + (size_t)i * TB;
                g.xb = d.Xtg + (size_t)j * TB;
                g.ldx = ntp;
                g.na = std::min(TB, lf.nt - i * TB);
                g.nb = std::min(TB, lf.nt - j * TB);
                g.diag = (i == j);
                g.kid = lf.kid;
                g.n = lf.n;
                g.with_noise = with_noise ? 1 : 0;
                cov.push_back(g);
            }
        mats.push_back(CholBlock{F, lf.nt, ntp, c->arenaSampleDinv.p + doff[(size_t)l], c->d_sinfo.p + l});
    }
    CholSteps steps;
    chol_blocks_plan(mats, c->arenaSampleDinv.p + negi_off, c->arenaSampleDinv.p + scratch_off, steps);
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    if (int rc = stage_upload_list(c, c->scov, cov)) return rc;
    CholLists lists{c->supd, c->strsm, c->sres, c->strsm2, c->sadd, c->sdiag};
    if (int rc = chol_blocks_upload(c, steps, lists)) return rc;
    if (int rc = stage_upload(c, c->d_sinfo.p, flags.data(), (size_t)L * sizeof(int))) return rc;
    HIPCHK(c, hipMemsetAsync(c->arenaSample.p, 0, std::max<size_t>(1, ftot) * sizeof(double), c->stream));
    HIPCHK(c, hipMemsetAsync(c->arenaSampleDinv.p, 0, std::max<size_t>(1, dtot) * sizeof(double), c->stream));
    if (int rc = chol_blocks_negi(c, steps, c->arenaSampleDinv.p + negi_off)) return rc;
    if (!cov.empty()) predsample_sigma_kernel<<<(unsigned)cov.size(), 256, 0, c->stream>>>(c->scov.p, c->d_kp.p, c->D, jitter);
    HIPCHK(c, hipEventRecord(after_sigma, c->stream));
    chol_blocks_run(c, steps, lists);
    HIPCHK(c, hipGetLastError());
    c->sample_info.assign((size_t)L, 0);
    static_assert(sizeof(int) == sizeof(int32_t), "the flags are read back as int32_t");
    HIPCHK(c, hipMemcpyAsync(c->sample_info.data(), c->d_sinfo.p, (size_t)L * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (int rc = stage_done(c)) return rc;
    c->sample_noise = with_noise ? 1 : 0;
    c->sample_jitter = jitter;
    c->mark(P_SAMPLE);
    return 0;
}
}  // namespace

int dsmgp_predict_sample(dsmgp_ctx* c, int32_t with_noise, double jitter, const double* eps, int64_t ld_eps, int32_t S,
                         double* out, int64_t ld_out, int32_t* info_out, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "predict_sample before predict_run on the current fit");
    if (S < 1 || S > 65535) return fail(c, DSMGP_E_ARG, "predict_sample: S must be 1 .. 65535");
    if (!std::isfinite(jitter) || jitter < 0.0) return fail(c, DSMGP_E_ARG, "predict_sample: jitter must be finite and >= 0");
    const int L = c->L;
    const int64_t R = c->route_total;
    if (R == 0) {       // no routed rows at all: nothing to draw
        if (info_out) std::fill(info_out, info_out + L, 0);
        return 0;
    }
    if (!eps || !out) return fail(c, DSMGP_E_ARG, "predict_sample: eps or out is NULL");
    if (ld_eps < R || ld_out < R) return fail(c, DSMGP_E_ARG, "predict_sample: ld_eps or ld_out < route_total");
    for (int s = 0; s < S; ++s)
        for (int64_t e = 0; e < R; ++e)
            if (!std::isfinite(eps[e + (size_t)s * ld_eps])) return fail(c, DSMGP_E_ARG, "predict_sample: eps is not finite");
    HIPCHK(c, hipSetDevice(c->device));
    const int wn = with_noise ? 1 : 0;
    EventPair ev, evf;      // ev.a .. evf.a Sigma (after the lists' uploads), evf.a .. evf.b the block steps, evf.b .. ev.b the draws
    HIPCHK(c, ev.init());
    HIPCHK(c, evf.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    const bool factorise = !c->has(P_SAMPLE) || c->sample_noise != wn || c->sample_jitter != jitter;
    if (factorise)
        if (int rc = sample_factorise(c, wn, jitter, evf.a)) return rc;
    HIPCHK(c, hipEventRecord(evf.b, c->stream));
    const int ngrp = (S + SAMPLE_COLS - 1) / SAMPLE_COLS;
    const size_t S16 = (size_t)ngrp * SAMPLE_COLS;
    if (int rc = c->d_seps.grow(c, (size_t)R * S16)) return rc;
    if (int rc = c->d_sout.grow(c, (size_t)R * S16)) return rc;
    std::vector<SampleDrawTask> tasks;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        for (int i = lf.ntpad / TB - 1; i >= 0; --i)        // the long rows first
            for (int g = 0; g < ngrp; ++g) {
                SampleDrawTask t{};
                t.C = c->arenaSample.p + c->sample_off[(size_t)l];
                t.eps = c->d_seps.p + (size_t)lf.route_off + (size_t)g * SAMPLE_COLS * (size_t)R;
                t.out = c->d_sout.p + (size_t)lf.route_off + (size_t)g * SAMPLE_COLS * (size_t)R;
                t.mu = c->h_leaves[l].mu;
                t.info = c->d_sinfo.p + l;
                t.lde = (long long)R;
                t.ntpad = lf.ntpad;
                t.nt = lf.nt;
                t.ti = i;
                tasks.push_back(t);
            }
    }
    c->stage_top = 0;
    if (int rc = stage_upload_list(c, c->sdraw, tasks)) return rc;
    // the caller's S columns, and zeros in the columns that round S up to 16
    if (S16 > (size_t)S)
        HIPCHK(c, hipMemsetAsync(c->d_seps.p + (size_t)R * (size_t)S, 0, (size_t)R * (S16 - (size_t)S) * sizeof(double), c->stream));
    HIPCHK(c, hipMemcpy2DAsync(c->d_seps.p, (size_t)R * sizeof(double), eps, (size_t)ld_eps * sizeof(double), (size_t)R * sizeof(double),
                               (size_t)S, hipMemcpyHostToDevice, c->stream));
    predsample_draw_kernel<<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->sdraw.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipMemcpy2DAsync(out, (size_t)ld_out * sizeof(double), c->d_sout.p, (size_t)R * sizeof(double), (size_t)R * sizeof(double),
                               (size_t)S, hipMemcpyDeviceToHost, c->stream));
    if (int rc = stage_done(c)) return rc;
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    c->sample_seconds[0] = c->sample_seconds[1] = 0.0;
    if (factorise) {
        HIPCHK(c, hipEventElapsedTime(&ms, ev.a, evf.a));
        c->sample_seconds[0] = ms * 1e-3;
        HIPCHK(c, hipEventElapsedTime(&ms, evf.a, evf.b));
        c->sample_seconds[1] = ms * 1e-3;
    }
    HIPCHK(c, hipEventElapsedTime(&ms, evf.b, ev.b));
    c->sample_seconds[2] = ms * 1e-3;
    if (info_out) std::copy(c->sample_info.begin(), c->sample_info.end(), info_out);
    return 0;
}

int dsmgp_predict_sample_seconds(dsmgp_ctx* c, double* out) {
    if (!c || !out) return DSMGP_E_ARG;
    for (int i = 0; i < 3; ++i) out[i] = c->sample_seconds[i];
    return 0;
}

// Inspection: the factor of one leaf as the last dsmgp_predict_sample left it
int dsmgp_predict_cov_factor(dsmgp_ctx* c, int32_t leaf, double* Lc_out, int64_t ld) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_SAMPLE)) return fail(c, DSMGP_E_STATE, "predict_cov_factor without a current factor (dsmgp_predict_sample)");
    if (leaf < 0 || leaf >= c->L) return fail(c, DSMGP_E_ARG, "predict_cov_factor: leaf out of range");
    const LeafHost& lf = c->leaves[leaf];
    if (lf.nt == 0) return 0;
    if (!Lc_out || ld < lf.nt) return fail(c, DSMGP_E_ARG, "predict_cov_factor: Lc_out is NULL or ld < nt");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2D(Lc_out, (size_t)ld * sizeof(double), c->arenaSample.p + c->sample_off[(size_t)leaf],
                          (size_t)lf.ntpad * sizeof(double), (size_t)lf.nt * sizeof(double), (size_t)lf.nt, hipMemcpyDeviceToHost));
    return 0;
}

// -------------------------------------------------------------------------------------------------
// The score functions on the aggregated prediction (the aggregation itself: the section "predict(model, x): aggregation" below,
// after the per-entry products it reads)

int dsmgp_scores(dsmgp_ctx* c, const double* y_test, double* out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_DONE)) return fail(c, DSMGP_E_STATE, "scores before aggregate");
    if (!y_test || !out) return fail(c, DSMGP_E_ARG, "scores: NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nt = (size_t)c->n_t;
    const size_t nblk = (nt + 255) / 256;
    double* dy = c->d_agg_out.p + 2 * nt;
    double* dsum = dy + nt;
    HIPCHK(c, hipMemcpyAsync(dy, y_test, nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    std::vector<double> blk(3 * nblk);
    auto pass = [&](int which, double mse, double mae, double (&tot)[3]) -> int {
        agg_scores_kernel<<<(unsigned)nblk, 256, 0, c->stream>>>(dy, c->d_agg_out.p, c->d_agg_out.p + nt, c->n_t, which, mse, mae, dsum);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(blk.data(), dsum, blk.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        tot[0] = tot[1] = tot[2] = 0.0;
        for (size_t b = 0; b < nblk; ++b)
            for (int k = 0; k < 3; ++k) tot[k] += blk[3 * b + k];
        return 0;
    };
    double t0[3], t1[3];
    if (int rc = pass(0, 0.0, 0.0, t0)) return rc;
    const double n = (double)nt;
    const double mse = t0[0] / n, mae = t0[1] / n;
    if (int rc = pass(1, mse, mae, t1)) return rc;
    out[0] = mse;                                                        // mse  src/scorefunctions.jl:8
    out[1] = nt > 1 ? std::sqrt(t1[0] / (n - 1.0)) / std::sqrt(n) : NAN; // sse  :9  (std = unbiased)
    out[2] = mae;                                                        // mae  :13
    out[3] = nt > 1 ? std::sqrt(t1[1] / (n - 1.0)) / std::sqrt(n) : NAN; // sae  :14
    out[4] = t0[2] / n;                                                  // nlpd :16
    return 0;
}

namespace {

// ---- What the four hyper-parameter gradient passes share (dsmgp_gradients, dsmgp_loo_gradients, dsmgp_mll_columns_gradients,
// dsmgp_loo_columns_gradients): one builder of the contraction list, one launcher, one reducer of its sums.
//
// Order of a tile list.  A 128x128 tile task moves 2 x 128 x K operand doubles for 2 x 128^2 x K flops: 8 flop/B, below the
// ridge of the chip unless operands are shared through L2.  Tasks that are adjacent in the list run at the same time on one
// XCD, so the lower tiles (i, j) of a leaf are listed in super-tiles of GS x GS tiles: the GS^2 tasks of a super-tile read GS
// row panels and GS column panels between them (measured: tiles listed row by row 55 TFLOP/s; sorted by depth across leaves,
// i.e. no sharing at all, 26).  each_lower_tile lists them, marking the start of every block of GS tile rows in `gblock`
// (these tasks share their A panels); deal_tiles deals the blocks listed since `begin` to the XCDs by work = the length of a
// task's K range + `overhead` per task (neighbours in the list sit 8 apart in the launch: they run on one XCD and share its L2;
// the XCD slots get equal work).
constexpr int GS = 4;
extern "C++" {      // (templates cannot have C linkage, nor can the helpers below that return or take C++ types by value)
template <class SizeNow, class Emit>
void each_lower_tile(const LeafHost& lf, std::vector<size_t>& gblock, size_t begin, SizeNow&& size_now, Emit&& emit) {
    for (int ib = 0; ib < lf.nb; ib += GS) {
        gblock.push_back(size_now() - begin);
        for (int jb = 0; jb <= ib; jb += GS)
            for (int i = ib; i < std::min(ib + GS, lf.nb); ++i)
                for (int j = jb; j < std::min(jb + GS, i + 1); ++j)
                    emit(i, j, std::max(0, std::min(TB, lf.n - i * TB)), std::max(0, std::min(TB, lf.n - j * TB)));
    }
}
template <class Tasks>
void deal_tiles(dsmgp_ctx* c, Tasks& tasks, std::vector<int>& leaf_of, size_t begin, std::vector<size_t>& gblock, double overhead) {
    gblock.push_back(tasks.size() - begin);
    std::vector<double> work(tasks.size() - begin);
    for (size_t i = 0; i < work.size(); ++i) work[i] = (double)(tasks[begin + i].gemm.k1 - tasks[begin + i].gemm.k0) + overhead;
    xcd_deal_by_work(tasks, leaf_of, begin, tasks.size(), gblock, work, c->xcd_order);
}

// What a contraction task of one leaf reads: G = the matrix whose row tiles are multiplied (ld = ldg) -- L^-T, of which row tile
// i is zero left of column 128 i (tri: the K range starts there), or the full square H -- and the leaf's vector block.
struct DotOperand {
    const double* G;
    int ldg;
    bool tri;
    const double* vec;
};
// The contraction list of a pass: the four ranges in turn, in each the leaves of that range's kinds in leaf order, their lower
// tiles by each_lower_tile, dealt by deal_tiles.  has(l, kind): the leaf has tasks (an IsoLinear or ArdLinear leaf never has;
// whether an ArdSE leaf has is the caller's to say); operand(l): its DotOperand; fill(task, l, i, j): the mode's own fields.
template <class Task, class Has, class Operand, class Fill>
std::vector<Task> build_dot_list(dsmgp_ctx* c, DotRanges& r, double overhead, Has&& has, Operand&& operand, Fill&& fill) {
    std::vector<Task> gd;
    std::vector<size_t> gblock;
    r.leaf_of.clear();
    for (int pass = 0; pass < 4; ++pass) {
        const size_t begin = r.first[pass] = gd.size();
        gblock.clear();
        for (int l = 0; l < c->L; ++l) {
            const LeafHost& lf = c->leaves[l];
            const int kind = c->hyper[lf.kid].kind;
            if (!KINDS[kind].contraction && kind != DSMGP_KIND_ARD_SE) continue;
            if (KINDS[kind].dot_pass != pass || !has(l, kind)) continue;
            const LeafDev& d = c->h_leaves[l];
            const DotOperand o = operand(l);
            each_lower_tile(lf, gblock, begin, [&] { return gd.size(); }, [&](int i, int j, int na, int nb) {
                Task g{};
                g.gemm.A = o.G + (size_t)i * TB;
                g.gemm.B = o.G + (size_t)j * TB;
                g.gemm.C = nullptr;
                g.gemm.lda = g.gemm.ldb = o.ldg;
                g.gemm.ldc = TB;
                g.gemm.k0 = o.tri ? i * TB : 0;
                g.gemm.k1 = lf.npad;
                g.gemm.update = 0;
                g.xa = d.Xg + (size_t)i * TB;
                g.xb = d.Xg + (size_t)j * TB;
                g.alpha_a = o.vec + (size_t)i * TB;
                g.alpha_b = o.vec + (size_t)j * TB;
                g.ldx = lf.npad;
                g.na = na;
                g.nb = nb;
                g.diag = (i == j);
                g.kid = lf.kid;
                fill(g, l, i, j);
                gd.push_back(g);
                r.leaf_of.push_back(l);
            });
        }
        deal_tiles(c, gd, r.leaf_of, begin, gblock, overhead);
    }
    r.first[4] = gd.size();
    return gd;
}
// The up to four launches over a contraction list on the device: range p by the kernel of pass p, its sums at pdot + gs * first[p]
template <int MODE>
void launch_graddot(dsmgp_ctx* c, const graddot_task_t<MODE>* tasks, const DotRanges& r, double* pdot, int gs) {
    const size_t* f = r.first;
    auto grid = [&](int p) { return (unsigned)(f[p + 1] - f[p]); };
    auto out = [&](int p) { return pdot + (size_t)gs * f[p]; };
    if (grid(0)) tile_graddot_kernel<MODE><<<grid(0), 256, 0, c->stream>>>(tasks + f[0], c->d_kp.p, c->D, out(0), gs);
    if (grid(1)) tile_graddot_prod_kernel<MODE><<<grid(1), 256, 0, c->stream>>>(tasks + f[1], c->d_kp.p, c->D, out(1), gs);
    if (grid(2)) tile_graddot_matern_kernel<MODE><<<grid(2), 256, 0, c->stream>>>(tasks + f[2], c->d_kp.p, c->D, out(2), gs);
    if (grid(3)) tile_graddot_rq_kernel<MODE><<<grid(3), 256, 0, c->stream>>>(tasks + f[3], c->d_kp.p, c->D, out(3), gs);
}
// The tiles of H = K_y^-1 diag(sqrt w) of the LOO passes (tile_ginv_kernel): the leaves with has(l) in leaf order, one deal.
// place(l): what a leaf's tasks read and write.
struct GinvPlace {
    const double* Xt;       // L^-T of the leaf's factor owner (ld = ldt)
    int ldt;
    double* H;              // npad x npad
    const double* sw;       // sqrt w of the leaf's rows
};
template <class Has, class Place>
std::vector<GinvTask> build_ginv_list(dsmgp_ctx* c, Has&& has, Place&& place) {
    std::vector<GinvTask> gi;
    std::vector<int> gi_leaf;
    std::vector<size_t> gblock;
    for (int l = 0; l < c->L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (!has(l)) continue;
        const GinvPlace o = place(l);
        each_lower_tile(lf, gblock, 0, [&] { return gi.size(); }, [&](int i, int j, int na, int nb) {
            GinvTask g{};
            g.gemm.A = o.Xt + (size_t)i * TB;
            g.gemm.B = o.Xt + (size_t)j * TB;
            g.gemm.C = o.H + (size_t)i * TB + (size_t)j * TB * lf.npad;
            g.Ct = o.H + (size_t)j * TB + (size_t)i * TB * lf.npad;
            g.gemm.lda = g.gemm.ldb = o.ldt;
            g.gemm.ldc = lf.npad;
            g.gemm.k0 = i * TB;
            g.gemm.k1 = lf.npad;
            g.sw_a = o.sw + (size_t)i * TB;
            g.sw_b = o.sw + (size_t)j * TB;
            g.na = na;
            g.nb = nb;
            g.diag = (i == j);
            gi.push_back(g);
            gi_leaf.push_back(l);
        });
    }
    deal_tiles(c, gi, gi_leaf, 0, gblock, 64.0);
    return gi;
}

// The sums of a contraction list per leaf, the tasks of a leaf added in list order (fixed: bit-reproducible).  A task's slots:
// [0] weight . K r^2, [1] weight . K (LOO modes), [2 .. 2 + D) weight . dK / dlog l_d, [2 + D] weight . dK / dlog alpha (rational
// quadratic).  The LOO modes read slots 0 and 1 of every task; the marginal-likelihood modes read slot 0 of the kinds without
// per-dimension sums only.  Sd is empty when the tasks have no per-dimension slots (gs == 2).
struct DotSums {
    std::vector<double> S1, SK, Sd, Sa;
};
DotSums reduce_dot_sums(const dsmgp_ctx* c, const DotRanges& r, const double* pd, size_t gs, bool loo) {
    const size_t L = (size_t)c->L, D = (size_t)c->D;
    DotSums s;
    s.S1.assign(L, 0.0);
    s.Sa.assign(L, 0.0);
    if (loo) s.SK.assign(L, 0.0);
    if (gs > 2) s.Sd.assign(L * D, 0.0);
    for (size_t i = 0; i < r.count(); ++i) {
        const size_t l = (size_t)r.leaf_of[i];
        const KindInfo& ki = KINDS[c->hyper[c->leaves[l].kid].kind];
        const double* t = pd + gs * i;
        if (loo) {
            s.S1[l] += t[0];
            s.SK[l] += t[1];
        } else if (!ki.per_dim_grad) {
            s.S1[l] += t[0];
        }
        if (ki.per_dim_grad) {
            for (size_t d = 0; d < D; ++d) s.Sd[l * D + d] += t[2 + d];
            if (ki.rq) s.Sa[l] += t[2 + D];
        }
    }
    return s;
}
// The ardlin_quad_kernel tasks of an ArdLinear leaf, ARDLIN_COLS columns of M (ld = ldm: L^-T of the factor owner, or the leaf's H)
// each, with the leaf's inputs x and its vector block
void ardlin_tasks(std::vector<ArdLinTask>& tasks, std::vector<int>& leaf_of, int l, const LeafHost& lf, const double* M, int ldm,
                  const double* x, const double* vec) {
    for (int c0 = 0; c0 < lf.n; c0 += ARDLIN_COLS) {
        ArdLinTask a{};
        a.Xt = M;
        a.x = x;
        a.alpha = vec;
        a.ldt = ldm;
        a.ldx = lf.npad;      // FULL (the LOO passes): also the distance from alpha to u in the vector block
        a.c0 = c0;
        a.n = lf.n;
        tasks.push_back(a);
        leaf_of.push_back(l);
    }
}
// What the entry points check of their arguments alike
int check_stride(dsmgp_ctx* c, const char* who, int stride) {
    for (int l = 0; l < c->L; ++l)
        if ((int)c->hyper[c->leaves[l].kid].loghyp.size() > stride)
            return fail(c, DSMGP_E_ARG, std::string(who) + ": stride smaller than the hyper-vector");
    return 0;
}
// W[L x Q] = the caller's column weights (NULL: ones), sw[l] = their sum over the columns in ascending q
int column_weights(dsmgp_ctx* c, const char* who, const double* col_weight, bool refuse_negative, std::vector<double>& W,
                   std::vector<double>& sw) {
    const size_t L = (size_t)c->L, Q = (size_t)c->tg_Q;
    W.assign(L * Q, 1.0);
    sw.assign(L, 0.0);
    if (col_weight)
        for (size_t i = 0; i < W.size(); ++i) {
            if (!std::isfinite(col_weight[i]) || (refuse_negative && col_weight[i] < 0.0))
                return fail(c, DSMGP_E_ARG, std::string(who) + (refuse_negative ? ": non-finite or negative value in col_weight"
                                                                               : ": non-finite value in col_weight"));
            W[i] = col_weight[i];
        }
    for (size_t l = 0; l < L; ++l)
        for (size_t q = 0; q < Q; ++q) sw[l] += W[l + q * L];
    return 0;
}
}  // extern "C++"

// Task lists of the gradient pass: Xt = L^-T by a blocked triangular inversion on the same tile kernels
// (row tile t of Xt is e_t^T L^-T: zero left of block t, Dinv_t^T on the diagonal, then a left-looking sweep
// whose K range starts at column 128 t), then the contraction tiles of tile_graddot_kernel.
int build_grad_plan(dsmgp_ctx* c) {
    const int L = c->L;
    size_t xTot = 0;
    std::vector<size_t> xoff(L, 0);
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].owner == l) {
            xoff[l] = xTot;
            xTot += (size_t)c->leaves[l].npad * c->leaves[l].npad;
        }
    size_t freeB = 0, totalB = 0;
    HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
    if (!c->pool.active() && xTot * sizeof(double) + (size_t(2) << 30) > freeB)
        return fail(c, DSMGP_E_NOMEM, "gradients need " + std::to_string((xTot * 8) >> 20) + " MiB for L^-1, device has " +
                                          std::to_string(freeB >> 20) + " MiB free");
    // kept across changes of the active set (dsmgp_set_gradient_leaves)
    if (int rc = arena_status(c, c->arenaX.exact(arena_pool(c), xTot))) return rc;
    c->gxoff = xoff;
    auto Xt = [&](int l) { return c->arenaX.p + xoff[c->leaves[l].owner]; };
    // Active leaves (dsmgp_set_gradient_leaves; default all).  A leaf's gradient needs tr K_y^-1 = |L^-1|_F^2 of its factor
    // owner and, for the kernels with a length-scale term, the contraction tiles -- its own, or its source's where a COPY leaf
    // shares them (grad_src): needC = leaves whose contraction is computed, needX = owners whose L^-T is built.
    auto active = [&](int l) { return c->grad_active.empty() || c->grad_active[l] != 0; };
    c->grad_src.assign(L, -1);
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.op == DSMGP_SHARE_COPY && lf.mean == c->leaves[lf.src].mean) c->grad_src[l] = lf.src;
    }
    std::vector<char> needC(L, 0), needX(L, 0);
    for (int l = 0; l < L; ++l)
        if (active(l)) {
            needC[c->grad_src[l] >= 0 ? c->grad_src[l] : l] = 1;
            needX[c->leaves[l].owner] = 1;
        }
    for (int l = 0; l < L; ++l)
        if (needC[l] || c->grad_all_owners) needX[c->leaves[l].owner] = 1;     // (dsmgp_loo reads L^-T of every owner)

    c->grad_lists_all = true;
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].owner == l && !needX[l]) c->grad_lists_all = false;

    std::vector<TransTask> trans;
    std::vector<FrobTask> frob;
    c->gfrob_leaf.clear();
    int nsteps = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.owner != l || !needX[l]) continue;
        nsteps = std::max(nsteps, lf.nb);
        const LeafDev& d = c->h_leaves[l];
        for (int t = 0; t < lf.nb; ++t) {
            TransTask tt{};
            tt.src = d.Dinv + (size_t)t * TB * TB;
            tt.dst = Xt(l) + (size_t)t * TB + (size_t)t * TB * lf.npad;
            tt.ldd = lf.npad;
            trans.push_back(tt);
            FrobTask f{};
            f.X = Xt(l) + (size_t)t * TB;
            f.ld = lf.npad;
            f.col0 = t * TB;
            f.col1 = lf.npad;
            f.nrows = std::max(0, std::min(TB, lf.n - t * TB));
            f.n = lf.n;
            frob.push_back(f);
            c->gfrob_leaf.push_back(l);
        }
    }
    // the inversion runs lane by lane like the factorisation (SweepLists; a leaf inverts in the lane that factorised it)
    const int nl = c->nlanes;
    std::vector<SweepLane> lanes = sweep_lanes(c, nl, nsteps);
    for (int q = 0; q < nl; ++q) {
        SweepLane& ln = lanes[(size_t)q];
        for (int k = 1; k < nsteps; ++k) {
            ln.mark(k);
            std::vector<TileTask> tiles;
            double depth = 0.0;
            for (int l = 0; l < L; ++l) {
                const LeafHost& lf = c->leaves[l];
                if (lf.owner != l || lf.nb <= k || !needX[l] || (nl > 1 && c->leaf_lane[l] != q)) continue;
                const LeafDev& d = c->h_leaves[l];
                for (int t = 0; t < k; ++t) {
                    double* tile = Xt(l) + (size_t)t * TB + (size_t)k * TB * lf.npad;
                    TileTask u{};
                    u.A = Xt(l) + (size_t)t * TB;
                    u.B = d.F + (size_t)k * TB;
                    u.C = tile;
                    u.lda = u.ldb = u.ldc = lf.npad;
                    u.k0 = t * TB;
                    u.k1 = k * TB;
                    u.update = 2;            // the block is defined here: -product, nothing to read (Xt needs no zero fill:
                    u.rev = 1;               //   every later task reads row tile t from column 128 t on only)
                    tiles.push_back(u);
                    depth += u.k1 - u.k0;
                    TileTask s{};
                    s.A = tile;
                    s.B = d.Dinv + (size_t)k * TB * TB;
                    s.C = tile;
                    s.lda = lf.npad;
                    s.ldb = TB;
                    s.ldc = lf.npad;
                    s.k0 = 0;
                    s.k1 = TB;
                    s.update = 0;
                    ln.trsm.push_back(s);
                }
            }
            const int Kavg = tiles.empty() ? 0 : (int)(depth / tiles.size()) / TB * TB;
            ln.U.add_step_ragged(tiles, std::max(TB, Kavg), k);
        }
    }

    // contraction tiles (build_dot_list): every IsoSE, ArdSEProduct, Matern and rational quadratic leaf, and the ArdSE leaves when
    // the true length-scale gradient is asked for (COPY leaves too: their alpha is their own).
    // Shared gradients (the idea of src/fit.jl:313-395: a leaf whose observation set equals its main leaf's takes that leaf's
    // gradients, `copygradients`): a COPY leaf has its source's factor and kernel id; with the same ConstMean its alpha is the
    // source's too, so its contraction is the source's and is not computed again.
    bool any_ard = false, any_prod = false;
    for (int l = 0; l < L; ++l) {
        const int kind_l = c->hyper[c->leaves[l].kid].kind;
        any_ard = any_ard || (kind_l == DSMGP_KIND_ARD_SE && c->ard_true_gradient);
        any_prod = any_prod || KINDS[kind_l].dot_pass != 0;
    }
    const std::vector<GradTask> gd = build_dot_list<GradTask>(
        c, c->gdot_ranges, 64.0,
        [&](int l, int kind) { return (kind != DSMGP_KIND_ARD_SE || c->ard_true_gradient) && c->grad_src[l] < 0 && needC[l]; },
        [&](int l) { return DotOperand{Xt(l), c->leaves[l].npad, true, c->h_leaves[l].alpha}; }, [](GradTask&, int, int, int) {});
    if (int rc = dev_upload(c, c->gtrans, trans)) return rc;
    if (int rc = dev_upload(c, c->gfrob, frob)) return rc;
    if (int rc = pack_sweep(c, c->ginv, lanes, copy_upload)) return rc;
    if (int rc = dev_upload(c, c->gdot, gd)) return rc;
    if (any_ard && c->D > GRADDOT_STAGE_D)
        return fail(c, DSMGP_E_ARG, "ArdSE length-scale gradients need D <= " + std::to_string(GRADDOT_STAGE_D));
    c->gstride = (any_ard || any_prod) ? 2 + c->D : 2;     // ArdSEProduct, Matern, rational quadratic: any D (staged in chunks)
    if (any_rq(c)) c->gstride = 3 + c->D;                  // one more slot behind the dimensions: the sum for dK / dlog alpha

    // ArdLinear leaves: ARDLIN_COLS columns of L^-T per task (a COPY leaf with its source's mean takes the source's sums,
    // as for the contraction), the tasks of the longest columns first
    std::vector<ArdLinTask> al;
    c->gardlin_leaf.clear();
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (c->hyper[lf.kid].kind != DSMGP_KIND_ARD_LINEAR) continue;
        if (c->grad_src[l] >= 0 || !needC[l]) continue;
        ardlin_tasks(al, c->gardlin_leaf, l, lf, Xt(l), c->leaves[lf.owner].npad, c->h_leaves[l].Xg, c->h_leaves[l].alpha);
    }
    {
        std::vector<size_t> ord(al.size());
        for (size_t i = 0; i < ord.size(); ++i) ord[i] = i;
        std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return al[a].c0 > al[b].c0; });
        std::vector<ArdLinTask> al2(al.size());
        std::vector<int> leaf2(al.size());
        for (size_t i = 0; i < ord.size(); ++i) {
            al2[i] = al[ord[i]];
            leaf2[i] = c->gardlin_leaf[ord[i]];
        }
        al.swap(al2);
        c->gardlin_leaf.swap(leaf2);
    }
    if (int rc = dev_upload(c, c->gardlin, al)) return rc;
    c->gpart_count = frob.size() + (size_t)c->gstride * gd.size() + 2 * (size_t)L + 2 * (size_t)c->D * al.size();
    if (int rc = c->d_gpart.grow(c, c->gpart_count)) return rc;
    c->mark(P_GRAD_LISTS);
    return 0;
}

}  // namespace

namespace {
// The per-kind assembly of one leaf's gradient row from the sums of the device passes: S1 / Sd / Sa the contractions of the
// weight matrix with K P, dK / dlog l_d and dK / dlog alpha, Sl the ArdLinear forms, trK = s tr K_y^-1, ya = sum w (y - m) . alpha,
// aa = sum w alpha . alpha, ns = n s -- s = 1 and one column for dsmgp_gradients, s = sum_q w_q for dsmgp_mll_columns_gradients.
struct GradSums {
    double S1;
    const double* Sd;       // D sums, or null when no per-dimension sums were taken
    double Sa;
    const double* Sl;       // D sums
    double trK, ya, aa, ns;
};
void assemble_gradient(const dsmgp_ctx* c, const HyperHost& h, const GradSums& q, double* g) {
    const int nl = n_lengthscales(h.kind, h.loghyp.size());
    const int ns = nl + KINDS[h.kind].n_shape;               // the slot of logs; logNoise behind it
    const double noise = std::exp(2.0 * h.loghyp[ns + 1]);
    const double cc = noise + 1e-8;
    const double ya = q.ya, aa = q.aa;
    const double n = q.ns;
    // tr(precomp K) with K = K_y - c I:  (y.alpha - c alpha.alpha) - (n - c tr K_y^-1)
    const double trPK = (ya - cc * aa) - (n - cc * q.trK);
    if (h.kind == DSMGP_KIND_ISO_SE) {
        const double sigma = std::exp(h.loghyp[1]);
        const double ell2 = std::exp(2.0 * h.loghyp[0]);
        g[0] = 0.5 * sigma * q.S1 / ell2;                 // src/kernels.jl:95-97
        g[1] = sigma * trPK;                              // src/kernels.jl:90-93
    } else if (h.kind == DSMGP_KIND_ARD_SE) {
        const double sigma = std::exp(h.loghyp[nl]);
        for (int d = 0; d < nl; ++d)                      // src/kernels.jl:161: identically zero unless the
            g[d] = (c->ard_true_gradient && q.Sd) ? 0.5 * q.Sd[d] : 0.0;   // true gradient is asked for
        g[nl] = sigma * trPK;                             // src/kernels.jl:157
    } else if (h.kind == DSMGP_KIND_ISO_LINEAR) {
        g[0] = -trPK;                                     // src/kernels.jl:198
        g[1] = 0.0;                                       // src/kernels.jl:201
    } else if (h.kind == DSMGP_KIND_ARD_LINEAR) {
        // the true derivative -S_d / l_d^2 (src/kernels.jl:234-246 is the same trace with kappa = z / l_d and does not run;
        // DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT is about ArdSE only); no variance gradient (the slot is a dummy, :216-218)
        for (int d = 0; d < nl; ++d) g[d] = -q.Sl[d] / std::exp(2.0 * h.loghyp[d]);
        g[nl] = 0.0;
    } else if (h.kind == DSMGP_KIND_ARD_SE_PRODUCT) {
        // the true derivatives: 0.5 tr(W dK / dlog l_d) from the per-dimension sums, 0.5 tr(W 2K) = tr(W K) (no SURVEY F7 factor)
        for (int d = 0; d < nl; ++d) g[d] = 0.5 * q.Sd[d];
        g[nl] = trPK;
    } else if (KINDS[h.kind].matern || KINDS[h.kind].rq) {
        // the true derivatives as for ArdSEProduct; an iso kind's dl is the sum over the dimensions, added in ascending d
        if (KINDS[h.kind].iso_matern) {
            double sl = 0.0;
            for (int d = 0; d < c->D; ++d) sl += q.Sd[d];
            g[0] = 0.5 * sl;
        } else {
            for (int d = 0; d < nl; ++d) g[d] = 0.5 * q.Sd[d];
        }
        if (KINDS[h.kind].rq) g[nl] = 0.5 * q.Sa;         // da = 0.5 tr(W dK / dlog alpha)
        g[ns] = trPK;
    }
    g[ns + 1] = noise * (aa - q.trK);                     // src/gaussianprocess.jl:176
}
}  // namespace

int dsmgp_set_gradient_leaves(dsmgp_ctx* c, const int32_t* active) {
    if (!c) return DSMGP_E_ARG;
    if (c->L == 0) return fail(c, DSMGP_E_STATE, "set_gradient_leaves before set_leaves");
    std::vector<char> m;
    if (active) {
        m.resize(c->L);
        bool all = true;
        for (int l = 0; l < c->L; ++l) {
            m[l] = active[l] != 0;
            all = all && m[l];
        }
        if (all) m.clear();
    }
    if (m != c->grad_active) {
        HIPCHK(c, hipSetDevice(c->device));
        free_grad_lists(c);
        c->grad_active = std::move(m);
    }
    return 0;
}

int dsmgp_gradients(dsmgp_ctx* c, double* grad_out, int32_t stride) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "gradients before fit");
    if (!grad_out) return fail(c, DSMGP_E_ARG, "grad_out is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const int L = c->L;
    if (int rc = check_stride(c, "gradients", stride)) return rc;
    if (!c->has(P_GRAD_LISTS))
        if (int rc = build_grad_plan(c)) return rc;
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = ensure_alpha(c)) return rc;
    c->timings[10] = 0.0;
    EventPair ev;
    HIPCHK(c, ev.init());
    const hipEvent_t t0 = ev.a, t1 = ev.b;
    HIPCHK(c, hipEventRecord(t0, c->stream));
    for (int i = 15; i < 18; ++i) c->timings[i] = 0.0;
    EventPair e_inv, e_dot;     // three spans: L^-T | contraction | traces and dots
    HIPCHK(c, e_inv.init());
    HIPCHK(c, e_dot.init());
    // Xt = L^-T (blocks left of the diagonal are never written and never read)
    c->invalidate(P_XINV);
    if (c->gtrans.count) transpose_tile_kernel<<<(int)c->gtrans.count * 16, 256, 0, c->stream>>>(c->gtrans.p);
    if (int rc = run_sweep(c, c->ginv, nullptr)) return rc;     // the lanes' streams wait for the transposes
    HIPCHK(c, hipEventRecord(e_inv.a, c->stream));
    double* pfrob = c->d_gpart.p;
    double* pdot = pfrob + c->gfrob.count;
    double* pleaf = pdot + (size_t)c->gstride * c->gdot.count;
    launch_graddot<GD_MLL>(c, c->gdot.p, c->gdot_ranges, pdot, c->gstride);
    HIPCHK(c, hipEventRecord(e_dot.a, c->stream));
    if (c->gfrob.count) frob_kernel<<<(int)c->gfrob.count, 256, 0, c->stream>>>(c->gfrob.p, pfrob);
    dots_kernel<<<L, 256, 0, c->stream>>>(c->d_leaves.p, pleaf);
    double* pardlin = pleaf + 2 * (size_t)L;
    if (c->gardlin.count)
        ardlin_quad_kernel<false><<<dim3((unsigned)c->gardlin.count, (unsigned)((c->D + ARDLIN_DC - 1) / ARDLIN_DC)), 256, 0, c->stream>>>(
            c->gardlin.p, c->D, pardlin);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(t1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->grad_lists_all) c->mark(P_XINV);     // dsmgp_loo on this fit reads the arena as it is (this pass itself inverts on every call, as
                                                // it always did); under a mask that leaves owners out, theirs is stale or rewritten by other lists
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
    c->timings[10] = ms * 1e-3;
    HIPCHK(c, hipEventElapsedTime(&ms, t0, e_inv.a));
    c->timings[15] = ms * 1e-3;
    HIPCHK(c, hipEventElapsedTime(&ms, e_inv.a, e_dot.a));
    c->timings[16] = ms * 1e-3;
    HIPCHK(c, hipEventElapsedTime(&ms, e_dot.a, t1));
    c->timings[17] = ms * 1e-3;
    std::vector<double> part(c->gpart_count);
    HIPCHK(c, hipMemcpy(part.data(), c->d_gpart.p, c->gpart_count * sizeof(double), hipMemcpyDeviceToHost));
    // host assembly (fixed summation order -> reproducible)
    std::vector<double> trK(L, 0.0);
    for (size_t i = 0; i < c->gfrob.count; ++i) trK[c->gfrob_leaf[i]] += part[i];
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].owner != l) trK[l] = trK[c->leaves[l].owner];
    const double* pd = part.data() + c->gfrob.count;
    const size_t gs = (size_t)c->gstride;
    DotSums sums = reduce_dot_sums(c, c->gdot_ranges, pd, gs, false);
    for (int l = 0; l < L; ++l)
        if (c->grad_src[l] >= 0) {   // copygradients (src/fit.jl:352-356)
            sums.S1[l] = sums.S1[c->grad_src[l]];
            sums.Sa[l] = sums.Sa[c->grad_src[l]];
            if (gs > 2)
                for (int d = 0; d < c->D; ++d) sums.Sd[(size_t)l * c->D + d] = sums.Sd[(size_t)c->grad_src[l] * c->D + d];
        }
    const double* pl = pd + gs * c->gdot.count;
    // ArdLinear: S_d = (alpha . x_d)^2 - |L^-1 x_d|^2 per leaf, the task sums added in list order
    std::vector<double> Sl((size_t)L * c->D, 0.0);
    if (c->gardlin.count) {
        const size_t D = (size_t)c->D;
        std::vector<double> A((size_t)L * D, 0.0), Q((size_t)L * D, 0.0);
        const double* pq = pl + 2 * (size_t)L;
        for (size_t i = 0; i < c->gardlin.count; ++i) {
            const size_t l = (size_t)c->gardlin_leaf[i];
            for (size_t d = 0; d < D; ++d) {
                A[l * D + d] += pq[2 * D * i + d];
                Q[l * D + d] += pq[2 * D * i + D + d];
            }
        }
        for (int l = 0; l < L; ++l) {
            const int s = c->grad_src[l] >= 0 ? c->grad_src[l] : l;      // copygradients (src/fit.jl:352-356)
            for (size_t d = 0; d < D; ++d) Sl[l * D + d] = A[s * D + d] * A[s * D + d] - Q[s * D + d];
        }
    }
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        double* g = grad_out + (size_t)l * stride;
        for (int j = 0; j < stride; ++j) g[j] = 0.0;
        if (!c->grad_active.empty() && !c->grad_active[l]) continue;      // not asked for (dsmgp_set_gradient_leaves): zeros
        GradSums q{};
        q.S1 = sums.S1[l];
        q.Sd = gs > 2 ? sums.Sd.data() + (size_t)l * c->D : nullptr;
        q.Sa = sums.Sa[l];
        q.Sl = Sl.data() + (size_t)l * c->D;
        q.trK = trK[l];
        q.ya = pl[2 * l];
        q.aa = pl[2 * l + 1];
        q.ns = (double)lf.n;
        assemble_gradient(c, c->hyper[lf.kid], q, g);
    }
    return 0;
}

// Leave-one-out moments of every leaf from the diagonal of K_y^-1 and alpha (GPML 5.4.2): d = rowsumsq of L^-T per factor
// owner (rownorm_kernel: one task per 128-row tile and ROWNORM_COLS columns), then loo_moments_kernel per leaf.  L^-T comes from
// the gradient pass's lists; it is built here unless the arena holds it for the current fit and for every owner.
namespace {
// L^-T of every factor owner in arenaX for whoever reads it after a fit (dsmgp_loo, dsmgp_predict_gradients), in two halves.
// xinv_lists: the task lists of the inversion, unless the arena already holds the current fit's L^-T.  Lists made under a mask
// (dsmgp_set_gradient_leaves) leave out the owners no active leaf needs: then the sweep runs over lists of the call's own, built
// for every owner and dropped again when `own` goes out of scope (on every way out, the failing ones too), so that the next
// dsmgp_gradients builds the mask's lists as it would have without the call -- same launches, same bits.
// xinv_fill: queues the transposes and the sweep when they are needed; the caller marks P_XINV once the stream is through.
struct OwnGradLists {
    dsmgp_ctx* c;
    bool on = false;
    ~OwnGradLists() {
        if (on) free_grad_lists(c);
    }
};
int xinv_lists(dsmgp_ctx* c, OwnGradLists& own) {
    if (c->has(P_XINV)) return 0;
    if (c->has(P_GRAD_LISTS) && !c->grad_lists_all) free_grad_lists(c);
    if (!c->has(P_GRAD_LISTS)) {
        own.on = !c->grad_active.empty();
        c->grad_all_owners = true;
        const int rc = build_grad_plan(c);
        c->grad_all_owners = false;
        if (rc) return rc;
    }
    return 0;
}
int xinv_fill(dsmgp_ctx* c) {
    if (c->has(P_XINV)) return 0;
    if (c->gtrans.count) transpose_tile_kernel<<<(int)c->gtrans.count * 16, 256, 0, c->stream>>>(c->gtrans.p);
    return run_sweep(c, c->ginv, nullptr);
}

int build_loo_plan(dsmgp_ctx* c) {
    const int L = c->L;
    std::vector<size_t> poff(L, 0);
    size_t pTot = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.owner != l) continue;
        poff[l] = pTot;
        pTot += (size_t)lf.npad * ((lf.n + ROWNORM_COLS - 1) / ROWNORM_COLS);
    }
    const size_t nobs = (size_t)c->obs_ptr[L];
    if (int rc = c->d_loo.alloc(c, pTot + 2 * nobs + (size_t)L)) return rc;
    std::vector<RowNormTask> rows;
    std::vector<LooTask> lt((size_t)L);
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const LeafHost& ow = c->leaves[lf.owner];
        lt[l].P = c->d_loo.p + poff[lf.owner];
        lt[l].alpha = c->h_leaves[c->grad_src[l] >= 0 ? c->grad_src[l] : l].alpha;
        lt[l].off = (long long)c->obs_ptr[l];
        lt[l].ldp = ow.npad;
        if (lf.owner != l) continue;
        for (int t = 0; t * TB < lf.n; ++t)
            for (int c0 = t * TB, k = 0; c0 < lf.n; c0 += ROWNORM_COLS, ++k) {
                RowNormTask r{};
                r.X = c->arenaX.p + c->gxoff[l] + (size_t)t * TB;
                r.out = c->d_loo.p + poff[l] + (size_t)k * lf.npad + (size_t)t * TB;
                r.ld = lf.npad;
                r.col0 = c0;
                r.col1 = std::min(c0 + ROWNORM_COLS, lf.n);
                r.nrows = std::min(TB, lf.n - t * TB);
                rows.push_back(r);
            }
    }
    if (int rc = dev_upload(c, c->lrow, rows)) return rc;
    if (int rc = dev_upload(c, c->lleaf, lt)) return rc;
    c->mark(P_LOO_LISTS);
    return 0;
}
}  // namespace

int dsmgp_loo(dsmgp_ctx* c, double* mu_out, double* var_out, double* lpd_out, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "loo before fit");
    HIPCHK(c, hipSetDevice(c->device));
    const int L = c->L;
    // L^-T of every factor owner (xinv_lists / xinv_fill)
    OwnGradLists own_lists{c};
    if (int rc = xinv_lists(c, own_lists)) return rc;
    if (!c->has(P_LOO_LISTS))
        if (int rc = build_loo_plan(c)) return rc;
    EventPair ev;           // the device work of the call: what is left to complete of Dinv and alpha after this fit, the sweep, the two kernels
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = ensure_alpha(c)) return rc;
    if (int rc = xinv_fill(c)) return rc;
    const size_t nobs = (size_t)c->obs_ptr[L];
    double* dmu = c->d_loo.p + (c->d_loo.count - 2 * nobs - (size_t)L);
    double* dvar = dmu + nobs;
    double* dlpd = dvar + nobs;
    if (c->lrow.count) rownorm_kernel<<<(unsigned)c->lrow.count, 256, 0, c->stream>>>(c->lrow.p);
    loo_moments_kernel<<<L, 256, 0, c->stream>>>(c->d_leaves.p, c->lleaf.p, c->d_obs_idx.p, c->dy.p, dmu, dvar, dlpd);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_XINV);
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    if (mu_out) HIPCHK(c, hipMemcpy(mu_out, dmu, nobs * sizeof(double), hipMemcpyDeviceToHost));
    if (var_out) HIPCHK(c, hipMemcpy(var_out, dvar, nobs * sizeof(double), hipMemcpyDeviceToHost));
    if (lpd_out) HIPCHK(c, hipMemcpy(lpd_out, dlpd, (size_t)L * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

namespace {
// C^-T of every factorised block of dsmgp_kfold into `X` (block b at xoff[b], ld = mpad): the recipe of build_grad_plan's
// inversion -- the diagonal tiles are the transposed inverted diagonal blocks, then per block step k one update launch
// (tile (t, k) = -X[t, 128 t : 128 k] C[k, 128 t : 128 k]^T, nothing read: update = 2) and one panel solve against Dinv_k.
struct KfoldInverseTasks {
    std::vector<TransTask> trans;
    std::vector<TileTask> upd, trsm;        // task for task beside each other
    std::vector<size_t> step_off{0};        // step k's tasks are [step_off[k - 1], step_off[k])
};
static void kfold_inverse_tasks(const std::vector<CholBlock>& mats, double* X, const std::vector<size_t>& xoff, int nsteps,
                         KfoldInverseTasks& out) {
    for (size_t b = 0; b < mats.size(); ++b)
        for (int t = 0; t < mats[b].mpad / TB; ++t) {
            TransTask tt{};
            tt.src = mats[b].Dinv + (size_t)t * TB * TB;
            tt.dst = X + xoff[b] + (size_t)t * TB + (size_t)t * TB * mats[b].mpad;
            tt.ldd = mats[b].mpad;
            out.trans.push_back(tt);
        }
    for (int k = 1; k < nsteps; ++k) {
        for (size_t b = 0; b < mats.size(); ++b) {
            const int mp = mats[b].mpad;
            if (mp / TB <= k) continue;
            double* Xc = X + xoff[b];
            for (int t = 0; t < k; ++t) {
                double* tile = Xc + (size_t)t * TB + (size_t)k * TB * mp;
                TileTask u{};
                u.A = Xc + (size_t)t * TB;
                u.B = mats[b].F + (size_t)k * TB;
                u.C = tile;
                u.lda = u.ldb = u.ldc = mp;
                u.k0 = t * TB;
                u.k1 = k * TB;
                u.update = 2;
                u.rev = 1;
                out.upd.push_back(u);
                TileTask sv{};
                sv.A = tile;
                sv.B = mats[b].Dinv + (size_t)k * TB * TB;
                sv.C = tile;
                sv.lda = mp;
                sv.ldb = TB;
                sv.ldc = mp;
                sv.k0 = 0;
                sv.k1 = TB;
                out.trsm.push_back(sv);
            }
        }
        out.step_off.push_back(out.upd.size());
    }
}
}  // namespace

// k-fold cross-validation of every leaf GP from the current fit (the kernels and the formulas: kernels_kfold.hpp).  The blocks come
// from kfold_plan.hpp, once per factor owner -- a COPY leaf applies its source's factors to its own alpha, y and mean.  L^-T comes
// by dsmgp_loo's rule (xinv_lists / xinv_fill).  The labels are packed round by round (label k of every owner, then that round's
// G_FF tiles), so the panel arena has the largest round's size; the factorisation, the inversion and the moments run over all
// blocks together.  Nothing another entry point reads is written, and nothing is kept but the allocations.
int dsmgp_kfold(dsmgp_ctx* c, const int32_t* fold, int32_t K, double* mu_out, double* var_out, double* lpd_out, int32_t* info_out,
                double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "kfold before fit");
    if (!fold) return fail(c, DSMGP_E_ARG, "kfold: fold is NULL");
    if (K < 1 || K > 65535) return fail(c, DSMGP_E_ARG, "kfold: K must be 1 .. 65535");
    // every one of the N labels is checked, held by a leaf or not: what the call accepts does not depend on the leaf table or on
    // which fits succeeded (kfold_plan::build guards itself once more; after this loop it cannot refuse)
    for (int64_t i = 0; i < c->N; ++i)
        if (fold[i] < -1 || fold[i] >= K) return fail(c, DSMGP_E_ARG, "kfold: a label outside -1 .. K - 1");
    HIPCHK(c, hipSetDevice(c->device));
    const int L = c->L;
    const size_t nobs = (size_t)c->obs_ptr[L];
    const bool want_var = var_out != nullptr;
    std::vector<int32_t> finfo((size_t)L);
    if (int rc = fetch_fit_results(c, nullptr, finfo.data())) return rc;
    // L^-T of every factor owner (xinv_lists / xinv_fill); lists of the call's own are dropped again on every way out
    const bool had_xinv = c->has(P_XINV);
    OwnGradLists own_lists{c};
    if (int rc = xinv_lists(c, own_lists)) return rc;

    // the blocks, once per factor owner whose fit succeeded
    std::vector<kfold_plan::Owner> owners;
    std::vector<int> owner_at((size_t)L, -1);
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].owner == l && finfo[(size_t)l] == 0) {
            owner_at[(size_t)l] = (int)owners.size();
            owners.push_back(kfold_plan::Owner{l, c->leaves[l].n, c->obs_ptr[l]});
        }
    kfold_plan::Plan plan;
    if (kfold_plan::build(owners, c->obs_idx.data(), fold, K, plan) != 0) return fail(c, DSMGP_E_ARG, "kfold: a label outside -1 .. K - 1");
    const size_t nblk = plan.blocks.size();
    std::vector<size_t> foff(nblk, 0), doff(nblk, 0), poff(nblk, 0);
    size_t ftot = 0, dtot = 0, pmax = 0;
    for (int32_t k = 0; k < K; ++k) {
        size_t pk = 0;
        for (int64_t b = plan.label_first[(size_t)k]; b < plan.label_first[(size_t)k + 1]; ++b) {
            const kfold_plan::Block& B = plan.blocks[(size_t)b];
            foff[(size_t)b] = ftot;
            doff[(size_t)b] = dtot;
            poff[(size_t)b] = pk;
            ftot += (size_t)B.mpad * B.mpad;
            dtot += (size_t)B.mpad * TB;
            pk += (size_t)B.mpad * c->leaves[owners[(size_t)B.owner].id].npad;
        }
        pmax = std::max(pmax, pk);
    }
    if (int rc = arena_status(c, c->arenaKP.grow(arena_pool(c), pmax))) return rc;
    if (int rc = arena_status(c, c->arenaKF.grow(arena_pool(c), ftot))) return rc;
    if (want_var)
        if (int rc = arena_status(c, c->arenaKX.grow(arena_pool(c), ftot))) return rc;
    if (int rc = c->d_kinfo.grow(c, std::max<size_t>(1, nblk))) return rc;
    if (int rc = c->d_kout.grow(c, 2 * nobs + (size_t)L * (size_t)K)) return rc;
    double* dmu = c->d_kout.p;
    double* dvar = dmu + nobs;
    double* dlpd = dvar + nobs;

    // rounds: panels and G_FF tiles of label k
    std::vector<KfoldPackTask> pack;
    std::vector<KfoldGffTask> gff;
    std::vector<size_t> pack_off((size_t)K + 1, 0), gff_off((size_t)K + 1, 0);
    std::vector<CholBlock> mats;
    mats.reserve(nblk);
    if (int rc = c->d_kpos.grow(c, std::max<size_t>(1, plan.pos.size()))) return rc;
    for (int32_t k = 0; k < K; ++k) {
        for (int64_t b = plan.label_first[(size_t)k]; b < plan.label_first[(size_t)k + 1]; ++b) {
            const kfold_plan::Block& B = plan.blocks[(size_t)b];
            const int ol = owners[(size_t)B.owner].id;
            const int npad = c->leaves[ol].npad, nbt = B.mpad / TB;
            const double* Xt = c->arenaX.p + c->gxoff[(size_t)ol];
            double* P = c->arenaKP.p + poff[(size_t)b];
            double* F = c->arenaKF.p + foff[(size_t)b];
            for (int i = 0; i < nbt; ++i) {
                const int kstart = plan.tile_first[(size_t)B.tile_off + (size_t)i] / TB * TB;
                for (int c0 = kstart; c0 < npad; c0 += 2 * TB) {
                    KfoldPackTask t{};
                    t.X = Xt;
                    t.P = P + (size_t)i * TB;
                    t.pos = c->d_kpos.p + B.pos_off + (size_t)i * TB;
                    t.ldx = npad;
                    t.ldp = B.mpad;
                    t.nrows = std::min(TB, B.m - i * TB);
                    t.col0 = c0;
                    t.col1 = std::min(c0 + 2 * TB, npad);
                    pack.push_back(t);
                }
                for (int j = 0; j <= i; ++j) {
                    KfoldGffTask g{};
                    g.gemm.A = P + (size_t)i * TB;
                    g.gemm.B = P + (size_t)j * TB;
                    g.gemm.C = F + (size_t)i * TB + (size_t)j * TB * B.mpad;
                    g.gemm.lda = g.gemm.ldb = g.gemm.ldc = B.mpad;
                    g.gemm.k0 = kstart;
                    g.gemm.k1 = npad;
                    g.na = std::min(TB, B.m - i * TB);
                    g.nb = std::min(TB, B.m - j * TB);
                    g.diag = (i == j);
                    gff.push_back(g);
                }
            }
        }
        pack_off[(size_t)k + 1] = pack.size();
        gff_off[(size_t)k + 1] = gff.size();
    }
    // behind the inverted diagonal blocks: -I, and the scratch tiles of the panel solves
    const size_t negi_off = dtot, scratch_off = dtot + (size_t)TB * TB;
    for (size_t b = 0; b < nblk; ++b) mats.push_back(CholBlock{nullptr, plan.blocks[b].m, plan.blocks[b].mpad, nullptr, nullptr});
    if (int rc = arena_status(c, c->arenaKD.grow(arena_pool(c), scratch_off + chol_blocks_scratch_tiles(mats) * TB * TB))) return rc;
    for (size_t b = 0; b < nblk; ++b) {
        mats[b].F = c->arenaKF.p + foff[b];
        mats[b].Dinv = c->arenaKD.p + doff[b];
        mats[b].info = c->d_kinfo.p + b;
    }
    CholSteps steps;
    chol_blocks_plan(mats, c->arenaKD.p + negi_off, c->arenaKD.p + scratch_off, steps);

    // C^-T of every block, and one task per (leaf, label) with rows
    KfoldInverseTasks inv;
    if (want_var) kfold_inverse_tasks(mats, c->arenaKX.p, foff, steps.nsteps, inv);
    std::vector<KfoldMomTask> mom;
    std::vector<size_t> work_off;           // per task: its w | v in d_kwork
    size_t wtot = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (finfo[(size_t)l] != 0 || owner_at[(size_t)lf.owner] < 0) continue;
        const int al = (lf.op == DSMGP_SHARE_COPY && lf.mean == c->leaves[lf.src].mean) ? lf.src : l;   // LooTask's rule
        for (int32_t k = 0; k < K; ++k) {
            const int32_t b = plan.find((size_t)owner_at[(size_t)lf.owner], k);
            if (b < 0) continue;
            const kfold_plan::Block& B = plan.blocks[(size_t)b];
            KfoldMomTask t{};
            t.C = mats[(size_t)b].F;
            t.Xc = want_var ? c->arenaKX.p + foff[(size_t)b] : nullptr;
            t.pos = c->d_kpos.p + B.pos_off;
            t.alpha = c->h_leaves[al].alpha;
            t.info = c->d_kinfo.p + b;
            t.lpd = dlpd + (size_t)l + (size_t)k * (size_t)L;
            t.off = (long long)c->obs_ptr[l];
            t.m = B.m;
            t.mpad = B.mpad;
            mom.push_back(t);
            work_off.push_back(wtot);
            wtot += 2 * (size_t)B.mpad;
        }
    }
    if (int rc = c->d_kwork.grow(c, std::max<size_t>(1, wtot))) return rc;
    for (size_t i = 0; i < mom.size(); ++i) mom[i].work = c->d_kwork.p + work_off[i];

    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    if (int rc = stage_upload_list(c, c->kpack, pack)) return rc;
    if (int rc = stage_upload_list(c, c->kgff, gff)) return rc;
    CholLists lists{c->kupd, c->ktrsm, c->kres, c->ktrsm2, c->kadd, c->kdiag};
    if (int rc = chol_blocks_upload(c, steps, lists)) return rc;
    if (int rc = stage_upload_list(c, c->kxtrans, inv.trans)) return rc;
    if (int rc = stage_upload_list(c, c->kxupd, inv.upd)) return rc;
    if (int rc = stage_upload_list(c, c->kxtrsm, inv.trsm)) return rc;
    if (int rc = stage_upload_list(c, c->kmom, mom)) return rc;
    if (int rc = stage_upload(c, c->d_kpos.p, plan.pos.data(), plan.pos.size() * sizeof(int32_t))) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_kinfo.p, 0, std::max<size_t>(1, nblk) * sizeof(int), c->stream));
    HIPCHK(c, hipMemsetAsync(c->arenaKD.p, 0, std::max<size_t>(1, dtot) * sizeof(double), c->stream));
    if (int rc = chol_blocks_negi(c, steps, c->arenaKD.p + negi_off)) return rc;
    HIPCHK(c, hipMemsetAsync(dmu, 0xff, std::max<size_t>(1, 2 * nobs) * sizeof(double), c->stream));   // NaN: rows no block holds
    HIPCHK(c, hipMemsetAsync(dlpd, 0, (size_t)L * (size_t)K * sizeof(double), c->stream));             // empty blocks

    EventPair e01, e23, e4;     // e01.a .. e01.b L^-T, .. e23.a pack and G_FF, .. e23.b factorisation, .. e4.a inversion and moments
    HIPCHK(c, e01.init());
    HIPCHK(c, e23.init());
    HIPCHK(c, e4.init());
    HIPCHK(c, hipEventRecord(e01.a, c->stream));
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = ensure_alpha(c)) return rc;
    if (int rc = xinv_fill(c)) return rc;
    HIPCHK(c, hipEventRecord(e01.b, c->stream));
    for (int32_t k = 0; k < K; ++k) {
        const size_t np = pack_off[(size_t)k + 1] - pack_off[(size_t)k], ng = gff_off[(size_t)k + 1] - gff_off[(size_t)k];
        if (np) kfold_pack_kernel<<<(unsigned)np, 256, 0, c->stream>>>(c->kpack.p + pack_off[(size_t)k]);
        if (ng) kfold_gff_kernel<<<(unsigned)ng, 256, 0, c->stream>>>(c->kgff.p + gff_off[(size_t)k]);
    }
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(e23.a, c->stream));
    chol_blocks_run(c, steps, lists);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(e23.b, c->stream));
    if (want_var) {
        if (!inv.trans.empty()) transpose_tile_kernel<<<(unsigned)inv.trans.size() * 16, 256, 0, c->stream>>>(c->kxtrans.p);
        for (size_t s = 0; s + 1 < inv.step_off.size(); ++s) {
            const int n = (int)(inv.step_off[s + 1] - inv.step_off[s]);
            if (n == 0) continue;
            launch_tiles(c, c->kxupd.p + inv.step_off[s], n);
            launch_tiles(c, c->kxtrsm.p + inv.step_off[s], n, 1);
        }
    }
    if (!mom.empty())
        kfold_moments_kernel<<<(unsigned)mom.size(), 256, 0, c->stream>>>(c->kmom.p, c->d_obs_idx.p, c->dy.p, dmu, dvar);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(e4.a, c->stream));
    std::vector<int> binfo(std::max<size_t>(1, nblk), 0);
    HIPCHK(c, hipMemcpyAsync(binfo.data(), c->d_kinfo.p, std::max<size_t>(1, nblk) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (int rc = stage_done(c)) return rc;
    c->mark(P_XINV);
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, e01.a, e4.a));
    if (seconds) *seconds = ms * 1e-3;
    // the four parts add up to the call's time: with L^-T current part [0] is 0 by definition, and what was left to complete of
    // the diagonal-block inverses and alpha (e01.a .. e01.b then) counts with part [1]
    HIPCHK(c, hipEventElapsedTime(&ms, e01.a, e01.b));
    c->kfold_seconds[0] = had_xinv ? 0.0 : ms * 1e-3;
    HIPCHK(c, hipEventElapsedTime(&ms, had_xinv ? e01.a : e01.b, e23.a));
    c->kfold_seconds[1] = ms * 1e-3;
    HIPCHK(c, hipEventElapsedTime(&ms, e23.a, e23.b));
    c->kfold_seconds[2] = ms * 1e-3;
    HIPCHK(c, hipEventElapsedTime(&ms, e23.b, e4.a));
    c->kfold_seconds[3] = ms * 1e-3;
    if (mu_out) HIPCHK(c, hipMemcpy(mu_out, dmu, nobs * sizeof(double), hipMemcpyDeviceToHost));
    if (var_out) HIPCHK(c, hipMemcpy(var_out, dvar, nobs * sizeof(double), hipMemcpyDeviceToHost));
    if (lpd_out) HIPCHK(c, hipMemcpy(lpd_out, dlpd, (size_t)L * (size_t)K * sizeof(double), hipMemcpyDeviceToHost));
    // per (leaf, label): -1 and NaN where the leaf's fit failed, else the block's flag (0 for an empty block)
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int l = 0; l < L; ++l) {
        const bool failed = finfo[(size_t)l] != 0;
        const int oa = owner_at[(size_t)c->leaves[l].owner];
        for (int32_t k = 0; k < K; ++k) {
            const size_t at = (size_t)l + (size_t)k * (size_t)L;
            if (failed) {
                if (lpd_out) lpd_out[at] = qnan;
                if (info_out) info_out[at] = -1;
                continue;
            }
            const int32_t b = oa >= 0 ? plan.find((size_t)oa, k) : -1;
            if (info_out) info_out[at] = b >= 0 ? binfo[(size_t)b] : 0;
        }
    }
    return 0;
}

int dsmgp_kfold_stats(dsmgp_ctx* c, int64_t* out) {
    if (!c || !out) return DSMGP_E_ARG;
    const DevArena* a[4] = {&c->arenaKP, &c->arenaKF, &c->arenaKD, &c->arenaKX};
    for (int i = 0; i < 4; ++i) out[i] = (int64_t)(a[i]->p ? a[i]->cap * sizeof(double) : 0);
    return 0;
}

int dsmgp_kfold_seconds(dsmgp_ctx* c, double* out) {
    if (!c || !out) return DSMGP_E_ARG;
    for (int i = 0; i < 4; ++i) out[i] = c->kfold_seconds[i];
    return 0;
}

// Input gradients of the predictive moments (the kernels and the formulas: kernels.hpp at tile_predbeta_kernel).  The mean half
// reads alpha and the gathered inputs only.  The variance half needs beta_t = K_y^-1 k_t for every routed row: B = Vt L^-1 by a
// tile GEMM against the L^-T arena (dsmgp_loo's rule for filling it), into an arena of its own -- Vt stays for dsmgp_predict_cov.
// Nothing any other entry point reads is written.
namespace {
// The device part: dmu (and dvar with `var`) of every routed row into d_pgout, no host copy.  route_total > 0.
static int predict_gradients_device(dsmgp_ctx* c, bool var, double* seconds) {
    const size_t nr = (size_t)c->route_total;
    HIPCHK(c, hipSetDevice(c->device));
    const int L = c->L, D = c->D;
    if (var) c->invalidate(P_PGRAD);    // until both halves are written again
    OwnGradLists own_lists{c};
    std::vector<size_t> boff((size_t)L, 0);
    if (var) {
        if (int rc = xinv_lists(c, own_lists)) return rc;
        size_t bTot = 0;
        for (int l = 0; l < L; ++l) {
            const LeafHost& lf = c->leaves[l];
            if (lf.nt == 0) continue;
            boff[l] = bTot;
            bTot += (size_t)lf.ntpad * lf.npad;
        }
        if (int rc = arena_status(c, c->arenaB.grow(arena_pool(c), bTot))) return rc;
    }
    // task lists: the tiles of B; per test tile its slabs of training rows, next to each other in the list and in d_pgpart
    const size_t planes = (var ? 2 : 1) * (size_t)D * TB;
    std::vector<PredBetaTask> beta;
    std::vector<PredGradTask> tasks;
    std::vector<PredGradFinTask> fin;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        const int nslab = (lf.n + PGRAD_SLAB - 1) / PGRAD_SLAB;
        for (int i = 0; i < lf.ntpad / TB; ++i) {
            PredGradFinTask f{};
            f.nslab = nslab;
            f.nrows = std::min(TB, lf.nt - i * TB);
            fin.push_back(f);
            for (int s = 0; s < nslab; ++s) tasks.push_back(PredGradTask{});
        }
    }
    if (int rc = c->d_pgpart.grow(c, tasks.size() * planes)) return rc;
    if (int rc = c->d_pgout.grow(c, (var ? 2 : 1) * nr * (size_t)D)) return rc;
    size_t ti = 0, fi = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        const LeafDev& d = c->h_leaves[l];
        const int nslab = (lf.n + PGRAD_SLAB - 1) / PGRAD_SLAB;
        double* Bl = var ? c->arenaB.p + boff[l] : nullptr;
        for (int i = 0; i < lf.ntpad / TB; ++i) {
            PredGradFinTask& f = fin[fi++];
            f.part = c->d_pgpart.p + ti * planes;
            f.xt = d.Xtg + (size_t)i * TB;
            f.dmu = c->d_pgout.p + (size_t)lf.route_off + (size_t)i * TB;
            f.dvar = var ? f.dmu + nr * (size_t)D : nullptr;
            f.info = d.info;
            f.pstride = (long long)planes;
            f.ldo = (long long)nr;
            f.ldt = lf.ntpad;
            f.kid = lf.kid;
            for (int s = 0; s < nslab; ++s) {
                PredGradTask& g = tasks[ti];
                g.xt = f.xt;
                g.xg = d.Xg;
                g.alpha = d.alpha;
                g.B = var ? Bl + (size_t)i * TB : nullptr;
                g.part = c->d_pgpart.p + ti * planes;
                g.ldt = lf.ntpad;
                g.ldg = lf.npad;
                g.nrows = f.nrows;
                g.c0 = s * PGRAD_SLAB;
                g.c1 = std::min(lf.n, g.c0 + PGRAD_SLAB);
                g.kid = lf.kid;
                ++ti;
            }
            if (!var) continue;
            const LeafHost& ow = c->leaves[lf.owner];       // a COPY leaf: its source's L^-T, its own Vt
            for (int j = 0; j * TB < lf.n; ++j) {
                PredBetaTask b{};
                b.gemm.A = d.Vt + (size_t)i * TB;
                b.gemm.B = c->arenaX.p + c->gxoff[lf.owner] + (size_t)j * TB;
                b.gemm.C = Bl + (size_t)i * TB + (size_t)j * TB * lf.ntpad;
                b.gemm.lda = b.gemm.ldc = lf.ntpad;
                b.gemm.ldb = ow.npad;
                b.gemm.k0 = j * TB;
                b.gemm.k1 = lf.n - lf.n % KC2;
                b.n = lf.n;
                beta.push_back(b);
            }
        }
    }
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    if (int rc = stage_upload_list(c, c->pgbeta, beta)) return rc;
    if (int rc = stage_upload_list(c, c->pgtasks, tasks)) return rc;
    if (int rc = stage_upload_list(c, c->pgfin, fin)) return rc;
    if (int rc = stage_done(c)) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = ensure_alpha(c)) return rc;
    if (var) {
        if (int rc = xinv_fill(c)) return rc;
        tile_predbeta_kernel<<<(unsigned)beta.size(), 256, 0, c->stream>>>(c->pgbeta.p);
        pred_inputgrad_kernel<true><<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->pgtasks.p, c->d_kp.p, D);
        if (any_rq(c)) pred_inputgrad_rq_kernel<true><<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->pgtasks.p, c->d_kp.p, D);
    } else {
        pred_inputgrad_kernel<false><<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->pgtasks.p, c->d_kp.p, D);
        if (any_rq(c)) pred_inputgrad_rq_kernel<false><<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->pgtasks.p, c->d_kp.p, D);
    }
    pred_inputgrad_finish_kernel<<<(unsigned)fin.size(), 128, 0, c->stream>>>(c->pgfin.p, c->d_kp.p, D);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (var) {
        c->mark(P_XINV);
        c->mark(P_PGRAD);   // both halves are this prediction's (a mean-only call later writes the same dmu into the same place)
    }
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    return 0;
}
}  // namespace

int dsmgp_predict_gradients(dsmgp_ctx* c, double* dmu_out, double* dvar_out, int64_t ld, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "predict_gradients before predict_run on the current fit");
    const size_t nr = (size_t)c->route_total;
    if (nr == 0) return 0;
    if (ld < c->route_total) return fail(c, DSMGP_E_ARG, "predict_gradients: ld < route_total");
    const int D = c->D;
    if (int rc = predict_gradients_device(c, dvar_out != nullptr, seconds)) return rc;
    if (dmu_out)
        HIPCHK(c, hipMemcpy2D(dmu_out, (size_t)ld * sizeof(double), c->d_pgout.p, nr * sizeof(double), nr * sizeof(double), (size_t)D,
                              hipMemcpyDeviceToHost));
    if (dvar_out)
        HIPCHK(c, hipMemcpy2D(dvar_out, (size_t)ld * sizeof(double), c->d_pgout.p + nr * (size_t)D, nr * sizeof(double),
                              nr * sizeof(double), (size_t)D, hipMemcpyDeviceToHost));
    return 0;
}

// Several target columns on the current factors (kernels_targets.hpp).  Z = L^-1 (Y[obs] - mean) for every leaf by a
// right-looking block sweep on the matrix cores, one launch per block column and lane, every factor tile read once; then the
// per-(leaf, column) log-marginals.  Writes its own arena only: z, alpha and everything else a fit left stay as they are
// (ensure_dinv completes Dinv as every other reader of it does).
namespace {
static int build_targets_plan(dsmgp_ctx* c, int qpad) {      // (static: inside extern "C" an unnamed namespace alone still exports the name)
    const int L = c->L;
    c->invalidate(P_TG_LISTS);
    c->toff.assign((size_t)L, 0);
    size_t tot = 0;
    int maxnb = 0;
    for (int l = 0; l < L; ++l) {
        c->toff[(size_t)l] = tot;
        tot += 2 * (size_t)c->leaves[l].npad * (size_t)qpad;
        maxnb = std::max(maxnb, c->leaves[l].nb);
    }
    if (int rc = arena_status(c, c->arenaT.grow(arena_pool(c), tot))) {
        (void)hipGetLastError();
        return rc;
    }
    std::vector<long long> ho((size_t)L);
    for (int l = 0; l < L; ++l) ho[(size_t)l] = (long long)c->toff[(size_t)l];
    if (int rc = dev_upload(c, c->d_toff, ho)) return rc;
    // launch 0: Z_0 = Dinv_0 Yc_0 of every leaf; launch s >= 1: block column k = s - 1, the tasks of blocks i = k + 1 .. nb - 1,
    // that of i = k + 1 going on to Z_i.  A COPY leaf reads its source's factor (h_leaves: F / Dinv alias) and has blocks of its own.
    const int nl = c->nlanes, ns = maxnb;
    std::vector<TargetsFwdTask> tasks;
    c->tfwd_off.assign((size_t)nl * ns + 1, 0);
    for (int q = 0; q < nl; ++q)
        for (int s = 0; s < ns; ++s) {
            c->tfwd_off[(size_t)q * ns + s] = (int)tasks.size();
            for (int l = 0; l < L; ++l) {
                const LeafHost& lf = c->leaves[l];
                if ((nl > 1 && c->leaf_lane[l] != q) || lf.nb <= s) continue;
                const LeafDev& d = c->h_leaves[l];
                double* yc = c->arenaT.p + c->toff[(size_t)l];
                double* z = yc + (size_t)lf.npad * qpad;
                TargetsFwdTask t{};
                t.ldt = t.ldz = lf.npad;
                t.qpad = qpad;
                if (s == 0) {
                    t.src = yc;
                    t.dst = z;
                    t.Dinv = d.Dinv;
                    t.nrows = std::min(TB, lf.n);
                    tasks.push_back(t);
                    continue;
                }
                const int k = s - 1;
                for (int i = k + 1; i < lf.nb; ++i) {
                    t.T = d.F + (size_t)i * TB + (size_t)k * TB * lf.npad;
                    t.Zk = z + (size_t)k * TB;
                    t.src = (k == 0 ? yc : z) + (size_t)i * TB;
                    t.dst = z + (size_t)i * TB;
                    t.Dinv = i == k + 1 ? d.Dinv + (size_t)i * TB * TB : nullptr;
                    t.nrows = std::min(TB, lf.n - i * TB);
                    tasks.push_back(t);
                }
            }
        }
    c->tfwd_off[(size_t)nl * ns] = (int)tasks.size();
    if (int rc = dev_upload(c, c->tfwd, tasks)) return rc;
    c->tfwd_steps = ns;
    c->tfwd_lanes = nl;
    c->tg_qpad = qpad;
    c->mark(P_TG_LISTS);
    return 0;
}
}  // namespace

int dsmgp_solve_targets(dsmgp_ctx* c, const double* Y, int64_t N, int32_t Q, int64_t ldy, const double* mean, double* mll_out,
                        double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "solve_targets before fit");
    if (!Y || N != c->N || Q < 1 || Q > 65535 || ldy < N)
        return fail(c, DSMGP_E_ARG, "solve_targets: Y is NULL, N is not the N of set_train, Q outside 1 .. 65535 or ldy < N");
    const int L = c->L;
    for (int32_t j = 0; j < Q; ++j)
        for (int64_t i = 0; i < N; ++i)
            if (!std::isfinite(Y[i + (size_t)j * ldy])) return fail(c, DSMGP_E_ARG, "solve_targets: non-finite value in Y");
    if (mean)
        for (size_t i = 0; i < (size_t)L * Q; ++i)
            if (!std::isfinite(mean[i])) return fail(c, DSMGP_E_ARG, "solve_targets: non-finite value in mean");
    HIPCHK(c, hipSetDevice(c->device));
    const int qpad = round_up(Q, TQ);
    if (!c->has(P_TG_LISTS) || c->tg_qpad != qpad)
        if (int rc = build_targets_plan(c, qpad)) return rc;
    c->invalidate(P_Z);
    if (int rc = c->d_tY.grow(c, (size_t)N * Q)) return rc;
    if (int rc = c->d_tmean.grow(c, (size_t)L * Q)) return rc;
    if (int rc = c->d_tmll.grow(c, (size_t)L * Q)) return rc;
    HIPCHK(c, hipMemcpy2D(c->d_tY.p, (size_t)N * sizeof(double), Y, (size_t)ldy * sizeof(double), (size_t)N * sizeof(double),
                          (size_t)Q, hipMemcpyHostToDevice));
    if (mean) HIPCHK(c, hipMemcpy(c->d_tmean.p, mean, (size_t)L * Q * sizeof(double), hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemset(c->d_tmean.p, 0, (size_t)L * Q * sizeof(double)));
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = ensure_dinv(c)) return rc;       // the diagonal solves multiply with the whole Dinv_k
    {
        int maxpad = 0;
        for (auto& lf : c->leaves) maxpad = std::max(maxpad, lf.npad);
        for_leaf_chunks((size_t)L, [&](size_t leaf0, size_t cnt) {
            targets_gather_kernel<<<dim3((maxpad + 255) / 256, (unsigned)cnt), 256, 0, c->stream>>>(
                c->d_leaves.p, c->d_obs_ptr.p, c->d_obs_idx.p, c->d_tY.p, N, Q, qpad, c->d_tmean.p, L, c->arenaT.p, c->d_toff.p,
                (int)leaf0);
        });
    }
    if (int rc = fork_lanes(c, c->tfwd_lanes)) return rc;
    for (int s = 0; s < c->tfwd_steps; ++s)
        for (int lane = 0; lane < c->tfwd_lanes; ++lane) {
            const int v = lane * c->tfwd_steps + s;
            const int nt = c->tfwd_off[(size_t)v + 1] - c->tfwd_off[(size_t)v];
            if (nt > 0) targets_fwd_kernel<<<nt, 256, 0, c->lane_stream[lane]>>>(c->tfwd.p + c->tfwd_off[(size_t)v]);
        }
    if (int rc = join_lanes(c, c->tfwd_lanes)) return rc;
    targets_mll_kernel<<<dim3(L, Q), 256, 0, c->stream>>>(c->d_leaves.p, c->arenaT.p, c->d_toff.p, qpad, L, c->d_tmll.p);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    c->tg_Q = Q;
    c->mark(P_Z);
    if (mll_out) HIPCHK(c, hipMemcpy(mll_out, c->d_tmll.p, (size_t)L * Q * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

namespace {
// The device part: the means of every resident column per routed row into d_tmu, no host copy.  route_total > 0.
static int predict_targets_device(dsmgp_ctx* c, double* seconds) {
    const size_t nr = (size_t)c->route_total;
    HIPCHK(c, hipSetDevice(c->device));
    const int L = c->L, Q = c->tg_Q, qpad = c->tg_qpad;
    c->invalidate(P_TMU);
    if (int rc = c->d_tmu.grow(c, nr * (size_t)Q)) return rc;
    std::vector<TargetsMuTask> tasks;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        const LeafDev& d = c->h_leaves[l];
        for (int i = 0; i < lf.ntpad / TB; ++i) {
            TargetsMuTask t{};
            t.Vt = d.Vt + (size_t)i * TB;
            t.Z = c->arenaT.p + c->toff[(size_t)l] + (size_t)lf.npad * qpad;
            t.out = c->d_tmu.p + (size_t)lf.route_off + (size_t)i * TB;
            t.info = d.info;
            t.ldo = (long long)nr;
            t.ldv = lf.ntpad;
            t.ldz = lf.npad;
            t.n = lf.n;
            t.nrows = std::min(TB, lf.nt - i * TB);
            t.leaf = l;
            tasks.push_back(t);
        }
    }
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    if (int rc = stage_upload_list(c, c->tmu, tasks)) return rc;
    if (int rc = stage_done(c)) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    targets_mu_kernel<<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->tmu.p, c->d_tmean.p, L, Q, qpad);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    c->mark(P_TMU);
    return 0;
}
}  // namespace

int dsmgp_predict_targets(dsmgp_ctx* c, double* mu_out, int64_t ld, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "predict_targets before solve_targets on the current fit");
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "predict_targets before predict_run on the current fit");
    const size_t nr = (size_t)c->route_total;
    if (nr == 0) return 0;
    if (!mu_out || ld < c->route_total) return fail(c, DSMGP_E_ARG, "predict_targets: mu_out is NULL or ld < route_total");
    if (int rc = predict_targets_device(c, seconds)) return rc;
    HIPCHK(c, hipMemcpy2D(mu_out, (size_t)ld * sizeof(double), c->d_tmu.p, nr * sizeof(double), nr * sizeof(double), (size_t)c->tg_Q,
                          hipMemcpyDeviceToHost));
    return 0;
}

int dsmgp_targets_fetch(dsmgp_ctx* c, int32_t leaf, double* Z_out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "targets_fetch before solve_targets on the current fit");
    if (leaf < 0 || leaf >= c->L || !Z_out) return fail(c, DSMGP_E_ARG, "targets_fetch: leaf out of range or Z_out is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    const LeafHost& lf = c->leaves[leaf];
    const double* z = c->arenaT.p + c->toff[(size_t)leaf] + (size_t)lf.npad * c->tg_qpad;
    HIPCHK(c, hipMemcpy2D(Z_out, (size_t)lf.n * sizeof(double), z, (size_t)lf.npad * sizeof(double), (size_t)lf.n * sizeof(double),
                          (size_t)c->tg_Q, hipMemcpyDeviceToHost));
    return 0;
}

namespace {
// An arena of npad x Qpad doubles per leaf at offset toff / 2 (A, U): grown on first use, from the pool when there is one
// (static, like build_targets_plan: inside extern "C" an unnamed namespace alone still exports the name)
static int targets_slab(dsmgp_ctx* c, DevArena& a, const char* what) {
    size_t tot = 0;
    for (int l = 0; l < c->L; ++l) tot += (size_t)c->leaves[l].npad * (size_t)c->tg_qpad;
    if (int rc = arena_status(c, a.grow(arena_pool(c), tot))) {
        (void)hipGetLastError();
        return rc == DSMGP_E_NOMEM ? rc : fail(c, DSMGP_E_NOMEM, std::string(what) + " (" + std::to_string((tot * 8) >> 20) + " MiB)");
    }
    return 0;
}
// The tasks of A = L^-T Z (targets_a_kernel), one per 128-row block of every leaf; arenaA must be there
static void targets_a_tasks(const dsmgp_ctx* c, std::vector<TargetsATask>& ta) {
    ta.clear();
    for (int l = 0; l < c->L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const double* Xt = c->arenaX.p + c->gxoff[(size_t)lf.owner];
        for (int i = 0; i < lf.nb; ++i) {
            TargetsATask t{};
            t.Xt = Xt + (size_t)i * TB;
            t.Z = c->arenaT.p + c->toff[(size_t)l] + (size_t)lf.npad * c->tg_qpad;
            t.A = c->arenaA.p + c->toff[(size_t)l] / 2 + (size_t)i * TB;
            t.ldt = c->leaves[lf.owner].npad;
            t.ldz = lf.npad;
            t.k0 = i * TB;
            t.n = lf.n;
            t.nrows = std::max(0, std::min(TB, lf.n - i * TB));
            ta.push_back(t);
        }
    }
}
}  // namespace

// Input gradients of the predictive means of the resident target columns (kernels_targets.hpp at targets_inputgrad_kernel): A as
// dsmgp_mll_columns_gradients obtains it (L^-T by dsmgp_loo's rule, targets_a_kernel into arenaA), then one matrix product per
// dimension with the kernel derivatives made in registers.  A COPY leaf reads its source's L^-T with its own Z.  The lists are
// rebuilt per call; the partial sums and the output live in buffers of this entry point (TestProducts): nothing another entry point
// reads is written, and the mask of dsmgp_set_gradient_leaves neither applies nor changes.
namespace {
// The device part: the input gradients of the columns' means into d_tigout, no host copy.  route_total > 0.
static int predict_columns_gradients_device(dsmgp_ctx* c, double* seconds) {
    const size_t nr = (size_t)c->route_total;
    HIPCHK(c, hipSetDevice(c->device));
    const int L = c->L, D = c->D, Q = c->tg_Q, qpad = c->tg_qpad;
    c->invalidate(P_TIG);
    // L^-T of every factor owner (xinv_lists / xinv_fill); lists of the call's own are dropped again on every way out
    OwnGradLists own_lists{c};
    if (int rc = xinv_lists(c, own_lists)) return rc;
    if (int rc = targets_slab(c, c->arenaA, "predict_targets_gradients: no room for A = L^-T Z")) return rc;
    std::vector<TargetsATask> ta;
    targets_a_tasks(c, ta);
    // per test tile its slabs of training rows, next to each other in the list and in d_tigpart
    const size_t planes = (size_t)D * (size_t)qpad * TB;
    std::vector<TargetsInputGradTask> tasks;
    std::vector<TargetsInputGradFinTask> fin;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        const int nslab = (lf.n + TIG_SLAB - 1) / TIG_SLAB;
        fin.resize(fin.size() + (size_t)(lf.ntpad / TB));
        tasks.resize(tasks.size() + (size_t)(lf.ntpad / TB) * (size_t)nslab);
    }
    if (int rc = c->d_tigpart.grow(c, tasks.size() * planes)) return rc;
    if (int rc = c->d_tigout.grow(c, nr * (size_t)D * (size_t)Q)) return rc;
    size_t ti = 0, fi = 0;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.nt == 0) continue;
        const LeafDev& d = c->h_leaves[l];
        const int nslab = (lf.n + TIG_SLAB - 1) / TIG_SLAB;
        for (int i = 0; i < lf.ntpad / TB; ++i) {
            TargetsInputGradFinTask& f = fin[fi++];
            f = TargetsInputGradFinTask{};
            f.part = c->d_tigpart.p + ti * planes;
            f.out = c->d_tigout.p + (size_t)lf.route_off + (size_t)i * TB;
            f.info = d.info;
            f.pstride = (long long)planes;
            f.ldo = (long long)nr;
            f.nslab = nslab;
            f.nrows = std::min(TB, lf.nt - i * TB);
            for (int s = 0; s < nslab; ++s) {
                TargetsInputGradTask& g = tasks[ti];
                g = TargetsInputGradTask{};
                g.xt = d.Xtg + (size_t)i * TB;
                g.xg = d.Xg;
                g.A = c->arenaA.p + c->toff[(size_t)l] / 2;
                g.part = c->d_tigpart.p + ti * planes;
                g.ldt = lf.ntpad;
                g.ldg = lf.npad;
                g.nrows = f.nrows;
                g.c0 = s * TIG_SLAB;
                g.c1 = std::min(lf.n, g.c0 + TIG_SLAB);
                g.kid = lf.kid;
                ++ti;
            }
        }
    }
    if (int rc = dev_upload(c, c->tga, ta)) return rc;
    c->stage_top = 0;       // (the stream is idle: every entry point synchronises before it returns)
    if (int rc = stage_upload_list(c, c->tigtasks, tasks)) return rc;
    if (int rc = stage_upload_list(c, c->tigfin, fin)) return rc;
    if (int rc = stage_done(c)) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = xinv_fill(c)) return rc;
    if (!ta.empty()) targets_a_kernel<<<(unsigned)ta.size(), 256, 0, c->stream>>>(c->tga.p, qpad);
    targets_inputgrad_kernel<<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->tigtasks.p, c->d_kp.p, D, qpad);
    if (any_rq(c)) targets_inputgrad_rq_kernel<<<(unsigned)tasks.size(), 256, 0, c->stream>>>(c->tigtasks.p, c->d_kp.p, D, qpad);
    targets_inputgrad_finish_kernel<<<dim3((unsigned)fin.size(), (unsigned)Q), 128, 0, c->stream>>>(c->tigfin.p, D, qpad);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_XINV);
    c->mark(P_TIG);
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    return 0;
}
}  // namespace

int dsmgp_predict_columns_gradients(dsmgp_ctx* c, double* dmu_out, int64_t ld, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "predict_targets_gradients before solve_targets on the current fit");
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "predict_targets_gradients before predict_run on the current fit");
    const size_t nr = (size_t)c->route_total;
    if (nr == 0) return 0;
    if (!dmu_out || ld < c->route_total) return fail(c, DSMGP_E_ARG, "predict_targets_gradients: dmu_out is NULL or ld < route_total");
    if (int rc = predict_columns_gradients_device(c, seconds)) return rc;
    HIPCHK(c, hipMemcpy2D(dmu_out, (size_t)ld * sizeof(double), c->d_tigout.p, nr * sizeof(double), nr * sizeof(double),
                          (size_t)c->D * (size_t)c->tg_Q, hipMemcpyDeviceToHost));
    return 0;
}

// -------------------------------------------------------------------------------------------------
// predict(model, x): aggregation over the leaves of every test row on the device -- the moments, their input gradients, and both
// for every resident target column.  The arithmetic of a family, the kernels and the layout of the sums: kernels_agg.hpp; this
// section checks the arguments, keeps the resident family, makes the per-entry products a call reads, launches and downloads.
//   single y    family, coefficients and groups are those of the last dsmgp_aggregate_partial (c->agg, d_agg_*), resident since;
//               the gradient calls read the per-entry gradients d_pgout.  Sums and results have buffers of their own: nothing
//               another entry point reads is written.
//   columns     a state of their own beside it (c->col, d_col_*): d_agg_* and what dsmgp_scores / dsmgp_aggregate_finish answer
//               stay as they are.  One context only: no partial / finish split.
namespace {
int agg_width(int family, int G, int D = 1) { return (family == AGG_MIXTURE ? 3 : (family == AGG_RBCM ? 2 * G : 2)) * D; }

static AggState agg_state(int family, int n_groups) {
    const int G = family == AGG_RBCM ? n_groups : 0;
    return AggState{family, G, agg_width(family, G)};
}

// The family, coefficient and group arguments of the two calls that take them
static int agg_family_check(dsmgp_ctx* c, int family, const double* leaf_coef, const int32_t* leaf_group, int n_groups,
                            const std::string& who) {
    if (family < AGG_MIXTURE || family > AGG_RBCM) return fail(c, DSMGP_E_ARG, who + ": unknown family");
    if (family == AGG_RBCM) {
        if (!leaf_group || n_groups <= 0 || n_groups > 4096) return fail(c, DSMGP_E_ARG, who + ": rBCM needs leaf groups");
        for (int l = 0; l < c->L; ++l)
            if (leaf_group[l] < 0 || leaf_group[l] >= n_groups) return fail(c, DSMGP_E_ARG, who + ": leaf group out of range");
    } else if (!leaf_coef) {
        return fail(c, DSMGP_E_ARG, who + ": leaf_coef is NULL");
    }
    return 0;
}

// rBCM: the prior is the kernel id of the model's first leaf
static int agg_prior_check(dsmgp_ctx* c, int family, int prior_kernel_id, const std::string& who) {
    if (family != AGG_RBCM) return 0;
    if (prior_kernel_id < 0 || prior_kernel_id >= (int)c->hyper.size() || c->hyper[prior_kernel_id].kind < 0)
        return fail(c, DSMGP_E_ARG, who + ": rBCM needs the kernel id of the model's first leaf");
    if (ard_linear_short(c, prior_kernel_id))
        return fail(c, DSMGP_E_ARG, who + ": " + KINDS[c->hyper[prior_kernel_id].kind].name + " needs one lengthscale per input dimension");
    return 0;
}

static int agg_upload(dsmgp_ctx* c, int family, const double* leaf_coef, const int32_t* leaf_group, double* d_coef, int32_t* d_group) {
    const size_t L = (size_t)c->L;
    if (leaf_coef) HIPCHK(c, hipMemcpyAsync(d_coef, leaf_coef, L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (family == AGG_RBCM) HIPCHK(c, hipMemcpyAsync(d_group, leaf_group, L * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    return 0;
}

// What every kernel that walks the entries reads, for the resident family `s` with its coefficients and groups; the caller adds
// the arrays of its own (the columns: mu = d_tmu).
static AggArgs agg_args(dsmgp_ctx* c, const AggState& s, const double* d_coef, const int32_t* d_group, int plain = 0,
                        int prior_kernel_id = 0) {
    AggArgs a{};
    a.rows = AggRows{c->d_row_ptr.p, c->d_row_ent.p, c->d_ent_leaf.p};
    a.mu = c->arenaPV.p;
    a.var = c->arenaPV.p + (size_t)c->route_total;
    a.coef = d_coef;
    a.group = d_group;
    a.kp = c->d_kp.p;
    a.Xt = c->dXt.p;
    a.n_t = c->n_t;
    a.ld = c->route_total;
    a.D = c->D;
    a.Q = c->tg_Q;
    a.family = s.family;
    a.G = s.G;
    a.plain = plain ? 1 : 0;
    a.prior_kid = s.family == AGG_RBCM ? prior_kernel_id : 0;
    return a;
}

// Make a per-entry product with `make(&its device seconds)` unless it is this prediction's already; the time is added to
// `seconds`.  With no entry there is nothing to make: `mark_empty` then marks it current (the columns' gradient call never did).
static int agg_ensure(dsmgp_ctx* c, Product p, bool mark_empty, double& seconds, const std::function<int(double*)>& make) {
    if (c->has(p)) return 0;
    if (!c->route_total) {
        if (mark_empty) c->mark(p);
        return 0;
    }
    double s = 0.0;
    const int rc = make(&s);
    seconds += s;
    return rc;
}

// `cols` planes of n_t doubles to the caller's matrix of leading dimension ld; a NULL destination takes nothing
static hipError_t agg_download(dsmgp_ctx* c, double* dst, int64_t ld, const double* d_src, size_t cols) {
    if (!dst) return hipSuccess;
    const size_t w = (size_t)c->n_t * sizeof(double);
    return hipMemcpy2DAsync(dst, (size_t)ld * sizeof(double), d_src, w, w, cols, hipMemcpyDeviceToHost, c->stream);
}

static dim3 agg_grid(dsmgp_ctx* c, int ny = 1) { return dim3((unsigned)((c->n_t + 255) / 256), (unsigned)ny); }
}  // namespace

int dsmgp_aggregate_partial(dsmgp_ctx* c, int32_t family, const double* leaf_coef, const int32_t* leaf_group,
                            int32_t n_groups, double* partial_out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "aggregate before predict_run");
    if (int rc = agg_family_check(c, family, leaf_coef, leaf_group, n_groups, "aggregate")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const AggState s = agg_state(family, n_groups);
    const size_t need = (size_t)s.W * (size_t)c->n_t;
    if (int rc = c->d_agg_part.grow(c, need)) return rc;
    if (int rc = c->d_agg_coef.grow(c, (size_t)c->L)) return rc;
    if (int rc = c->d_agg_group.grow(c, (size_t)c->L)) return rc;
    if (int rc = agg_upload(c, family, leaf_coef, leaf_group, c->d_agg_coef.p, c->d_agg_group.p)) return rc;
    AggArgs a = agg_args(c, s, c->d_agg_coef.p, c->d_agg_group.p);
    a.out = c->d_agg_part.p;
    agg_partial_kernel<<<agg_grid(c), 256, 0, c->stream>>>(a);
    HIPCHK(c, hipGetLastError());
    if (partial_out) HIPCHK(c, hipMemcpyAsync(partial_out, c->d_agg_part.p, need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));   // leaf_coef / leaf_group are the caller's
    c->agg = s;
    c->invalidate(P_PARTIAL);
    c->mark(P_PARTIAL);
    return 0;
}

int dsmgp_aggregate_finish(dsmgp_ctx* c, const double* partial_in, int32_t plain, int32_t prior_kernel_id,
                           double* mu_out, double* var_out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_PARTIAL)) return fail(c, DSMGP_E_STATE, "aggregate_finish before aggregate_partial");
    if (int rc = agg_prior_check(c, c->agg.family, prior_kernel_id, "aggregate_finish")) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nt = (size_t)c->n_t;
    const size_t nblk = (nt + 255) / 256;
    if (int rc = c->d_agg_out.grow(c, 3 * nt + 3 * nblk + 8)) return rc;
    if (partial_in)   // sums over all ranks / contexts, added by the caller
        HIPCHK(c, hipMemcpyAsync(c->d_agg_part.p, partial_in, (size_t)c->agg.W * nt * sizeof(double), hipMemcpyHostToDevice, c->stream));
    agg_finish_kernel<<<agg_grid(c), 256, 0, c->stream>>>(c->d_agg_part.p, c->n_t, c->agg.family, c->agg.G, plain ? 1 : 0, c->d_kp.p,
                                                        c->agg.family == AGG_RBCM ? prior_kernel_id : 0, c->dXt.p, c->D,
                                                        c->d_agg_out.p, c->d_agg_out.p + nt);
    HIPCHK(c, hipGetLastError());
    if (mu_out) HIPCHK(c, hipMemcpyAsync(mu_out, c->d_agg_out.p, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (var_out) HIPCHK(c, hipMemcpyAsync(var_out, c->d_agg_out.p + nt, nt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->invalidate(P_DONE);      // what was made from the moments of another total (the gradient sums) falls
    c->mark(P_DONE);
    return 0;
}

int dsmgp_aggregate(dsmgp_ctx* c, int32_t family, const double* leaf_coef, const int32_t* leaf_group, int32_t n_groups,
                    int32_t plain, int32_t prior_kernel_id, double* mu_out, double* var_out) {
    if (int rc = dsmgp_aggregate_partial(c, family, leaf_coef, leaf_group, n_groups, nullptr)) return rc;
    return dsmgp_aggregate_finish(c, nullptr, plain, prior_kernel_id, mu_out, var_out);
}

int dsmgp_aggregate_gradients_partial(dsmgp_ctx* c, double* partial_out, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_DONE)) return fail(c, DSMGP_E_STATE, "aggregate_gradients before aggregate on the current prediction");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t need = (size_t)agg_width(c->agg.family, c->agg.G, c->D) * (size_t)c->n_t;
    c->invalidate(P_GSUMS);
    if (int rc = c->d_agg_gpart.grow(c, need)) return rc;
    double sec = 0.0;
    if (int rc = agg_ensure(c, P_PGRAD, true, sec, [&](double* s) { return predict_gradients_device(c, true, s); })) return rc;
    AggArgs a = agg_args(c, c->agg, c->d_agg_coef.p, c->d_agg_group.p);
    a.dmu = c->d_pgout.p;
    a.dvar = c->d_pgout.p + (size_t)c->route_total * (size_t)c->D;
    a.agg_mu = c->d_agg_out.p;
    a.out = c->d_agg_gpart.p;
    EventPair ev;
    HIPCHK(c, ev.timed(c->stream, [&] { agg_grad_partial_kernel<<<agg_grid(c, c->D), 256, 0, c->stream>>>(a); }));
    if (partial_out) HIPCHK(c, hipMemcpyAsync(partial_out, c->d_agg_gpart.p, need * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, ev.add_seconds(sec));
    if (seconds) *seconds = sec;
    c->mark(P_GSUMS);
    return 0;
}

int dsmgp_aggregate_gradients_finish(dsmgp_ctx* c, const double* partial_in, int32_t plain, int32_t prior_kernel_id,
                                     double* dmu_out, double* dvar_out, int64_t ld) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_GSUMS)) return fail(c, DSMGP_E_STATE, "aggregate_gradients_finish before aggregate_gradients_partial");
    if (int rc = agg_prior_check(c, c->agg.family, prior_kernel_id, "aggregate_gradients_finish")) return rc;
    if (ld < c->n_t) return fail(c, DSMGP_E_ARG, "aggregate_gradients_finish: ld < n_t");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nt = (size_t)c->n_t;
    const int D = c->D;
    if (int rc = c->d_agg_gout.grow(c, 2 * nt * (size_t)D)) return rc;
    if (partial_in)     // sums over all contexts, added by the caller
        HIPCHK(c, hipMemcpyAsync(c->d_agg_gpart.p, partial_in, (size_t)agg_width(c->agg.family, c->agg.G, D) * nt * sizeof(double),
                                 hipMemcpyHostToDevice, c->stream));
    double* gm = c->d_agg_gout.p;
    double* gv = gm + nt * (size_t)D;
    agg_grad_finish_kernel<<<agg_grid(c, D), 256, 0, c->stream>>>(c->d_agg_gpart.p, c->d_agg_part.p, c->n_t, D, c->agg.family, c->agg.G,
                                                                plain ? 1 : 0, c->d_kp.p,
                                                                c->agg.family == AGG_RBCM ? prior_kernel_id : 0, c->dXt.p, gm, gv);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, agg_download(c, dmu_out, ld, gm, (size_t)D));
    HIPCHK(c, agg_download(c, dvar_out, ld, gv, (size_t)D));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int dsmgp_aggregate_gradients(dsmgp_ctx* c, int32_t plain, int32_t prior_kernel_id, double* dmu_out, double* dvar_out, int64_t ld,
                              double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (c->has(P_DONE) && ld < c->n_t) return fail(c, DSMGP_E_ARG, "aggregate_gradients: ld < n_t");    // before any device work
    if (int rc = dsmgp_aggregate_gradients_partial(c, nullptr, seconds)) return rc;
    return dsmgp_aggregate_gradients_finish(c, nullptr, plain, prior_kernel_id, dmu_out, dvar_out, ld);
}

int dsmgp_aggregate_columns(dsmgp_ctx* c, int32_t family, const double* leaf_coef, const int32_t* leaf_group, int32_t n_groups,
                            int32_t plain, int32_t prior_kernel_id, double* mu_out, double* var_out, int64_t ld, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "aggregate_columns before solve_targets on the current fit");
    if (!c->has(P_PRED)) return fail(c, DSMGP_E_STATE, "aggregate_columns before predict_run on the current fit");
    if (int rc = agg_family_check(c, family, leaf_coef, leaf_group, n_groups, "aggregate_columns")) return rc;
    if (int rc = agg_prior_check(c, family, prior_kernel_id, "aggregate_columns")) return rc;
    if (ld < c->n_t) return fail(c, DSMGP_E_ARG, "aggregate_columns: ld < n_t");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t nt = (size_t)c->n_t, L = (size_t)c->L;
    const int Q = c->tg_Q;
    c->invalidate(P_CDONE);
    if (int rc = c->d_col_coef.grow(c, L)) return rc;
    if (int rc = c->d_col_group.grow(c, L)) return rc;
    if (int rc = c->d_col_out.grow(c, 2 * nt * (size_t)Q)) return rc;
    double sec = 0.0;
    if (int rc = agg_ensure(c, P_TMU, true, sec, [&](double* s) { return predict_targets_device(c, s); })) return rc;
    if (int rc = agg_upload(c, family, leaf_coef, leaf_group, c->d_col_coef.p, c->d_col_group.p)) return rc;
    c->col = agg_state(family, n_groups);
    AggArgs a = agg_args(c, c->col, c->d_col_coef.p, c->d_col_group.p, plain, prior_kernel_id);
    a.mu = c->d_tmu.p;
    a.out = c->d_col_out.p;
    a.out_v = c->d_col_out.p + nt * (size_t)Q;
    EventPair ev;
    HIPCHK(c, ev.timed(c->stream, [&] { agg_columns_kernel<<<agg_grid(c, Q), 256, 0, c->stream>>>(a); }));
    HIPCHK(c, agg_download(c, mu_out, ld, a.out, (size_t)Q));
    HIPCHK(c, agg_download(c, var_out, ld, a.out_v, (size_t)Q));
    HIPCHK(c, hipStreamSynchronize(c->stream));     // leaf_coef / leaf_group are the caller's
    HIPCHK(c, ev.add_seconds(sec));
    if (seconds) *seconds = sec;
    c->mark(P_CDONE);
    return 0;
}

int dsmgp_aggregate_columns_gradients(dsmgp_ctx* c, int32_t plain, int32_t prior_kernel_id, double* dmu_out, double* dvar_out,
                                      int64_t ld, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_CDONE)) return fail(c, DSMGP_E_STATE, "aggregate_columns_gradients before aggregate_columns on the current prediction and columns");
    if (int rc = agg_prior_check(c, c->col.family, prior_kernel_id, "aggregate_columns_gradients")) return rc;
    if (ld < c->n_t) return fail(c, DSMGP_E_ARG, "aggregate_columns_gradients: ld < n_t");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t cols = (size_t)c->D * (size_t)c->tg_Q;
    if (int rc = c->d_col_gout.grow(c, 2 * (size_t)c->n_t * cols)) return rc;
    double sec = 0.0;
    if (int rc = agg_ensure(c, P_TIG, false, sec, [&](double* s) { return predict_columns_gradients_device(c, s); })) return rc;
    if (int rc = agg_ensure(c, P_PGRAD, false, sec, [&](double* s) { return predict_gradients_device(c, true, s); })) return rc;
    AggArgs a = agg_args(c, c->col, c->d_col_coef.p, c->d_col_group.p, plain, prior_kernel_id);
    a.mu = c->d_tmu.p;
    a.dmu = c->d_tigout.p;
    a.dvar = c->d_pgout.p + (size_t)c->route_total * (size_t)c->D;
    a.out = c->d_col_gout.p;
    a.out_v = c->d_col_gout.p + (size_t)c->n_t * cols;
    EventPair ev;
    HIPCHK(c, ev.timed(c->stream, [&] { agg_columns_grad_kernel<<<agg_grid(c, c->tg_Q), 256, 0, c->stream>>>(a); }));
    HIPCHK(c, agg_download(c, dmu_out, ld, a.out, cols));
    HIPCHK(c, agg_download(c, dvar_out, ld, a.out_v, cols));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, ev.add_seconds(sec));
    if (seconds) *seconds = sec;
    return 0;
}

// Hyper-parameter gradients of sum_q w_lq mll_lq over the resident target columns (kernels_targets.hpp at targets_a_kernel):
// one inversion -- or none, when the arena holds L^-T of this fit (dsmgp_loo's rule) -- and one contraction per leaf whatever Q is,
// plus O(n^2 Q) for A = L^-T Z and the rank-Q term.  Every leaf has tasks of its own (a COPY leaf reads its source's L^-T with its
// own A); the lists are rebuilt per call and live in buffers of this entry point, as do A, the weights and the partial sums:
// nothing another entry point reads is written, and the mask of dsmgp_set_gradient_leaves neither applies nor changes.
int dsmgp_mll_columns_gradients(dsmgp_ctx* c, double* grad_out, int32_t stride, const double* col_weight, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "targets_gradients before solve_targets on the current fit");
    if (!grad_out) return fail(c, DSMGP_E_ARG, "targets_gradients: grad_out is NULL");
    const int L = c->L, Q = c->tg_Q, qpad = c->tg_qpad, D = c->D;
    if (int rc = check_stride(c, "targets_gradients", stride)) return rc;
    bool any_ard = false, any_prod = false;
    for (int l = 0; l < L; ++l) {
        const int kind_l = c->hyper[c->leaves[l].kid].kind;
        any_ard = any_ard || (kind_l == DSMGP_KIND_ARD_SE && c->ard_true_gradient);
        any_prod = any_prod || KINDS[kind_l].dot_pass != 0;
    }
    if (any_ard && D > GRADDOT_STAGE_D)
        return fail(c, DSMGP_E_ARG, "ArdSE length-scale gradients need D <= " + std::to_string(GRADDOT_STAGE_D));
    std::vector<double> W, sw;
    if (int rc = column_weights(c, "targets_gradients", col_weight, false, W, sw)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // L^-T of every factor owner (xinv_lists / xinv_fill); lists of the call's own are dropped again on every way out
    OwnGradLists own_lists{c};
    if (int rc = xinv_lists(c, own_lists)) return rc;
    if (int rc = targets_slab(c, c->arenaA, "targets_gradients: no room for A = L^-T Z")) return rc;
    const int gs = any_rq(c) ? 3 + D : (any_ard || any_prod) ? 2 + D : 2;
    auto Xt = [&](int l) { return c->arenaX.p + c->gxoff[(size_t)c->leaves[l].owner]; };
    auto Al = [&](int l) { return c->arenaA.p + c->toff[(size_t)l] / 2; };
    std::vector<TargetsATask> ta;
    targets_a_tasks(c, ta);
    std::vector<FrobTask> frob;
    std::vector<int> frob_leaf;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (lf.owner != l) continue;
        for (int i = 0; i < lf.nb; ++i) {
            FrobTask f{};
            f.X = Xt(l) + (size_t)i * TB;
            f.ld = lf.npad;
            f.col0 = i * TB;
            f.col1 = lf.npad;
            f.nrows = std::max(0, std::min(TB, lf.n - i * TB));
            f.n = lf.n;
            frob.push_back(f);
            frob_leaf.push_back(l);
        }
    }
    // contraction tiles (build_dot_list), as dsmgp_gradients lists them but for every leaf; the columns add qpad to a task's cost
    DotRanges ranges;
    std::vector<GradTaskTg> gd = build_dot_list<GradTaskTg>(
        c, ranges, 64.0 + qpad, [&](int, int kind) { return kind != DSMGP_KIND_ARD_SE || c->ard_true_gradient; },
        [&](int l) { return DotOperand{Xt(l), c->leaves[c->leaves[l].owner].npad, true, c->h_leaves[l].alpha}; },
        [&](GradTaskTg& g, int l, int i, int j) {
            g.Aa = Al(l) + (size_t)i * TB;
            g.Ab = Al(l) + (size_t)j * TB;
            g.wq = c->d_tgw.p;      // + l once the buffer is there (below)
            g.sw = sw[(size_t)l];
            g.lda_t = c->leaves[l].npad;
            g.ldw = L;
            g.Q = Q;
            g.qpad = qpad;
        });
    const std::vector<int>& gd_leaf = ranges.leaf_of;
    // ArdLinear leaves: |L^-1 x_d|^2 by ardlin_quad_kernel (its alpha sums are not used: any vector of the leaf serves), and the
    // weighted squares of a_q . x_d
    std::vector<ArdLinTask> quad;
    std::vector<int> quad_leaf;
    std::vector<TargetsArdLinTask> al;
    std::vector<int> al_leaf;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (c->hyper[lf.kid].kind != DSMGP_KIND_ARD_LINEAR) continue;
        const LeafDev& d = c->h_leaves[l];
        ardlin_tasks(quad, quad_leaf, l, lf, Xt(l), c->leaves[lf.owner].npad, d.Xg, d.Xg);
        TargetsArdLinTask t{};
        t.A = Al(l);
        t.x = d.Xg;
        t.wq = nullptr;
        t.ld = lf.npad;
        t.ldw = L;
        t.n = lf.n;
        t.Q = Q;
        al.push_back(t);
        al_leaf.push_back(l);
    }
    if (int rc = c->d_tgw.grow(c, W.size())) return rc;
    for (size_t i = 0; i < gd.size(); ++i) gd[i].wq = c->d_tgw.p + gd_leaf[i];
    for (size_t i = 0; i < al.size(); ++i) al[i].wq = c->d_tgw.p + al_leaf[i];
    HIPCHK(c, hipMemcpy(c->d_tgw.p, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice));
    if (int rc = dev_upload(c, c->tga, ta)) return rc;
    if (int rc = dev_upload(c, c->tgfrob, frob)) return rc;
    if (int rc = dev_upload(c, c->tgdot, gd)) return rc;
    if (int rc = dev_upload(c, c->tgquad, quad)) return rc;
    if (int rc = dev_upload(c, c->tgardlin, al)) return rc;
    const size_t npart = frob.size() + (size_t)gs * gd.size() + 2 * (size_t)L + 2 * (size_t)D * quad.size() + (size_t)D * al.size();
    if (int rc = c->d_tgpart.grow(c, std::max<size_t>(1, npart))) return rc;
    double* pfrob = c->d_tgpart.p;
    double* pdot = pfrob + frob.size();
    double* pleaf = pdot + (size_t)gs * gd.size();
    double* pquad = pleaf + 2 * (size_t)L;
    double* pal = pquad + 2 * (size_t)D * quad.size();
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = xinv_fill(c)) return rc;
    if (!ta.empty()) targets_a_kernel<<<(unsigned)ta.size(), 256, 0, c->stream>>>(c->tga.p, qpad);
    launch_graddot<GD_TARGETS>(c, c->tgdot.p, ranges, pdot, gs);
    if (!frob.empty()) frob_kernel<<<(unsigned)frob.size(), 256, 0, c->stream>>>(c->tgfrob.p, pfrob);
    targets_wsums_kernel<<<L, 256, 0, c->stream>>>(c->d_leaves.p, c->arenaT.p, c->d_toff.p, c->arenaA.p, c->d_tgw.p, L, Q, qpad, pleaf);
    if (!quad.empty())
        ardlin_quad_kernel<false><<<dim3((unsigned)quad.size(), (unsigned)((D + ARDLIN_DC - 1) / ARDLIN_DC)), 256, 0, c->stream>>>(
            c->tgquad.p, D, pquad);
    if (!al.empty()) targets_ardlin_kernel<<<dim3((unsigned)al.size(), (unsigned)D), 256, 0, c->stream>>>(c->tgardlin.p, D, pal);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_XINV);
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    std::vector<double> part(std::max<size_t>(1, npart));
    HIPCHK(c, hipMemcpy(part.data(), c->d_tgpart.p, npart * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> info((size_t)L);
    HIPCHK(c, hipMemcpy(info.data(), c->d_info.p, (size_t)L * sizeof(int), hipMemcpyDeviceToHost));
    // host assembly, every sum in list order
    std::vector<double> trG((size_t)L, 0.0), Sl((size_t)L * D, 0.0);
    for (size_t i = 0; i < frob.size(); ++i) trG[(size_t)frob_leaf[i]] += part[i];
    for (int l = 0; l < L; ++l)
        if (c->leaves[l].owner != l) trG[(size_t)l] = trG[(size_t)c->leaves[l].owner];
    const double* pd = part.data() + frob.size();
    const DotSums sums = reduce_dot_sums(c, ranges, pd, (size_t)gs, false);
    const double* pl = pd + (size_t)gs * gd.size();
    const double* pq = pl + 2 * (size_t)L;
    const double* pa = pq + 2 * (size_t)D * quad.size();
    {
        std::vector<double> Qf((size_t)L * D, 0.0);
        for (size_t i = 0; i < quad.size(); ++i)
            for (int d = 0; d < D; ++d) Qf[(size_t)quad_leaf[i] * D + d] += pq[2 * (size_t)D * i + D + d];
        for (size_t i = 0; i < al.size(); ++i) {
            const size_t l = (size_t)al_leaf[i];
            for (int d = 0; d < D; ++d) Sl[l * D + d] = pa[i * D + d] - sw[l] * Qf[l * D + d];
        }
    }
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        double* g = grad_out + (size_t)l * stride;
        for (int j = 0; j < stride; ++j) g[j] = 0.0;
        if (info[(size_t)lf.owner] != 0) {
            for (int j = 0; j < stride; ++j) g[j] = qnan;
            continue;
        }
        GradSums q{};
        q.S1 = sums.S1[(size_t)l];
        q.Sd = gs > 2 ? sums.Sd.data() + (size_t)l * D : nullptr;
        q.Sa = sums.Sa[(size_t)l];
        q.Sl = Sl.data() + (size_t)l * D;
        q.trK = sw[(size_t)l] * trG[(size_t)l];
        q.ya = pl[2 * l];
        q.aa = pl[2 * l + 1];
        q.ns = (double)lf.n * sw[(size_t)l];
        assemble_gradient(c, c->hyper[lf.kid], q, g);
    }
    return 0;
}

// Hyper-parameter gradients of the LOO log predictive density (GPML eq. 5.13; the kernels and the formulas: kernels.hpp at
// loo_weights_kernel).  dsmgp_loo itself runs first -- L^-T of every owner, the row sums, lpd -- so lpd_out is its lpd_out to
// the bit and everything that call promises about dsmgp_gradients and the mask holds here too; then the passes of this call's
// own lists over an arena of their own.  Nothing the gradient pass or dsmgp_loo reads is written.
namespace {
int build_loo_grad_plan(dsmgp_ctx* c) {
    const int L = c->L;
    const int D = c->D;
    std::vector<size_t> hoff(L, 0), voff(L, 0);
    size_t hTot = 0, vTot = 0;
    bool any_ardse = false;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        any_ardse = any_ardse || c->hyper[lf.kid].kind == DSMGP_KIND_ARD_SE;
        if (c->grad_src[l] >= 0) continue;
        hoff[l] = hTot;
        voff[l] = vTot;
        hTot += (size_t)lf.npad * lf.npad;
        vTot += 4 * (size_t)lf.npad;
    }
    if (any_ardse && D > GRADDOT_STAGE_D)
        return fail(c, DSMGP_E_ARG, "loo_gradients: ArdSE length-scale gradients need D <= " + std::to_string(GRADDOT_STAGE_D));
    if (!c->arenaH.p) {
        size_t freeB = 0, totalB = 0;
        HIPCHK(c, hipMemGetInfo(&freeB, &totalB));
        if (!c->pool.active() && hTot * sizeof(double) + (size_t(2) << 30) > freeB)
            return fail(c, DSMGP_E_NOMEM, "loo_gradients need " + std::to_string((hTot * 8) >> 20) + " MiB for K_y^-1, device has " +
                                              std::to_string(freeB >> 20) + " MiB free");
        if (int rc = arena_status(c, c->arenaH.get(arena_pool(c), hTot))) return rc;
    }
    if (int rc = c->d_lgvec.alloc(c, vTot)) return rc;
    auto H = [&](int l) { return c->arenaH.p + hoff[l]; };
    auto V = [&](int l) { return c->d_lgvec.p + voff[l]; };
    auto Xt = [&](int l) { return c->arenaX.p + c->gxoff[c->leaves[l].owner]; };

    std::vector<LooVecTask> vt((size_t)L);
    std::vector<LooHvecTask> hv;
    c->lghvec_leaf.clear();
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        vt[l].npad = lf.npad;
        vt[l].vec = c->grad_src[l] >= 0 ? nullptr : V(l);
        if (c->grad_src[l] >= 0) continue;
        for (int t = 0; t * TB < lf.n; ++t) {
            LooHvecTask h{};
            h.H = H(l);
            h.vec = V(l);
            h.ld = lf.npad;
            h.n = lf.n;
            h.row0 = t * TB;
            h.nrows = std::min(TB, lf.n - t * TB);
            hv.push_back(h);
            c->lghvec_leaf.push_back(l);
        }
    }
    // tiles of H (build_ginv_list), then of the contraction (build_dot_list): ArdSE leaves always have tasks here
    auto computes = [&](int l) { return c->grad_src[l] < 0; };
    const std::vector<GinvTask> gi = build_ginv_list(c, computes, [&](int l) {
        return GinvPlace{Xt(l), c->leaves[l].npad, H(l), V(l) + 2 * (size_t)c->leaves[l].npad};
    });
    const std::vector<GradTask> gd = build_dot_list<GradTask>(
        c, c->lgdot_ranges, 64.0, [&](int l, int) { return computes(l); },
        [&](int l) { return DotOperand{H(l), c->leaves[l].npad, false, V(l)}; },
        [&](GradTask& g, int l, int, int) { g.uoff = c->leaves[l].npad; });
    std::vector<ArdLinTask> al;
    c->lgardlin_leaf.clear();
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (c->hyper[lf.kid].kind != DSMGP_KIND_ARD_LINEAR || !computes(l)) continue;
        ardlin_tasks(al, c->lgardlin_leaf, l, lf, H(l), lf.npad, c->h_leaves[l].Xg, V(l));
    }
    if (int rc = dev_upload(c, c->lgvec, vt)) return rc;
    if (int rc = dev_upload(c, c->lghvec, hv)) return rc;
    if (int rc = dev_upload(c, c->lginv, gi)) return rc;
    if (int rc = dev_upload(c, c->lgdot, gd)) return rc;
    if (int rc = dev_upload(c, c->lgardlin, al)) return rc;
    c->lgstride = 2 + D + (any_rq(c) ? 1 : 0);      // one more slot behind the dimensions: the sum for dK / dlog alpha
    if (int rc = c->d_lgpart.grow(c, 2 * (size_t)L + 2 * hv.size() + (size_t)c->lgstride * gd.size() + 3 * (size_t)D * al.size())) return rc;
    c->mark(P_LG_LISTS);
    return 0;
}

// The per-kind assembly of one leaf's row from the sums of the LOO passes (dsmgp_loo_gradients, dsmgp_loo_columns_gradients):
// every slot the true derivative sum_rc M_rc (dK_y / dtheta)_rc.  S1 / SK / Sd / Sa: M contracted with K r^2, K, dK / dlog l_d and
// dK / dlog alpha; xMx the ArdLinear forms x_d^T M x_d; trM and trMKy = tr(M K_y) from their identities.
struct LooSums {
    double S1, SK, Sa, trM, trMKy;
    const double* Sd;       // D sums
    const double* xMx;      // D forms, or null when the leaf is not ArdLinear
};
static void assemble_loo_gradient(const dsmgp_ctx* c, const HyperHost& h, const LooSums& q, double* g) {
    const int D = c->D;
    const int nl = n_lengthscales(h.kind, h.loghyp.size());
    const int ns = nl + KINDS[h.kind].n_shape;                // the slot of logs; logNoise behind it
    const double noise = std::exp(2.0 * h.loghyp[ns + 1]);
    const double cc = noise + 1e-8;
    if (h.kind == DSMGP_KIND_ISO_SE) {
        g[0] = q.S1 / std::exp(2.0 * h.loghyp[0]);            // dK / dlog l = K r^2 / l^2
        g[1] = 2.0 * q.SK;                                    // dK / dlog sigma = 2 K, contracted directly
    } else if (h.kind == DSMGP_KIND_ISO_LINEAR) {
        g[0] = -2.0 * (q.trMKy - cc * q.trM);                 // dK / dlog l = -2 K; sum M K = tr(M K_y) - c tr M
        g[1] = 0.0;
    } else if (h.kind == DSMGP_KIND_ARD_LINEAR) {
        for (int d = 0; d < nl; ++d) g[d] = -2.0 * q.xMx[d] / std::exp(2.0 * h.loghyp[d]);
        g[nl] = 0.0;
    } else {                                                  // ArdSE, ArdSEProduct, Matern, rational quadratic: per-dimension sums
        if (KINDS[h.kind].iso_matern) {
            double sl = 0.0;
            for (int d = 0; d < D; ++d) sl += q.Sd[d];
            g[0] = sl;
        } else {
            for (int d = 0; d < nl; ++d) g[d] = q.Sd[d];
        }
        if (KINDS[h.kind].rq) g[nl] = q.Sa;                   // sum M dK / dlog alpha
        g[ns] = 2.0 * q.SK;
    }
    g[ns + 1] = 2.0 * noise * q.trM;
}
}  // namespace

int dsmgp_loo_gradients(dsmgp_ctx* c, double* grad_out, int32_t stride, double* lpd_out, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "loo_gradients before fit");
    if (!grad_out) return fail(c, DSMGP_E_ARG, "grad_out is NULL");
    const int L = c->L;
    const int D = c->D;
    if (int rc = check_stride(c, "loo_gradients", stride)) return rc;
    std::vector<double> lpd((size_t)L);
    double sec_loo = 0.0;
    if (int rc = dsmgp_loo(c, nullptr, nullptr, lpd.data(), &sec_loo)) return rc;
    if (!c->has(P_LG_LISTS))        // (built for the kernel kinds of now: a change of kind drops them, free_grad in dsmgp_set_hyper)
        if (int rc = build_loo_grad_plan(c)) return rc;
    const int gs = c->lgstride;
    double* pw = c->d_lgpart.p;
    double* ph = pw + 2 * (size_t)L;
    double* pdot = ph + 2 * c->lghvec.count;
    double* pal = pdot + (size_t)gs * c->lgdot.count;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    loo_weights_kernel<<<L, 256, 0, c->stream>>>(c->d_leaves.p, c->lleaf.p, c->lgvec.p, pw);
    if (c->lginv.count) tile_ginv_kernel<<<(unsigned)c->lginv.count, 256, 0, c->stream>>>(c->lginv.p);
    if (c->lghvec.count) loo_hvec_kernel<<<(unsigned)c->lghvec.count, 256, 0, c->stream>>>(c->lghvec.p, ph);
    launch_graddot<GD_LOO>(c, c->lgdot.p, c->lgdot_ranges, pdot, gs);
    if (c->lgardlin.count)
        ardlin_quad_kernel<true><<<dim3((unsigned)c->lgardlin.count, (unsigned)((D + ARDLIN_DC - 1) / ARDLIN_DC)), 256, 0, c->stream>>>(
            c->lgardlin.p, D, pal);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = sec_loo + ms * 1e-3;
    std::vector<double> part(c->d_lgpart.count);
    HIPCHK(c, hipMemcpy(part.data(), c->d_lgpart.p, part.size() * sizeof(double), hipMemcpyDeviceToHost));
    // host assembly: the task sums of a leaf are added in list order (fixed: bit-reproducible)
    const double* hw = part.data();
    const double* hh = hw + 2 * (size_t)L;
    const double* hd = hh + 2 * c->lghvec.count;
    const double* ha = hd + (size_t)gs * c->lgdot.count;
    std::vector<double> frob(L, 0.0), ua(L, 0.0);
    for (size_t i = 0; i < c->lghvec.count; ++i) {
        frob[c->lghvec_leaf[i]] += hh[2 * i];
        ua[c->lghvec_leaf[i]] += hh[2 * i + 1];
    }
    const DotSums sums = reduce_dot_sums(c, c->lgdot_ranges, hd, (size_t)gs, true);
    std::vector<double> A, U, Q;
    if (c->lgardlin.count) {
        A.assign((size_t)L * D, 0.0);
        U = A;
        Q = A;
        for (size_t i = 0; i < c->lgardlin.count; ++i) {
            const size_t l = (size_t)c->lgardlin_leaf[i];
            for (int d = 0; d < D; ++d) {
                A[l * D + d] += ha[3 * (size_t)D * i + d];
                Q[l * D + d] += ha[3 * (size_t)D * i + D + d];
                U[l * D + d] += ha[3 * (size_t)D * i + 2 * D + d];
            }
        }
    }
    std::vector<double> xMx((size_t)D, 0.0);
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const HyperHost& h = c->hyper[lf.kid];
        const size_t s = (size_t)(c->grad_src[l] >= 0 ? c->grad_src[l] : l);      // a COPY leaf with its source's mean: the source's
        double* g = grad_out + (size_t)l * stride;
        for (int j = 0; j < stride; ++j) g[j] = 0.0;
        if (std::isnan(lpd[l])) {       // the fit of this leaf failed (info != 0)
            for (size_t j = 0; j < h.loghyp.size(); ++j) g[j] = std::nan("");
            continue;
        }
        LooSums q{};
        q.S1 = sums.S1[s];
        q.SK = sums.SK[s];
        q.Sa = sums.Sa[s];
        q.Sd = sums.Sd.data() + s * D;
        q.trM = ua[s] - frob[s];                                  // tr M = u . alpha - |H|_F^2
        q.trMKy = hw[2 * s] - hw[2 * s + 1];                      // tr(M K_y) = sum alpha_i^2 / d_i - sum w_i d_i
        if (h.kind == DSMGP_KIND_ARD_LINEAR) {
            for (int d = 0; d < D; ++d)                           // x_d^T M x_d = (x_d . u)(x_d . alpha) - |H^T x_d|^2
                xMx[d] = U[s * D + d] * A[s * D + d] - Q[s * D + d];
            q.xMx = xMx.data();
        }
        assemble_loo_gradient(c, h, q, g);
    }
    if (lpd_out) std::memcpy(lpd_out, lpd.data(), (size_t)L * sizeof(double));
    return 0;
}

// Leave-one-out moments and gradients of the resident target columns (the kernels and the formulas: kernels_targets.hpp at
// LooColsTask).  d and L^-T come by dsmgp_loo's rule (xinv_lists / xinv_fill, the row sums by rownorm_kernel over that call's own
// lists), A by the kernel and the tasks of dsmgp_mll_columns_gradients.  Every leaf has tasks of its own: a COPY leaf reads its
// source's d and L^-T with its own A, mean and weights.  H, U, the vectors, the lists and the sums live in buffers of these two
// entry points: nothing another entry point reads is written, and the mask of dsmgp_set_gradient_leaves neither applies nor changes.
namespace {
// What both calls need before their own kernels: the lists of the inversion and of the row sums, A's arena and its tasks
static int loo_columns_prepare(dsmgp_ctx* c, OwnGradLists& own) {
    if (int rc = xinv_lists(c, own)) return rc;
    if (!c->has(P_LOO_LISTS))
        if (int rc = build_loo_plan(c)) return rc;
    if (int rc = targets_slab(c, c->arenaA, "loo_columns: no room for A = L^-T Z")) return rc;
    std::vector<TargetsATask> ta;
    targets_a_tasks(c, ta);
    return dev_upload(c, c->tga, ta);
}
// ... and queues: L^-T (when the arena does not hold this fit's), the row sums of diag K_y^-1, A
static int loo_columns_front(dsmgp_ctx* c) {
    if (int rc = ensure_dinv(c)) return rc;
    if (int rc = xinv_fill(c)) return rc;
    if (c->lrow.count) rownorm_kernel<<<(unsigned)c->lrow.count, 256, 0, c->stream>>>(c->lrow.p);
    if (c->tga.count) targets_a_kernel<<<(unsigned)c->tga.count, 256, 0, c->stream>>>(c->tga.p, c->tg_qpad);
    return 0;
}
}  // namespace

int dsmgp_loo_columns(dsmgp_ctx* c, double* mu_out, int64_t ld, double* var_out, double* lpd_out, double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "loo_columns before solve_targets on the current fit");
    const int L = c->L, Q = c->tg_Q;
    const size_t nobs = (size_t)c->obs_ptr[L];
    if (mu_out && ld < (int64_t)nobs) return fail(c, DSMGP_E_ARG, "loo_columns: ld < obs_ptr[L]");
    HIPCHK(c, hipSetDevice(c->device));
    OwnGradLists own_lists{c};
    if (int rc = loo_columns_prepare(c, own_lists)) return rc;
    std::vector<LooColsTask> lt((size_t)L);
    for (int l = 0; l < L; ++l) {
        lt[(size_t)l].A = c->arenaA.p + c->toff[(size_t)l] / 2;
        lt[(size_t)l].npad = c->leaves[l].npad;
        lt[(size_t)l].Q = Q;
    }
    if (int rc = dev_upload(c, c->lcleaf, lt)) return rc;
    if (int rc = c->d_lcout.grow(c, nobs * (size_t)Q + nobs + (size_t)L * Q)) return rc;
    double* dmu = c->d_lcout.p;
    double* dvar = dmu + nobs * (size_t)Q;
    double* dlpd = dvar + nobs;
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = loo_columns_front(c)) return rc;
    loo_columns_moments_kernel<<<dim3((unsigned)L, (unsigned)Q), 256, 0, c->stream>>>(
        c->d_leaves.p, c->lleaf.p, c->lcleaf.p, c->d_obs_idx.p, c->d_tY.p, c->N, L, dmu, (long long)nobs, dvar, dlpd);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_XINV);
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    if (mu_out && nobs)
        HIPCHK(c, hipMemcpy2D(mu_out, (size_t)ld * sizeof(double), dmu, nobs * sizeof(double), nobs * sizeof(double), (size_t)Q,
                              hipMemcpyDeviceToHost));
    if (var_out) HIPCHK(c, hipMemcpy(var_out, dvar, nobs * sizeof(double), hipMemcpyDeviceToHost));
    if (lpd_out) HIPCHK(c, hipMemcpy(lpd_out, dlpd, (size_t)L * Q * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int dsmgp_loo_columns_gradients(dsmgp_ctx* c, double* grad_out, int32_t stride, const double* col_weight, double* lpd_out,
                                double* seconds) {
    if (!c) return DSMGP_E_ARG;
    if (seconds) *seconds = 0.0;
    if (!c->has(P_Z)) return fail(c, DSMGP_E_STATE, "loo_columns_gradients before solve_targets on the current fit");
    if (!grad_out) return fail(c, DSMGP_E_ARG, "loo_columns_gradients: grad_out is NULL");
    const int L = c->L, Q = c->tg_Q, qpad = c->tg_qpad, D = c->D;
    if (int rc = check_stride(c, "loo_columns_gradients", stride)) return rc;
    bool any_ardse = false;
    for (int l = 0; l < L; ++l) any_ardse = any_ardse || c->hyper[c->leaves[l].kid].kind == DSMGP_KIND_ARD_SE;
    if (any_ardse && D > GRADDOT_STAGE_D)
        return fail(c, DSMGP_E_ARG, "loo_columns_gradients: ArdSE length-scale gradients need D <= " + std::to_string(GRADDOT_STAGE_D));
    std::vector<double> W, sw;
    if (int rc = column_weights(c, "loo_columns_gradients", col_weight, true, W, sw)) return rc;
    auto active = [&](int l) { return sw[(size_t)l] > 0.0; };      // a row of zero weights: a row of zeros and no tasks
    HIPCHK(c, hipSetDevice(c->device));
    OwnGradLists own_lists{c};
    if (int rc = loo_columns_prepare(c, own_lists)) return rc;
    if (int rc = targets_slab(c, c->arenaU, "loo_columns_gradients: no room for U = K_y^-1 (A / d)")) return rc;
    std::vector<size_t> hoff((size_t)L, 0), voff((size_t)L, 0);
    size_t hTot = 0, vTot = 0;
    for (int l = 0; l < L; ++l) {
        hoff[(size_t)l] = hTot;
        voff[(size_t)l] = vTot;
        hTot += (size_t)c->leaves[l].npad * c->leaves[l].npad;
        vTot += 3 * (size_t)c->leaves[l].npad;
    }
    if (int rc = arena_status(c, c->arenaHc.grow(arena_pool(c), hTot))) {
        (void)hipGetLastError();
        return rc == DSMGP_E_NOMEM ? rc : fail(c, DSMGP_E_NOMEM, "loo_columns_gradients: no room for K_y^-1 (" + std::to_string((hTot * 8) >> 20) + " MiB)");
    }
    if (int rc = c->d_lcvec.grow(c, std::max<size_t>(1, vTot))) return rc;
    if (int rc = c->d_lcw.grow(c, W.size())) return rc;
    auto H = [&](int l) { return c->arenaHc.p + hoff[(size_t)l]; };
    auto V = [&](int l) { return c->d_lcvec.p + voff[(size_t)l]; };
    auto Al = [&](int l) { return c->arenaA.p + c->toff[(size_t)l] / 2; };
    auto Ul = [&](int l) { return c->arenaU.p + c->toff[(size_t)l] / 2; };
    auto Xt = [&](int l) { return c->arenaX.p + c->gxoff[(size_t)c->leaves[l].owner]; };
    const double* wdev = c->d_lcw.p;

    std::vector<LooColsTask> lt((size_t)L);
    std::vector<LooColsUTask> ut;
    std::vector<LooColsRowTask> rt;
    std::vector<int> rt_leaf;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        LooColsTask& t = lt[(size_t)l];
        t.A = Al(l);
        t.vec = active(l) ? V(l) : nullptr;
        t.wq = wdev + l;
        t.s = sw[(size_t)l];
        t.npad = lf.npad;
        t.ldw = L;
        t.Q = Q;
        if (!active(l)) continue;
        for (int i = 0; i * TB < lf.n; ++i) {
            const int nrows = std::min(TB, lf.n - i * TB);
            LooColsUTask u{};
            u.H = H(l) + (size_t)i * TB;
            u.A = Al(l);
            u.tq = V(l) + 2 * (size_t)lf.npad;
            u.U = Ul(l) + (size_t)i * TB;
            u.ld = lf.npad;
            u.n = lf.n;
            u.nrows = nrows;
            ut.push_back(u);
            LooColsRowTask r{};
            r.H = H(l);
            r.A = Al(l);
            r.U = Ul(l);
            r.wq = wdev + l;
            r.ld = lf.npad;
            r.ldw = L;
            r.n = lf.n;
            r.Q = Q;
            r.row0 = i * TB;
            r.nrows = nrows;
            rt.push_back(r);
            rt_leaf.push_back(l);
        }
    }
    // tiles of H (build_ginv_list), then of the contraction (build_dot_list), as dsmgp_loo_gradients lists them but for every
    // leaf with weight
    const std::vector<GinvTask> gi = build_ginv_list(c, active, [&](int l) {
        return GinvPlace{Xt(l), c->leaves[c->leaves[l].owner].npad, H(l), V(l) + (size_t)c->leaves[l].npad};
    });
    DotRanges ranges;
    const std::vector<GradTaskLc> gd = build_dot_list<GradTaskLc>(
        c, ranges, 64.0, [&](int l, int) { return active(l); },
        // (the vector block is staged by the epilogues, never in a weight: any vector of the leaf serves)
        [&](int l) { return DotOperand{H(l), c->leaves[l].npad, false, V(l)}; },
        [&](GradTaskLc& g, int l, int i, int j) {
            g.Aa = Al(l) + (size_t)i * TB;
            g.Ab = Al(l) + (size_t)j * TB;
            g.Ua = Ul(l) + (size_t)i * TB;
            g.Ub = Ul(l) + (size_t)j * TB;
            g.wq = wdev + l;
            g.lda_t = c->leaves[l].npad;
            g.ldw = L;
            g.Q = Q;
            g.qpad = qpad;
        });
    // ArdLinear leaves: |H^T x_d|^2 by ardlin_quad_kernel<true> (its two vector sums are not used: any block of the leaf serves) and
    // the weighted products of x_d . u_q and x_d . a_q
    std::vector<ArdLinTask> quad;
    std::vector<int> quad_leaf;
    std::vector<LooColsArdLinTask> al;
    std::vector<int> al_leaf;
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        if (c->hyper[lf.kid].kind != DSMGP_KIND_ARD_LINEAR || !active(l)) continue;
        const LeafDev& d = c->h_leaves[l];
        ardlin_tasks(quad, quad_leaf, l, lf, H(l), lf.npad, d.Xg, V(l));
        LooColsArdLinTask t{};
        t.A = Al(l);
        t.U = Ul(l);
        t.x = d.Xg;
        t.wq = wdev + l;
        t.ld = lf.npad;
        t.ldw = L;
        t.n = lf.n;
        t.Q = Q;
        al.push_back(t);
        al_leaf.push_back(l);
    }
    HIPCHK(c, hipMemcpy(c->d_lcw.p, W.data(), W.size() * sizeof(double), hipMemcpyHostToDevice));
    if (int rc = dev_upload(c, c->lcleaf, lt)) return rc;
    if (int rc = dev_upload(c, c->lcginv, gi)) return rc;
    if (int rc = dev_upload(c, c->lcu, ut)) return rc;
    if (int rc = dev_upload(c, c->lcrow, rt)) return rc;
    if (int rc = dev_upload(c, c->lcdot, gd)) return rc;
    if (int rc = dev_upload(c, c->lcquad, quad)) return rc;
    if (int rc = dev_upload(c, c->lcardlin, al)) return rc;
    const int gs = 2 + D + (any_rq(c) ? 1 : 0);
    const size_t npart = 2 * (size_t)L + 2 * rt.size() + (size_t)gs * gd.size() + 3 * (size_t)D * quad.size() + (size_t)D * al.size();
    if (int rc = c->d_lcpart.grow(c, npart)) return rc;
    if (int rc = c->d_lcout.grow(c, (size_t)L * Q)) return rc;
    double* pw = c->d_lcpart.p;
    double* prow = pw + 2 * (size_t)L;
    double* pdot = prow + 2 * rt.size();
    double* pquad = pdot + (size_t)gs * gd.size();
    double* pal = pquad + 3 * (size_t)D * quad.size();
    EventPair ev;
    HIPCHK(c, ev.init());
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    if (int rc = loo_columns_front(c)) return rc;
    loo_columns_moments_kernel<<<dim3((unsigned)L, (unsigned)Q), 256, 0, c->stream>>>(
        c->d_leaves.p, c->lleaf.p, c->lcleaf.p, c->d_obs_idx.p, c->d_tY.p, c->N, L, nullptr, 0, nullptr, c->d_lcout.p);
    loo_columns_weights_kernel<<<L, 256, 0, c->stream>>>(c->d_leaves.p, c->lleaf.p, c->lcleaf.p, pw);
    if (!gi.empty()) tile_ginv_kernel<<<(unsigned)gi.size(), 256, 0, c->stream>>>(c->lcginv.p);
    if (!ut.empty()) loo_columns_u_kernel<<<(unsigned)ut.size(), 256, 0, c->stream>>>(c->lcu.p, qpad);
    if (!rt.empty()) loo_columns_rowsums_kernel<<<(unsigned)rt.size(), 256, 0, c->stream>>>(c->lcrow.p, prow);
    launch_graddot<GD_LOO_COLUMNS>(c, c->lcdot.p, ranges, pdot, gs);
    if (!quad.empty())
        ardlin_quad_kernel<true><<<dim3((unsigned)quad.size(), (unsigned)((D + ARDLIN_DC - 1) / ARDLIN_DC)), 256, 0, c->stream>>>(
            c->lcquad.p, D, pquad);
    if (!al.empty()) loo_columns_ardlin_kernel<<<dim3((unsigned)al.size(), (unsigned)D), 256, 0, c->stream>>>(c->lcardlin.p, D, pal);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_XINV);
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    if (seconds) *seconds = ms * 1e-3;
    std::vector<double> part(std::max<size_t>(1, npart));
    HIPCHK(c, hipMemcpy(part.data(), c->d_lcpart.p, npart * sizeof(double), hipMemcpyDeviceToHost));
    std::vector<int> info((size_t)L);
    HIPCHK(c, hipMemcpy(info.data(), c->d_info.p, (size_t)L * sizeof(int), hipMemcpyDeviceToHost));
    // host assembly: the task sums of a leaf are added in list order (fixed: bit-reproducible)
    const double* hw = part.data();
    const double* hr = hw + 2 * (size_t)L;
    const double* hd = hr + 2 * rt.size();
    const double* hq = hd + (size_t)gs * gd.size();
    const double* ha = hq + 3 * (size_t)D * quad.size();
    std::vector<double> frob((size_t)L, 0.0), ua((size_t)L, 0.0), xMx((size_t)L * D, 0.0);
    for (size_t i = 0; i < rt.size(); ++i) {
        frob[(size_t)rt_leaf[i]] += hr[2 * i];
        ua[(size_t)rt_leaf[i]] += hr[2 * i + 1];
    }
    const DotSums sums = reduce_dot_sums(c, ranges, hd, (size_t)gs, true);
    for (size_t i = 0; i < al.size(); ++i)
        for (int d = 0; d < D; ++d) xMx[(size_t)al_leaf[i] * D + d] = ha[i * D + d];
    for (size_t i = 0; i < quad.size(); ++i)                      // x_d^T M x_d = sum_q c_q (x_d . u_q)(x_d . a_q) - |H^T x_d|^2
        for (int d = 0; d < D; ++d) xMx[(size_t)quad_leaf[i] * D + d] -= hq[3 * (size_t)D * i + D + d];
    for (int l = 0; l < L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const HyperHost& h = c->hyper[lf.kid];
        double* g = grad_out + (size_t)l * stride;
        for (int j = 0; j < stride; ++j) g[j] = 0.0;
        if (info[(size_t)lf.owner] != 0) {
            for (size_t j = 0; j < h.loghyp.size(); ++j) g[j] = std::nan("");
            continue;
        }
        if (!active(l)) continue;
        LooSums q{};
        q.S1 = sums.S1[(size_t)l];
        q.SK = sums.SK[(size_t)l];
        q.Sa = sums.Sa[(size_t)l];
        q.Sd = sums.Sd.data() + (size_t)l * D;
        q.xMx = xMx.data() + (size_t)l * D;
        q.trM = ua[(size_t)l] - frob[(size_t)l];                  // tr M = sum_q c_q u_q . a_q - |H|_F^2
        q.trMKy = hw[2 * l] - hw[2 * l + 1];                      // tr(M K_y) = sum_q c_q sum_i a_iq^2 / d_i - sum_i W_i d_i
        assemble_loo_gradient(c, h, q, g);
    }
    if (lpd_out) HIPCHK(c, hipMemcpy(lpd_out, c->d_lcout.p, (size_t)L * Q * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

// -------------------------------------------------------------------------------------------------
int dsmgp_kernel_matrix(dsmgp_ctx* c, int32_t kernel_id, const double* x1, int64_t n1, const double* x2,
                        int64_t n2, double* K_out) {
    if (!c) return DSMGP_E_ARG;
    if (!x1 || !x2 || !K_out || n1 <= 0 || n2 <= 0 || c->D <= 0) return fail(c, DSMGP_E_ARG, "kernel_matrix: bad arguments");
    if (kernel_id < 0 || kernel_id >= (int)c->hyper.size() || c->hyper[kernel_id].kind < 0)
        return fail(c, DSMGP_E_STATE, "kernel_matrix: kernel id without hyper-parameters");
    if (ard_linear_short(c, kernel_id))
        return fail(c, DSMGP_E_ARG, std::string("kernel_matrix: ") + KINDS[c->hyper[kernel_id].kind].name +
                                        " needs one lengthscale per input dimension");
    HIPCHK(c, hipSetDevice(c->device));
    if (int rc = upload_hyper(c)) return rc;
    const int D = c->D;
    const int p1 = round_up((int)n1, TB), p2 = round_up((int)n2, TB);
    DevBuf<double> dx1, dx2, dK;
    if (int rc = dx1.alloc(c, (size_t)n1 * D)) return rc;
    if (int rc = dx2.alloc(c, (size_t)n2 * D)) return rc;
    if (int rc = dK.alloc(c, (size_t)p1 * p2)) return rc;
    HIPCHK(c, hipMemcpy(dx1.p, x1, (size_t)n1 * D * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(dx2.p, x2, (size_t)n2 * D * sizeof(double), hipMemcpyHostToDevice));
    std::vector<GramTask> g;
    for (int j = 0; j < p2 / TB; ++j)
        for (int i = 0; i < p1 / TB; ++i) {
            GramTask t{};
            t.xa = dx1.p + (size_t)i * TB;
            t.xb = dx2.p + (size_t)j * TB;
            t.out = dK.p + (size_t)i * TB + (size_t)j * TB * p1;
            t.lda = (int)n1;
            t.ldb = (int)n2;
            t.ldo = p1;
            t.na = (int)std::min<int64_t>(TB, n1 - (int64_t)i * TB);
            t.nb = (int)std::min<int64_t>(TB, n2 - (int64_t)j * TB);
            t.kid = kernel_id;
            g.push_back(t);
        }
    DevBuf<GramTask> dg;
    if (int rc = dev_upload(c, dg, g)) return rc;
    gram_tile_kernel<<<2 * (int)g.size(), 256, 0, c->stream>>>(dg.p, c->d_kp.p, D);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy2D(K_out, (size_t)n1 * sizeof(double), dK.p, (size_t)p1 * sizeof(double), (size_t)n1 * sizeof(double),
                          (size_t)n2, hipMemcpyDeviceToHost));
    return 0;
}

int dsmgp_download_factor(dsmgp_ctx* c, int32_t leaf, double* F, double* alpha) {
    if (!c) return DSMGP_E_ARG;
    if (!c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "download_factor before fit");
    if (leaf < 0 || leaf >= c->L) return fail(c, DSMGP_E_ARG, "leaf out of range");
    HIPCHK(c, hipSetDevice(c->device));
    const LeafHost& lf = c->leaves[leaf];
    const LeafDev& d = c->h_leaves[leaf];
    if (F) {
        HIPCHK(c, hipMemcpy2D(F, (size_t)lf.n * sizeof(double), d.F, (size_t)lf.npad * sizeof(double),
                              (size_t)lf.n * sizeof(double), (size_t)lf.n, hipMemcpyDeviceToHost));
        for (int col = 1; col < lf.n; ++col)
            for (int r = 0; r < col; ++r) F[r + (size_t)col * lf.n] = 0.0;
    }
    if (alpha) {
        if (int rc = ensure_alpha(c)) return rc;
        HIPCHK(c, hipMemcpy(alpha, d.alpha, lf.n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}

int dsmgp_timings(dsmgp_ctx* c, double* out) {
    if (!c || !out) return DSMGP_E_ARG;
    for (int i = 0; i < DSMGP_N_TIMINGS; ++i) out[i] = c->timings[i];
    return 0;
}

int dsmgp_work_gradients(dsmgp_ctx* c, double* alg_flops_inverse, double* alg_flops_contraction, int32_t* n_contraction_tiles) {
    if (!c) return DSMGP_E_ARG;
    // L^-T of every factor owner: n^3/3; contraction (alpha alpha^T - K_y^-1) o K o P of every IsoSE / ArdSEProduct / Matern leaf: the lower
    // tiles of L^-T L^-1, n^3/3 again (2 x 128 x 128 x K per tile with K = n - 128 i)
    double fi = 0.0, fc = 0.0;
    for (int l = 0; l < c->L; ++l) {
        const LeafHost& lf = c->leaves[l];
        const double n = (double)lf.n;
        if (lf.owner == l) fi += n * n * n / 3.0;
        if (lf.kid < (int)c->hyper.size() && c->hyper[lf.kid].kind >= 0 && KINDS[c->hyper[lf.kid].kind].contraction)
            fc += n * n * n / 3.0;
    }
    if (alg_flops_inverse) *alg_flops_inverse = fi;
    if (alg_flops_contraction) *alg_flops_contraction = fc;
    if (n_contraction_tiles) *n_contraction_tiles = (int32_t)c->gdot.count;
    return 0;
}

int dsmgp_work(dsmgp_ctx* c, double* alg_flops_update, int32_t* n_update_launches) {
    if (!c) return DSMGP_E_ARG;
    if (alg_flops_update) *alg_flops_update = c->last_fit_joint ? c->alg_flops_joint : c->alg_flops_update;
    if (n_update_launches) *n_update_launches = c->n_update_launches;
    return 0;
}

int dsmgp_lanes(dsmgp_ctx* c, int32_t* lanes) {
    if (!c || !lanes) return DSMGP_E_ARG;
    *lanes = c->has(P_PLAN) ? c->nlanes : 0;
    return 0;
}

int dsmgp_work_fused(dsmgp_ctx* c, double* alg_flops_fused, int32_t* n_fused_launches) {
    if (!c) return DSMGP_E_ARG;
    if (alg_flops_fused) *alg_flops_fused = c->last_fit_joint ? c->alg_flops_fused_joint : c->alg_flops_fused;
    if (n_fused_launches) *n_fused_launches = c->n_fused_launches;
    return 0;
}

// Free every device buffer that scales with the leaf sizes (factors, inverse blocks, K_tn rows, L^-1, task lists),
// keeping the training data, the leaf table, the sharing schedule and the hyper-parameters: the next fit rebuilds
// them.  This is the "discard" half of the factor-and-discard streaming mode (hipabi.StreamingContext).
int dsmgp_reserve(dsmgp_ctx* c, int64_t bytes) {
    if (!c || bytes < 0) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    free_plan_and_test(c);
    c->pool.release();
    if (bytes == 0) return 0;
    if (c->pool.reserve((size_t)bytes) != 0) {
        (void)hipGetLastError();
        return fail(c, DSMGP_E_NOMEM, "cannot reserve " + std::to_string(bytes >> 20) + " MiB of device memory");
    }
    return 0;
}

int dsmgp_release(dsmgp_ctx* c) {
    if (!c) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HostLog hl("release");
    free_plan_and_test(c);
    return 0;
}

// Device bytes a leaf table of these sizes needs resident (factor + inverse blocks + gathered inputs + vectors,
// K_tn rows for n_test routed rows per leaf, and L^-1 when gradients are wanted); no context state involved.
int64_t dsmgp_estimate_bytes(int32_t L, const int64_t* n, const int64_t* n_test, int32_t D, int32_t with_gradients) {
    int64_t tot = 0;
    for (int l = 0; l < L; ++l) {
        const int64_t np_ = (n[l] + TB - 1) / TB * TB;
        const int64_t nt_ = n_test ? (n_test[l] + TB - 1) / TB * TB : 0;
        tot += np_ * np_ * (with_gradients ? 2 : 1) + np_ * TB + np_ * (D + 4) + nt_ * np_ + nt_ * (D + 4);
    }
    return tot * (int64_t)sizeof(double);
}

int dsmgp_memory(dsmgp_ctx* c, int64_t* needed, int64_t* free_bytes) {
    if (!c) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    size_t f = 0, t = 0;
    HIPCHK(c, hipMemGetInfo(&f, &t));
    if (needed) *needed = (int64_t)c->bytes_needed;
    if (free_bytes) *free_bytes = (int64_t)f;
    return 0;
}

int dsmgp_probe_f64_mfma(dsmgp_ctx* c, double* tflops) {
    double d[4];
    if (!tflops) return DSMGP_E_ARG;
    if (int rc = dsmgp_probe_f64_mfma_detail(c, 8, d)) return rc;
    *tflops = d[0];
    return 0;
}

// out[0] = TFLOP/s over the chip, out[1] = shader cycles per MFMA issued by one wave (median wave),
// out[2] = shader clock in GHz held during the loop, out[3] = waves per SIMD used
int dsmgp_probe_f64_mfma_detail(dsmgp_ctx* c, int32_t blocks_per_cu, double* out) {
    if (!c || !out || blocks_per_cu < 1 || blocks_per_cu > 8) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int blocks = c->ncu * blocks_per_cu;
    const int iters = 6000 / blocks_per_cu;
    const int nwaves = blocks * 4;
    DevBuf<double> sink;
    DevBuf<unsigned long long> stamps;
    if (int rc = sink.alloc(c, (size_t)blocks * 256)) return rc;
    if (int rc = stamps.alloc(c, (size_t)nwaves * 2)) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    const hipEvent_t t0 = ev.a, t1 = ev.b;
    for (int rep = 0; rep < 3; ++rep) mfma_probe_kernel<<<blocks, 256, 0, c->stream>>>(sink.p, stamps.p, iters);
    HIPCHK(c, hipEventRecord(t0, c->stream));
    mfma_probe_kernel<<<blocks, 256, 0, c->stream>>>(sink.p, stamps.p, iters);
    HIPCHK(c, hipEventRecord(t1, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, t0, t1));
    std::vector<unsigned long long> hs((size_t)nwaves * 2);
    HIPCHK(c, hipMemcpy(hs.data(), stamps.p, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::vector<double> cyc(nwaves), clk(nwaves);
    for (int i = 0; i < nwaves; ++i) {
        cyc[i] = (double)hs[2 * i] / ((double)iters * 16.0);
        clk[i] = hs[2 * i + 1] ? (double)hs[2 * i] / ((double)hs[2 * i + 1] * 10.0) : 0.0;   // cycles per ns
    }
    std::sort(cyc.begin(), cyc.end());
    std::sort(clk.begin(), clk.end());
    const double flops = (double)blocks * 4.0 * (double)iters * 16.0 * 2048.0;
    out[0] = flops / (ms * 1e-3) / 1e12;
    out[1] = cyc[nwaves / 2];
    out[2] = clk[nwaves / 2];   // cycles per 10 ns tick / 10 = GHz
    out[3] = blocks_per_cu;
    return 0;
}

// Shader clock held under load: a one-wave kernel on a stream of its own that sleeps for `milliseconds` of wall time beside
// whatever the context launches meanwhile and reports shader cycles per wall tick.  start returns at once; read waits for it.
int dsmgp_clock_sample_start(dsmgp_ctx* c, double milliseconds) {
    if (!c) return DSMGP_E_ARG;
    if (!(milliseconds > 0.0) || milliseconds > 5000.0) return fail(c, DSMGP_E_ARG, "clock_sample_start: 0 < milliseconds <= 5000");
    if (c->clock_pending) return fail(c, DSMGP_E_STATE, "clock_sample_start: a sample is already running (read it first)");
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->side) HIPCHK(c, hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    if (int rc = c->d_clock.alloc(c, 2)) return rc;
    clock_sample_kernel<<<1, 64, 0, c->side>>>(c->d_clock.p, (unsigned long long)(milliseconds * 1e5));   // 100 MHz ticks
    HIPCHK(c, hipGetLastError());
    c->clock_pending = true;
    return 0;
}

int dsmgp_clock_sample_read(dsmgp_ctx* c, double* ghz, double* milliseconds) {
    if (!c) return DSMGP_E_ARG;
    if (!c->clock_pending) return fail(c, DSMGP_E_STATE, "clock_sample_read before clock_sample_start");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->side));
    c->clock_pending = false;
    unsigned long long h[2] = {0, 0};
    HIPCHK(c, hipMemcpy(h, c->d_clock.p, sizeof(h), hipMemcpyDeviceToHost));
    if (ghz) *ghz = h[1] ? (double)h[0] / ((double)h[1] * 10.0) : 0.0;      // cycles per 10 ns tick / 10 = GHz
    if (milliseconds) *milliseconds = (double)h[1] * 1e-5;
    return 0;
}

#ifdef DSMGP_DIAG
// ---- diagnostic build only (libdsmgp_hip_diag.so, include/dsmgp_hip_diag.h): never part of the product library ----
// Diagnostic: f64 MFMA and f64 VALU FMA alone and co-issued (two waves per SIMD).  out[3*mode + {0,1,2}] =
// {MFMA TFLOP/s, VALU TFLOP/s, wall ms} for mode 0 (MFMA only), 1 (VALU only), 2 (one wave of each per SIMD).
int dsmgp_probe_coissue(dsmgp_ctx* c, double* out) {
    if (!c || !out) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int blocks = c->ncu, iters = 2000;
    DevBuf<double> sink;
    DevBuf<unsigned long long> st;
    if (int rc = sink.alloc(c, (size_t)blocks * 512)) return rc;
    if (int rc = st.alloc(c, (size_t)blocks * 8 * 2)) return rc;
    for (int mode = 0; mode < 3; ++mode) {
        EventPair ev;
        HIPCHK(c, ev.init());
        coissue_probe_kernel<<<blocks, 512, 0, c->stream>>>(sink.p, st.p, iters, mode);
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        coissue_probe_kernel<<<blocks, 512, 0, c->stream>>>(sink.p, st.p, iters, mode);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
        const double waves_mfma = (mode == 0) ? 8.0 : (mode == 2 ? 4.0 : 0.0);
        const double waves_valu = (mode == 1) ? 8.0 : (mode == 2 ? 4.0 : 0.0);
        const double fl_m = (double)blocks * waves_mfma * iters * 16.0 * 2048.0;
        const double fl_v = (double)blocks * waves_valu * iters * 8.0 * 32.0 * 128.0;   // 64 lanes x 2 flops per v_fma_f64
        out[3 * mode] = fl_m / (ms * 1e-3) / 1e12;
        out[3 * mode + 1] = fl_v / (ms * 1e-3) / 1e12;
        out[3 * mode + 2] = ms;
    }
    return 0;
}

// Diagnostic: steady-state rate of tile_gemm_kernel on a uniform batch (no factorisation around it).
// mode 0: every tile has its own A panel, groups of `group` tiles share a B panel (the access pattern of
// one block step); mode 1: all tiles read the same A and B panels (operands stay in L2).
int dsmgp_bench_tile(dsmgp_ctx* c, int32_t ntiles, int32_t K, int32_t mode, int32_t group, int32_t reps,
                     double* seconds_per_launch) {
    if (!c || ntiles <= 0 || K <= 0 || K % KC || !seconds_per_launch || group <= 0) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t panel = (size_t)TB * K;
    const int nA = mode == 1 ? 1 : ((mode == 3 || mode == 5) ? (ntiles + group - 1) / group * group : ntiles);
    const int nB = mode == 1 ? 1 : (ntiles + group - 1) / group;
    if (mode == 2 && std::getenv("DSMGP_STAMPS")) return fail(c, DSMGP_E_ARG, "no stamps in mode 2");
    DevBuf<double> A, B, C;
    if (int rc = A.alloc(c, nA * panel)) return rc;
    if (int rc = B.alloc(c, nB * panel)) return rc;
    if (int rc = C.alloc(c, (size_t)ntiles * TB * TB)) return rc;
    HIPCHK(c, hipMemset(A.p, 0, nA * panel * sizeof(double)));
    HIPCHK(c, hipMemset(B.p, 0, nB * panel * sizeof(double)));
    HIPCHK(c, hipMemset(C.p, 0, (size_t)ntiles * TB * TB * sizeof(double)));
    {   // non-trivial operand values (random-ish, bounded)
        std::vector<double> hv(panel);
        for (size_t i = 0; i < panel; ++i) hv[i] = 1e-3 * (double)((i * 2654435761u) % 2001) - 1.0;
        for (int i = 0; i < nA; ++i) HIPCHK(c, hipMemcpy(A.p + i * panel, hv.data(), panel * sizeof(double), hipMemcpyHostToDevice));
        for (int i = 0; i < nB; ++i) HIPCHK(c, hipMemcpy(B.p + i * panel, hv.data(), panel * sizeof(double), hipMemcpyHostToDevice));
    }
    std::vector<TileTask> tasks(ntiles);
    for (int i = 0; i < ntiles; ++i) {
        TileTask t{};
        t.A = A.p + (mode == 1 ? 0 : (size_t)i * panel);
        t.B = B.p + (mode == 1 ? 0 : (size_t)(i / group) * panel);
        t.C = C.p + (size_t)i * TB * TB;
        t.lda = t.ldb = TB;
        if (mode == 3 || mode == 5) {   // A.p tiles are row tiles of a (group*128) x K column-major matrix, like the rows of Vt
            t.A = A.p + (size_t)(i / group) * group * panel + (size_t)(i % group) * TB;
            t.lda = group * TB;
        }
        t.ldc = TB;
        t.k0 = 0;
        t.k1 = K;
        t.update = 1;
        if (mode == 4 || mode == 5) {   // diagonal tiles of the factorisation: C.p -= A.p A.p^T, lower blocks only
            t.B = t.A;
            t.ldb = t.lda;
            t.sym = 1;
        }
        tasks[i] = t;
    }
    // mode 0/1: the raw batch; mode 2: the batch as UpdateSplitter would schedule it (split-K + reduce)
    UpdateSplitter U = make_splitter(c, 1);
    DevBuf<double> slabs;
    if (mode == 2) {
        U.add_step(tasks, K);
        if (U.max_slabs)
            if (int rc = slabs.alloc(c, U.max_slabs * TB * TB)) return rc;
        U.bind(slabs.p);
        tasks = U.upd;
        std::fprintf(stderr, "  splitter: %zu tiles -> %zu tasks, %zu reduces\n", (size_t)ntiles, tasks.size(), U.red.size());
    } else {
        std::vector<int> dummy(tasks.size());
        xcd_permute(tasks, dummy, 0, tasks.size(), c->xcd_order && (mode == 0 || mode == 6));
        // mode 6: mode 0 with the first workgroup of every CU at half depth -- the two workgroups of a CU then run half a task
        // apart for the rest of the launch instead of reaching their epilogues (and the next tasks' first loads) together
        if (mode == 6)
            for (int i = 0; i < std::min(ntiles, c->ncu); ++i) tasks[i].k1 = K / 2 / KC * KC;
    }
    DevBuf<TileTask> dt;
    DevBuf<ReduceTask> dr;
    if (int rc = dev_upload(c, dt, tasks)) return rc;
    if (int rc = dev_upload(c, dr, U.red)) return rc;
    const int nt_ = (int)tasks.size();
    auto run = [&]() {
        launch_tiles(c, dt.p, nt_);
        if (dr.count) tile_reduce_kernel<<<(int)dr.count * REDUCE_WGS, 256, 0, c->stream>>>(dr.p);
    };
    EventPair ev;
    HIPCHK(c, ev.init());
    run();
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    for (int r = 0; r < reps; ++r) run();
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    *seconds_per_launch = ms * 1e-3 / reps;
    if (std::getenv("DSMGP_STAMPS")) {
        DevBuf<unsigned long long> st;
        if (int rc = st.alloc(c, (size_t)ntiles * 32)) return rc;
        tile_gemm_kernel_v2<true><<<ntiles, 256, 0, c->stream>>>(dt.p, st.p, nullptr, 0, 0, nullptr, 0);
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::vector<unsigned long long> hs((size_t)ntiles * 32);
        HIPCHK(c, hipMemcpy(hs.data(), st.p, hs.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        double tot = 0, mf = 0, bd = 0, nchs = 0, pro = 0, loop = 0, epi = 0;
        unsigned long long first = ~0ull, last = 0;
        for (size_t i = 0; i < (size_t)ntiles * 4; ++i) {
            const unsigned long long* h = hs.data() + 8 * i;
            tot += (double)h[0];
            mf += (double)h[1];
            bd += (double)h[2];
            nchs += (double)h[3];
            pro += (double)(h[4] - h[6]);
            loop += (double)(h[5] - h[4]);
            epi += (double)(h[7] - h[5]);
            first = std::min(first, h[6]);
            last = std::max(last, h[7]);
        }
        const double nw = (double)ntiles * 4.0;
        std::fprintf(stderr,
                     "  stamps: cycles/chunk-pair total %.0f  mfma-span %.0f  boundary %.0f (per wave, mean); per wave us: "
                     "prologue %.2f  loop %.2f  epilogue %.2f  -> loop clock %.3f GHz; launch span %.1f us, sum of wave "
                     "times / (span x slots) = %.3f\n",
                     tot / nchs, mf / nchs, bd / nchs, pro / nw * 0.01, loop / nw * 0.01, epi / nw * 0.01,
                     tot / loop / 10.0, (double)(last - first) * 0.01,
                     (pro + loop + epi) / ((double)(last - first) * std::min<double>(2.0 * c->ncu * 4.0, nw)));
    }
    return 0;
}
// Diagnostic: the eight-wave fused tile task (tile_fused8_kernel) on a uniform batch of `ntasks` tasks of depth K -- eight full
// 16-row blocks each with their own A rows, groups of `group` tasks sharing a B panel, the access pattern of bench_tile's mode 0.
// A task of depth K is its kernel function, K / 128 block columns of product, one substitution and a store: the SLOPE of the
// launch time over K is the steady-state rate of the eight-wave product loop (four waves per SIMD), to set against
// tile_gemm_kernel_v2's (two waves per SIMD) on the same shape.
int dsmgp_bench_fused8(dsmgp_ctx* c, int32_t ntasks, int32_t K, int32_t group, int32_t reps, double* seconds_per_launch) {
    if (!c || ntasks <= 0 || K < 0 || K % TB || !seconds_per_launch || group <= 0 || reps <= 0) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int D = 8;
    const size_t apanel = (size_t)TB * K, bpanel = (size_t)TB * (K + TB);
    const int nB = (ntasks + group - 1) / group;
    DevBuf<double> A, B, Cc, Dv, gx, l2;
    DevBuf<KParam> kp;
    if (int rc = A.alloc(c, std::max<size_t>(1, (size_t)ntasks * apanel))) return rc;
    if (int rc = B.alloc(c, (size_t)nB * bpanel)) return rc;
    if (int rc = Cc.alloc(c, (size_t)ntasks * TB * TB)) return rc;
    if (int rc = Dv.alloc(c, (size_t)TB * TB)) return rc;
    if (int rc = gx.alloc(c, (size_t)TB * D)) return rc;
    if (int rc = l2.alloc(c, 2)) return rc;
    if (int rc = kp.alloc(c, 1)) return rc;
    {
        std::vector<double> hv(std::max(apanel, bpanel));
        for (size_t i = 0; i < hv.size(); ++i) hv[i] = 1e-3 * (double)((i * 2654435761u) % 2001) - 1.0;
        for (int i = 0; i < ntasks && apanel; ++i) HIPCHK(c, hipMemcpy(A.p + i * apanel, hv.data(), apanel * sizeof(double), hipMemcpyHostToDevice));
        for (int i = 0; i < nB; ++i) HIPCHK(c, hipMemcpy(B.p + i * bpanel, hv.data(), bpanel * sizeof(double), hipMemcpyHostToDevice));
        std::vector<double> id((size_t)TB * TB, 0.0), xs((size_t)TB * D);
        for (int i = 0; i < TB; ++i) id[i + (size_t)i * TB] = 1.0;
        for (size_t i = 0; i < xs.size(); ++i) xs[i] = 1e-3 * (double)((i * 40503u) % 1000);
        HIPCHK(c, hipMemcpy(Dv.p, id.data(), id.size() * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(c, hipMemcpy(gx.p, xs.data(), xs.size() * sizeof(double), hipMemcpyHostToDevice));
        const double hl2[2] = {1.0, -0.5};
        HIPCHK(c, hipMemcpy(l2.p, hl2, sizeof(hl2), hipMemcpyHostToDevice));
        KParam h{};
        h.kind = 0;
        h.nl = 1;
        h.sigma2 = h.sigma = 1.0;
        h.noise = 0.01;
        h.l2 = l2.p;
        h.nh = l2.p + 1;
        h.nh0 = -0.5;
        h.il2 = 1.0;
        HIPCHK(c, hipMemcpy(kp.p, &h, sizeof(h), hipMemcpyHostToDevice));
    }
    std::vector<FusedTask8> tasks(ntasks);
    for (int i = 0; i < ntasks; ++i) {
        FusedTask8 t{};
        t.B = B.p + (size_t)(i / group) * bpanel;
        t.Dinv = Dv.p;
        t.zk = nullptr;
        t.gxb = gx.p;
        t.ldb = TB;
        t.gldb = TB;
        t.gnb = TB;
        t.k1 = K;
        t.kid = 0;
        t.nblk = 8;
        for (int w = 0; w < 8; ++w) {
            RowBlock& r = t.rb[w];
            r.A = (K ? A.p + (size_t)i * apanel : B.p) + 16 * w;
            r.C = Cc.p + (size_t)i * TB * TB + 16 * w;
            r.gx = gx.p + 16 * w;
            r.wi = nullptr;
            r.sq = nullptr;
            r.lda = TB;
            r.ldc = TB;
            r.glda = TB;
            r.nvalid = 16;
        }
        tasks[i] = t;
    }
    {
        std::vector<int> dummy(tasks.size());
        xcd_permute(tasks, dummy, 0, tasks.size(), c->xcd_order);
    }
    DevBuf<FusedTask8> dt;
    if (int rc = dev_upload(c, dt, tasks)) return rc;
    auto run = [&]() { tile_fused8_kernel<2><<<ntasks, 512, 0, c->stream>>>(dt.p, kp.p, D); };
    EventPair ev;
    HIPCHK(c, ev.init());
    run();
    HIPCHK(c, hipEventRecord(ev.a, c->stream));
    for (int r = 0; r < reps; ++r) run();
    HIPCHK(c, hipEventRecord(ev.b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
    *seconds_per_launch = ms * 1e-3 / reps;
    return 0;
}
// Diagnostic: the diagonal-block kernel alone on `ntiles` well-conditioned blocks (microseconds per launch over `reps`
// launches) and the wall-clock phases of block 0's wave 0 from one stamped launch: phases_us[0..19] = load, first
// 16x16 block, then (P1, P2) of the 8 block steps, write-back, inverse phase; [20], [21] = inside step 3's P2 on wave 0:
// the trailing product of the next diagonal block, its potrf + inverse (potrf_inv16 with its LDS reads and writes);
// [22] = shader cycles of [21].
int dsmgp_probe_diag(dsmgp_ctx* c, int32_t ntiles, int32_t ld, int32_t reps, double* kernel_us, double* phases_us) {
    if (!c || ntiles <= 0 || ld < TB || reps <= 0 || !kernel_us || !phases_us) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t tile = (size_t)ld * TB;
    std::vector<double> h(tile, 0.0);
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        return (double)(st >> 11) * (1.0 / 9007199254740992.0) - 0.5;
    };
    for (int cidx = 0; cidx < TB; ++cidx)
        for (int r = cidx; r < TB; ++r) h[r + (size_t)cidx * ld] = (r == cidx) ? 64.0 + rnd() : rnd();
    DevBuf<double> T0, T, Dinv, wz;
    DevBuf<int> info;
    DevBuf<unsigned long long> stamps;
    DevBuf<DiagTask> dt;
    if (int rc = T0.alloc(c, tile)) return rc;
    if (int rc = T.alloc(c, ntiles * tile)) return rc;
    if (int rc = Dinv.alloc(c, (size_t)ntiles * TB * TB)) return rc;
    if (int rc = wz.alloc(c, (size_t)ntiles * 2 * TB)) return rc;
    if (int rc = info.alloc(c, ntiles)) return rc;
    if (int rc = stamps.alloc(c, (size_t)ntiles * 24)) return rc;
    if (int rc = dt.alloc(c, ntiles)) return rc;
    HIPCHK(c, hipMemcpy(T0.p, h.data(), tile * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(wz.p, 0, (size_t)ntiles * 2 * TB * sizeof(double)));
    HIPCHK(c, hipMemset(Dinv.p, 0, (size_t)ntiles * TB * TB * sizeof(double)));
    HIPCHK(c, hipMemset(info.p, 0, ntiles * sizeof(int)));
    std::vector<DiagTask> tasks(ntiles);
    for (int i = 0; i < ntiles; ++i) {
        DiagTask g{};
        g.T = T.p + i * tile;
        g.Dinv = Dinv.p + (size_t)i * TB * TB;
        g.wk = wz.p + (size_t)i * 2 * TB;
        g.zk = wz.p + (size_t)i * 2 * TB + TB;
        g.info = info.p + i;
        g.ld = ld;
        g.nvalid = TB;
        g.row0 = 0;
        tasks[i] = g;
    }
    HIPCHK(c, hipMemcpy(dt.p, tasks.data(), ntiles * sizeof(DiagTask), hipMemcpyHostToDevice));
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(chol_diag_packed_stamp_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, DIAGP_LDS_BYTES);
    const size_t lds = DIAGP_LDS_BYTES;
    EventPair ev;
    HIPCHK(c, ev.init());
    auto refill = [&]() {
        for (int i = 0; i < ntiles; ++i)
            (void)hipMemcpyAsync(T.p + i * tile, T0.p, tile * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
    };
    double total = 0.0;
    for (int r = 0; r < reps + 1; ++r) {
        refill();
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        chol_diag_packed_kernel<<<ntiles, 256, lds, c->stream>>>(dt.p);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
        if (r > 0) total += ms;
    }
    *kernel_us = total / reps * 1e3;
    refill();
    chol_diag_packed_stamp_kernel<<<ntiles, 256, lds, c->stream>>>(dt.p, stamps.p);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long hs[24];
    HIPCHK(c, hipMemcpy(hs, stamps.p, sizeof(hs), hipMemcpyDeviceToHost));
    for (int i = 0; i < 20; ++i) phases_us[i] = (double)(hs[i + 1] - hs[i]) * 0.01;   // 100 MHz
    phases_us[20] = (double)(hs[21] - hs[9]) * 0.01;
    phases_us[21] = (double)(hs[22] - hs[21]) * 0.01;
    phases_us[22] = (double)hs[23];                       // shader cycles of the interval of [21]
    int bad = 0;
    HIPCHK(c, hipMemcpy(&bad, info.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad != 0) return fail(c, DSMGP_E_STATE, "probe block was not positive definite");
    return 0;
}

// diagnostic: the diagonal-block task of a FUSED step (diag_fused_reg_kernel) alone on ntiles synthetic blocks of depth K: IsoSE
// values of random points in [0, 1)^8 (l = 0.3, noise 0.01) minus a small product -- what a depth-4 fit launches 18k of per step.
// ntiles = 256 / 512 / 768 puts one / two / three tasks on every CU: the latency of a task alone and what co-residents cost it.
int dsmgp_probe_diag_fused(dsmgp_ctx* c, int32_t ntiles, int32_t K, int32_t reps, double* kernel_us) {
    if (!c || ntiles <= 0 || K < 0 || K % TB != 0 || reps <= 0 || !kernel_us) return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const int D = 8;
    const size_t leaf = (size_t)TB * (size_t)(K + TB);          // block row: 128 rows x (K + 128) columns, ld = 128
    uint64_t st = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        st ^= st << 13; st ^= st >> 7; st ^= st << 17;
        return (double)(st >> 11) * (1.0 / 9007199254740992.0);
    };
    std::vector<double> hx((size_t)TB * D), ha((size_t)TB * std::max(K, 1));
    for (double& v : hx) v = rnd();
    for (double& v : ha) v = (rnd() - 0.5) * 2e-3;
    DevBuf<double> F, X, Dinv, wz, nh;
    DevBuf<int> info;
    DevBuf<DiagFusedTask> dt;
    DevBuf<KParam> kp;
    if (int rc = F.alloc(c, (size_t)ntiles * leaf)) return rc;
    if (int rc = X.alloc(c, (size_t)TB * D)) return rc;
    if (int rc = Dinv.alloc(c, (size_t)ntiles * TB * TB)) return rc;
    if (int rc = wz.alloc(c, (size_t)ntiles * 2 * TB)) return rc;
    if (int rc = info.alloc(c, ntiles)) return rc;
    if (int rc = dt.alloc(c, ntiles)) return rc;
    if (int rc = kp.alloc(c, 1)) return rc;
    if (int rc = nh.alloc(c, 2)) return rc;
    HIPCHK(c, hipMemset(F.p, 0, (size_t)ntiles * leaf * sizeof(double)));
    HIPCHK(c, hipMemset(Dinv.p, 0, (size_t)ntiles * TB * TB * sizeof(double)));
    HIPCHK(c, hipMemset(wz.p, 0, (size_t)ntiles * 2 * TB * sizeof(double)));
    HIPCHK(c, hipMemset(info.p, 0, ntiles * sizeof(int)));
    HIPCHK(c, hipMemcpy(X.p, hx.data(), hx.size() * sizeof(double), hipMemcpyHostToDevice));
    if (K > 0)
        for (int i = 0; i < ntiles; ++i)
            HIPCHK(c, hipMemcpyAsync(F.p + (size_t)i * leaf, ha.data(), (size_t)TB * K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const double l2 = 0.09, hnh[2] = {-0.5 / l2, l2};
    HIPCHK(c, hipMemcpy(nh.p, hnh, sizeof(hnh), hipMemcpyHostToDevice));
    KParam p{};
    p.kind = DSMGP_KIND_ISO_SE;
    p.nl = 1;
    p.sigma2 = p.sigma = 1.0;
    p.noise = 0.01;
    p.l2 = nh.p + 1;
    p.nh = nh.p;
    p.nh0 = hnh[0];
    p.il2 = 1.0 / l2;
    HIPCHK(c, hipMemcpy(kp.p, &p, sizeof(p), hipMemcpyHostToDevice));
    std::vector<DiagFusedTask> tasks(ntiles);
    for (int i = 0; i < ntiles; ++i) {
        DiagFusedTask f{};
        f.d.T = F.p + (size_t)i * leaf + (size_t)K * TB;
        f.d.Dinv = Dinv.p + (size_t)i * TB * TB;
        f.d.wk = wz.p + (size_t)i * 2 * TB;
        f.d.zk = wz.p + (size_t)i * 2 * TB + TB;
        f.d.info = info.p + i;
        f.d.ld = TB;
        f.d.nvalid = TB;
        f.d.row0 = 0;
        f.A = F.p + (size_t)i * leaf;
        f.gx = X.p;
        f.k1 = K;
        f.glda = TB;
        f.kid = 0;
        tasks[i] = f;
    }
    HIPCHK(c, hipMemcpy(dt.p, tasks.data(), ntiles * sizeof(DiagFusedTask), hipMemcpyHostToDevice));
    EventPair ev;
    HIPCHK(c, ev.init());
    double total = 0.0;
    for (int r = 0; r < reps + 1; ++r) {
        HIPCHK(c, hipEventRecord(ev.a, c->stream));
        diag_fused_reg_kernel<<<ntiles, 256, DIAGR_LDS_BYTES, c->stream>>>(dt.p, kp.p, D);
        HIPCHK(c, hipEventRecord(ev.b, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
        if (r > 0) total += ms;
    }
    *kernel_us = total / reps * 1e3;
    int bad = 0;
    HIPCHK(c, hipMemcpy(&bad, info.p, sizeof(int), hipMemcpyDeviceToHost));
    if (bad != 0) return fail(c, DSMGP_E_STATE, "probe block was not positive definite");
    return 0;
}

// diagnostic: the kept blocks of `nleaves` leaves of kb x kb blocks each, from factors of leading dimension ld_old into factors of
// leading dimension ld_new (and their kb Dinv blocks), three ways: out[0] = seconds of the ONE relocate_tiles_kernel launch of
// dsmgp_append_rows, out[1] = of one device-to-device hipMemcpy of the same byte count (contiguous: the ceiling), out[2] = of the
// hipMemcpy2DAsync + hipMemcpyAsync pair per leaf the PREFIX phase of dsmgp_fit issues, out[3] = bytes moved.  Best of `reps`.
int dsmgp_bench_relocate(dsmgp_ctx* c, int32_t nleaves, int32_t kb, int32_t ld_old, int32_t ld_new, int32_t reps, double* out) {
    if (!c || !out || nleaves < 1 || kb < 1 || reps < 1 || ld_old < kb * TB || ld_new < kb * TB || ld_old % TB || ld_new % TB)
        return DSMGP_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t fo = (size_t)ld_old * ld_old, fn = (size_t)ld_new * ld_new, dv = (size_t)kb * TB * TB;
    DevBuf<double> Fo, Fn, Do, Dn;
    if (int rc = Fo.alloc(c, fo * nleaves)) return rc;
    if (int rc = Fn.alloc(c, fn * nleaves)) return rc;
    if (int rc = Do.alloc(c, dv * nleaves)) return rc;
    if (int rc = Dn.alloc(c, dv * nleaves)) return rc;
    HIPCHK(c, hipMemset(Fo.p, 0, fo * nleaves * sizeof(double)));
    HIPCHK(c, hipMemset(Do.p, 0, dv * nleaves * sizeof(double)));
    std::vector<RelocTask> rt;
    for (int l = 0; l < nleaves; ++l)
        for (int j = 0; j < kb; ++j) {
            for (int i = 0; i < kb; ++i)
                rt.push_back(RelocTask{Fo.p + l * fo + (size_t)i * TB + (size_t)j * TB * ld_old,
                                       Fn.p + l * fn + (size_t)i * TB + (size_t)j * TB * ld_new, ld_old, ld_new});
            rt.push_back(RelocTask{Do.p + l * dv + (size_t)j * TB * TB, Dn.p + l * dv + (size_t)j * TB * TB, TB, TB});
        }
    DevBuf<RelocTask> tasks;
    if (int rc = dev_upload(c, tasks, rt)) return rc;
    const size_t bytes = rt.size() * TB * TB * sizeof(double);
    DevBuf<double> flat_a, flat_b;
    if (int rc = flat_a.alloc(c, bytes / sizeof(double))) return rc;
    if (int rc = flat_b.alloc(c, bytes / sizeof(double))) return rc;
    EventPair ev;
    HIPCHK(c, ev.init());
    const size_t rows = (size_t)kb * TB;
    out[0] = out[1] = out[2] = 1e30;
    for (int r = 0; r <= reps; ++r)         // (pass 0 warms up)
        for (int way = 0; way < 3; ++way) {
            HIPCHK(c, hipEventRecord(ev.a, c->stream));
            if (way == 0) {
                relocate_tiles_kernel<<<(unsigned)tasks.count, 256, 0, c->stream>>>(tasks.p);
            } else if (way == 1) {
                HIPCHK(c, hipMemcpyAsync(flat_b.p, flat_a.p, bytes, hipMemcpyDeviceToDevice, c->stream));
            } else {
                for (int l = 0; l < nleaves; ++l) {
                    HIPCHK(c, hipMemcpy2DAsync(Fn.p + l * fn, (size_t)ld_new * sizeof(double), Fo.p + l * fo, (size_t)ld_old * sizeof(double),
                                               rows * sizeof(double), rows, hipMemcpyDeviceToDevice, c->stream));
                    HIPCHK(c, hipMemcpyAsync(Dn.p + l * dv, Do.p + l * dv, dv * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
                }
            }
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipEventRecord(ev.b, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            float ms = 0.f;
            HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
            if (r > 0) out[way] = std::min(out[way], (double)ms * 1e-3);
        }
    out[3] = (double)bytes;
    return 0;
}

#endif  // DSMGP_DIAG

// -------------------------------------------------------------------------------------------------
// The one exchange step of the path when leaves are sharded over the GPUs of a node: an all-gather of
// per-leaf log-marginals after fit! and of the aggregation's partial sums after predict, over RCCL (xGMI inside a node)
// on the context's stream.  librccl.so is opened with dlopen on first use: a single-GPU process never loads it, and
// the library itself has no link-time dependency on it.
namespace {
struct RcclApi {
    void* lib = nullptr;
    struct UniqueId { char internal[128]; };                         // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128)
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
    bool load() {
        if (lib) return true;
        // First choice: the librccl that sits NEXT TO the HIP runtime this library is bound to.  A process can hold two
        // ROCm runtimes -- the system's, and the one a PyTorch wheel bundles and maps under the plain names "librccl.so" /
        // "libamdhip64.so" -- and only the first of them to initialise owns the GPU.  dlopen("librccl.so") returns whichever
        // copy is already mapped under that name: with this library loaded first and torch imported later that was torch's
        // librccl on top of torch's never-initialised runtime, and ncclCommInitRank failed with 'no ROCm-capable device is
        // detected'.  (Loaded after torch, this library binds to torch's runtime by SONAME and the first choice IS torch's copy.)
        std::vector<std::string> names;
        Dl_info di;
        if (dladdr(reinterpret_cast<void*>(&hipGetDeviceCount), &di) && di.dli_fname) {
            const std::string f(di.dli_fname);
            const size_t p = f.rfind('/');
            if (p != std::string::npos) {
                names.push_back(f.substr(0, p + 1) + "librccl.so.1");
                names.push_back(f.substr(0, p + 1) + "librccl.so");
            }
        }
        for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so"}) names.push_back(n);
        for (const std::string& name : names) {
            lib = dlopen(name.c_str(), RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) {
            err = std::string("cannot load librccl.so: ") + dlerror();
            return false;
        }
        GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
        CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
        AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(lib, "ncclAllGather"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!GetUniqueId || !CommInitRank || !AllGather || !CommDestroy) {
            err = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy";
            lib = nullptr;
            return false;
        }
        return true;
    }
    std::string what(int rc) { return GetErrorString ? GetErrorString(rc) : ("nccl error " + std::to_string(rc)); }
};
RcclApi g_rccl;
constexpr int NCCL_FLOAT64 = 8;   // ncclDataType_t ncclFloat64 (rccl.h)
}  // namespace

int dsmgp_comm_unique_id(char* id_out) {
    if (!id_out) return DSMGP_E_ARG;
    if (!g_rccl.load()) return fail(nullptr, DSMGP_E_STATE, g_rccl.err);
    RcclApi::UniqueId id;
    const int rc = g_rccl.GetUniqueId(&id);
    if (rc != 0) return fail(nullptr, DSMGP_E_HIP, "ncclGetUniqueId: " + g_rccl.what(rc));
    std::memcpy(id_out, id.internal, sizeof(id.internal));
    return 0;
}

int dsmgp_comm_init(dsmgp_ctx* c, int32_t rank, int32_t world, const char* id) {
    if (!c) return DSMGP_E_ARG;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(c, DSMGP_E_ARG, "comm_init: bad arguments");
    if (c->comm) return fail(c, DSMGP_E_STATE, "comm_init: communicator already initialised");
    if (!g_rccl.load()) return fail(c, DSMGP_E_STATE, g_rccl.err);
    HIPCHK(c, hipSetDevice(c->device));
    RcclApi::UniqueId uid;
    std::memcpy(uid.internal, id, sizeof(uid.internal));
    const int rc = g_rccl.CommInitRank(&c->comm, world, uid, rank);
    if (rc != 0) {
        c->comm = nullptr;
        return fail(c, DSMGP_E_HIP, "ncclCommInitRank: " + g_rccl.what(rc));
    }
    c->comm_rank = rank;
    c->comm_world = world;
    return 0;
}

namespace {
// all-gather of `n` doubles per rank, device to device on the context's stream: d_xchg = [send n | recv world * n]
int xchg_reserve(dsmgp_ctx* c, size_t n) {
    const size_t need = n * (size_t)(c->comm_world + 1);
    return need > c->d_xchg.cap ? c->d_xchg.alloc(c, need) : 0;
}
int xchg_gather(dsmgp_ctx* c, size_t n) {
    const int rc = g_rccl.AllGather(c->d_xchg.p, c->d_xchg.p + n, n, NCCL_FLOAT64, c->comm, c->stream);
    if (rc != 0) return fail(c, DSMGP_E_HIP, "ncclAllGather: " + g_rccl.what(rc));
    return 0;
}
}  // namespace

int dsmgp_allgather(dsmgp_ctx* c, const double* send, int64_t count, double* recv) {
    if (!c) return DSMGP_E_ARG;
    if (!c->comm) return fail(c, DSMGP_E_STATE, "allgather before comm_init");
    if (!send || !recv || count <= 0) return fail(c, DSMGP_E_ARG, "allgather: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)count;
    if (int rc = xchg_reserve(c, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_xchg.p, send, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int rc = xchg_gather(c, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(recv, c->d_xchg.p + n, n * (size_t)c->comm_world * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int dsmgp_fit_exchange(dsmgp_ctx* c, int64_t count, double* out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->comm) return fail(c, DSMGP_E_STATE, "fit_exchange before comm_init");
    if (!out || count <= 0 || count < c->L) return fail(c, DSMGP_E_ARG, "fit_exchange: count must cover this rank's leaves");
    if (c->L > 0 && !c->has(P_FIT)) return fail(c, DSMGP_E_STATE, "fit_exchange before fit");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = 2 * (size_t)count;
    if (int rc = xchg_reserve(c, n)) return rc;
    if (c->L > 0) {
        // info lives per factor owner (the table is the plan's: build_plan)
        pack_mll_info_kernel<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(c->d_mll.p, c->d_info.p, c->d_owner.p, c->L, count, c->d_xchg.p);
        HIPCHK(c, hipGetLastError());
    } else {
        HIPCHK(c, hipMemsetAsync(c->d_xchg.p, 0, n * sizeof(double), c->stream));
    }
    if (int rc = xchg_gather(c, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->d_xchg.p + n, n * (size_t)c->comm_world * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int dsmgp_aggregate_exchange(dsmgp_ctx* c, double* total_out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->comm) return fail(c, DSMGP_E_STATE, "aggregate_exchange before comm_init");
    if (!c->has(P_PARTIAL)) return fail(c, DSMGP_E_STATE, "aggregate_exchange before aggregate_partial");
    if (c->has(P_TOTAL)) return fail(c, DSMGP_E_STATE, "aggregate_exchange: these partial sums already hold the total over ranks");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->agg.W * (size_t)c->n_t;
    if (int rc = xchg_reserve(c, n)) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_xchg.p, c->d_agg_part.p, n * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if (int rc = xchg_gather(c, n)) return rc;
    sum_ranks_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->d_xchg.p + n, c->comm_world, (int64_t)n, c->d_agg_part.p);
    HIPCHK(c, hipGetLastError());
    if (total_out) HIPCHK(c, hipMemcpyAsync(total_out, c->d_agg_part.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mark(P_TOTAL);
    return 0;
}

int dsmgp_aggregate_exchange_empty(dsmgp_ctx* c, int32_t W, int64_t n_t, double* total_out) {
    if (!c) return DSMGP_E_ARG;
    if (!c->comm) return fail(c, DSMGP_E_STATE, "aggregate_exchange before comm_init");
    if (W <= 0 || n_t <= 0) return fail(c, DSMGP_E_ARG, "aggregate_exchange_empty: bad arguments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)W * (size_t)n_t;
    if (int rc = xchg_reserve(c, n)) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_xchg.p, 0, n * sizeof(double), c->stream));
    if (int rc = xchg_gather(c, n)) return rc;
    if (total_out) {
        sum_ranks_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(c->d_xchg.p + n, c->comm_world, (int64_t)n, c->d_xchg.p);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(total_out, c->d_xchg.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}

int dsmgp_comm_destroy(dsmgp_ctx* c) {
    if (!c) return DSMGP_E_ARG;
    if (c->comm) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);
        (void)g_rccl.CommDestroy(c->comm);
        c->comm = nullptr;
    }
    c->d_xchg.release();
    c->comm_world = 1;
    c->comm_rank = 0;
    return 0;
}

}  // extern "C"
