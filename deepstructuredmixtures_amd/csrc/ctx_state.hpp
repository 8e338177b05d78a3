// What a context holds that is CURRENT: one bit per product and one table of what each product is made from.  A writer invalidates
// what it changed, and what was made from that falls with it; a builder marks what it made; a reader asks has().  Plain C++17,
// neither HIP nor dsmgp_hip.h: tests/ctx_state_dump.cpp prints the table for the host suite.
#pragma once
#include <cassert>
#include <cstdint>
namespace ctx_state {
enum Product : uint32_t {
    P_PLAN = 1u << 0, P_PHASE = 1u << 1, P_TEST = 1u << 2, P_JOINT = 1u << 3, P_FIT = 1u << 4, P_ALPHA = 1u << 5, P_DINV = 1u << 6,
    P_VT = 1u << 7, P_PRED = 1u << 8, P_PARTIAL = 1u << 9, P_TOTAL = 1u << 10, P_DONE = 1u << 11, P_GRAD_LISTS = 1u << 12,
    P_XINV = 1u << 13, P_LOO_LISTS = 1u << 14, P_LG_LISTS = 1u << 15, P_TG_LISTS = 1u << 16, P_Z = 1u << 17, P_RTREE = 1u << 18,
    P_PGRAD = 1u << 19, P_GSUMS = 1u << 20, P_TMU = 1u << 21, P_TIG = 1u << 22, P_CDONE = 1u << 23, P_SAMPLE = 1u << 24,
};
struct Row { Product product; const char* name; uint32_t parents; };

// The chains: each product, its DIRECT parents (what it is made from or points into) and the lifetime group of dsmgp_ctx that
// holds its storage (csrc/dsmgp_hip.cpp: the group's declarations are the list of what falls; a CONTENT product names the group
// whose arenas it fills).  The hyper-parameters, the options and the mask are inputs: their setters invalidate what was made
// from them (dsmgp_set_hyper the fit).
constexpr Row TABLE[] = {
    {P_PLAN,       "plan",         0},                   // PlanStore, as build_plan makes it
    {P_PHASE,      "phase_lists",  P_PLAN},              // PlanStore: the steps of a fit without resident test rows (ensure_phase)
    {P_TEST,       "test",         P_PLAN},              // TestInputs and TestProducts: the lists point into the plan's arenas
    {P_JOINT,      "joint_lists",  P_PLAN | P_TEST},     // TestProducts: the steps of a fit with the test rows riding along (ensure_joint)
    {P_FIT,        "fit",          P_PLAN},              // content of PlanStore: L, z, mll, info for the current hyper-parameters
    {P_ALPHA,      "alpha",        P_FIT},               // content of PlanStore: alpha = L^-T z (ensure_alpha)
    {P_DINV,       "dinv",         P_FIT},               // content of PlanStore: every Dinv_k whole: a fit's fused steps leave the 16x16 diagonal inverses only (ensure_dinv)
    {P_VT,         "vt",           P_FIT | P_TEST},      // content of TestProducts: K_tn L^-T, from the fit the rows rode through or from predict_run's sweep
    {P_PRED,       "prediction",   P_FIT | P_TEST},      // content of TestProducts: mu | var of every routed row
    {P_PARTIAL,    "partial",      P_PRED},              // content of TestProducts: this context's sums (agg_family / agg_G / agg_W describe them)
    {P_TOTAL,      "total",        P_PARTIAL},           // ... summed over the ranks (dsmgp_aggregate_exchange ran on them)
    {P_DONE,       "done",         P_PARTIAL},           // content of TestProducts: the aggregated moments
    {P_GRAD_LISTS, "grad_lists",   P_PLAN},              // GradLists: the gradient pass under the current mask
    {P_XINV,       "xinv",         P_FIT | P_PLAN},      // content of GradStore: L^-T of EVERY factor owner.  The leaf table's arena, not the lists': it outlives them
    {P_LOO_LISTS,  "loo_lists",    P_PLAN},              // GradStore: the lists of dsmgp_loo, they point into its L^-T arena
    {P_LG_LISTS,   "lg_lists",     P_PLAN},              // GradStore: the arena and the lists of dsmgp_loo_gradients
    {P_TG_LISTS,   "target_lists", P_PLAN},              // TargetsStore: the sweep's lists for tg_qpad columns
    {P_Z,          "targets",      P_FIT | P_TG_LISTS},  // content of TargetsStore: Z = L^-1 (Y - mean)
    {P_RTREE,      "routing_tree", 0},                   // RouteTreeStore: the model's tree (dsmgp_set_tree)
    {P_PGRAD,      "pred_gradients", P_PRED},            // content of TestProducts: dmu AND dvar of every routed row (d_pgout, both halves)
    {P_GSUMS,      "gradient_sums", P_PGRAD | P_DONE},   // content of TestProducts: this context's gradient sums about the aggregated moments
    {P_TMU,        "column_means", P_PRED | P_Z},        // content of TestProducts: the means of every resident column per routed row (d_tmu)
    {P_TIG,        "column_mean_gradients", P_PRED | P_Z},   // content of TestProducts: their input gradients (d_tigout)
    {P_CDONE,      "column_moments", P_TMU},             // content of TestProducts: the aggregated moments of the columns (col_family / col_G describe them)
    {P_SAMPLE,     "sample_factors", P_PRED},            // content of TestProducts: chol(Sigma_l + jitter I) of every leaf (sample_noise / sample_jitter tag them)
};
constexpr int N_PRODUCTS = (int)(sizeof(TABLE) / sizeof(TABLE[0]));

struct Closure { uint32_t above[N_PRODUCTS]; bool sound; };
constexpr Closure close_table() {       // above[i] = every ancestor of row i
    Closure c{};
    for (int i = 0; i < N_PRODUCTS; ++i) c.above[i] = TABLE[i].parents;
    for (int round = 0; round < N_PRODUCTS; ++round)
        for (int i = 0; i < N_PRODUCTS; ++i)
            for (int p = 0; p < N_PRODUCTS; ++p)
                if (c.above[i] >> p & 1u) c.above[i] |= c.above[p];
    c.sound = true;         // row i is bit i, and no product is its own descendant
    for (int i = 0; i < N_PRODUCTS; ++i) c.sound = c.sound && TABLE[i].product == 1u << i && !(c.above[i] >> i & 1u);
    return c;
}
constexpr Closure CLOSURE = close_table();
static_assert(CLOSURE.sound, "one row per product, in bit order, and no cycle");

constexpr int index_of(Product p) { return p == 1u ? 0 : 1 + index_of(Product(p >> 1)); }
constexpr uint32_t parents_of(Product p) { return TABLE[index_of(p)].parents; }
constexpr uint32_t falls_with(uint32_t mask) {      // the mask and everything below it
    uint32_t out = mask;
    for (int i = 0; i < N_PRODUCTS; ++i)
        if (CLOSURE.above[i] & mask) out |= 1u << i;
    return out;
}
// Whoever reads Vt asks for the prediction alone: dsmgp_predict_run marks Vt before it, and whatever fells Vt fells it too
static_assert(!(CLOSURE.above[index_of(P_VT)] & ~CLOSURE.above[index_of(P_PRED)]), "a prediction implies Vt");

struct Validity {       // base of dsmgp_ctx
    uint32_t valid = 0;
    void invalidate(uint32_t mask) { valid &= ~falls_with(mask); }
    void mark(Product p) {
        assert((valid & parents_of(p)) == parents_of(p) && "a product is marked while one of its parents is not current");
        valid |= p;
    }
    bool has(Product p) const { return (valid & p) != 0; }
};
}  // namespace ctx_state
