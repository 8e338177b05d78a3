// predict(model, x): sum/product aggregation of the leaf moments over the leaves every test row visits
// (src/common.jl:134-149,198-302) and the score functions (src/scorefunctions.jl:6-16), on the moments left in HBM
// by pred_finish_kernel; the input gradients of the aggregated prediction; and both for every resident target column.
// All four model families reduce to per-row sums over (leaf, row) entries:
//   mixture (DSMGP, :275-302): the nested log-domain recursion is linear in (mu, mu^2, sigma^2) -- unrolled it is the
//       flat mixture with weight W_l = product of the sum-node weights on leaf l's path: S0 = sum W mu,
//       S1 = sum W mu^2, S2 = sum W sigma^2 (sigma^2 <= 0 -> 1e-8, :137); mu = S0, var = S2 + S1 - S0^2
//   PoE / gPoE (:145-149,198-222): t = 1/sigma^2; P = sum beta t mu, T = sum beta t (beta = 1 resp. 1/#root children)
//   rBCM (:224-241): per root child g the PoE sums (P_g, T_g) with beta = 1, combined over the children with the prior
// A FAMILY IS DEFINED HERE ONCE: the agg_* rule functions below are its arithmetic (entry term, finish, and the same two for
// the input gradients), and the six kernels after them only walk a row's entries in ascending entry order (= leaf order: fixed
// summation order, no atomics), choose where the sums live -- [k][row] planes in HBM for the *_partial kernels, whose sums are
// added over ranks or contexts before the finish step; registers for the columns kernels -- and store.
#pragma once
#include "kernels.hpp"

namespace dsmgp {

constexpr int AGG_MIXTURE = 0, AGG_POE = 1, AGG_GPOE = 2, AGG_RBCM = 3;

struct AggRows {
    const int64_t* row_ptr;     // n_t + 1: entries of every test row
    const int32_t* row_ent;     // entry positions (index into mu / var), ascending per row
    const int32_t* ent_leaf;    // leaf of every entry position
};

// The arguments of the four kernels that walk the entries.  Planes of the per-entry arrays: ld = route_total apart.
struct AggArgs {
    AggRows rows;
    const double* mu;           // per (leaf, routed row), route order; columns: [pos + q * ld]
    const double* var;          // [pos]
    const double* dmu;          // gradients: [pos + d * ld]; columns: [pos + d * ld + q * ld * D]
    const double* dvar;         // gradients: [pos + d * ld]
    const double* coef;         // per leaf: W_l (mixture) or beta_l (PoE / gPoE); unused for rBCM
    const int32_t* group;       // per leaf: root child (rBCM); else unused
    const double* agg_mu;       // agg_grad_partial_kernel: n_t, the aggregated mean (mixture)
    const KParam* kp;           // columns: the rBCM prior is kp[prior_kid] at Xt (n_t x D)
    const double* Xt;
    double* out;                // partial: W x n_t planes; columns: mu n_t x Q, dmu [r + d * n_t + q * n_t * D]
    double* out_v;              // columns: var, dvar
    int64_t n_t;
    int64_t ld;                 // route_total
    int D, Q, family, G, plain, prior_kid;
};

// f(pos, leaf) for every entry of row r, ascending
template <class F>
__device__ __forceinline__ void agg_walk(const AggRows& w, int64_t r, F&& f) {
    for (int64_t e = w.row_ptr[r], e1 = w.row_ptr[r + 1]; e < e1; ++e) {
        const int pos = w.row_ent[e];
        f(pos, w.ent_leaf[pos]);
    }
}

// ---- the moments ----
__device__ __forceinline__ void agg_mix_term(double w, double m, double v, double& s0, double& s1, double& s2) {
    if (v <= 0.0) v = 1e-8;                                       // src/common.jl:137
    s0 += w * m;
    s1 += w * (m * m);
    s2 += w * v;
}

// PoE / gPoE: b = beta_l; rBCM: b = 1.0 (the product is exact).  src/common.jl:148
__device__ __forceinline__ void agg_prod_term(double b, double m, double v, double& P, double& T) {
    const double bt = b * (1.0 / v);
    P += bt * m;
    T += bt;
}

// plain: the root is a single GP (predict(node::GPNode), src/common.jl:175-179): no mixture term.
__device__ __forceinline__ void agg_mix_finish(double s0, double s1, double s2, int plain, double& mu, double& var) {
    mu = s0;
    var = plain ? s2 : s2 + (s1 - s0 * s0);                       // src/common.jl:299-300
}

// PoE / gPoE on (P, T); rBCM on (m, C) of its group steps
__device__ __forceinline__ void agg_prod_finish(double P, double T, double& mu, double& var) {
    mu = P / T;
    var = 1.0 / T;
}

// rBCM: s = k(x*, x*) + noise of the model's first leaf (leftGP, src/common.jl:227-228); C starts at 1 / s, m at 0, and every
// root child g adds its step.  The moments and the gradients were written apart and round beta and the child's share of m
// differently; both forms are kept as they were, here and in agg_rbcm_group_grad:
//   moments:   beta = (log s - log(1 / T)) / 2,  m += (P / T) (beta T)
//   gradients: beta = (log s + log T) / 2,       m += beta P,  C += beta (T - 1 / s)
__device__ __forceinline__ void agg_rbcm_group(double s, double P, double T, double& C, double& m) {
    if (T == 0.0) return;                                         // no leaf of this child saw the row
    const double M = P / T;                                       // mu_ of the child (:205)
    const double beta = 0.5 * (log(s) - log(1.0 / T));            // :234-235
    C += beta * T - beta / s;                                     // :236
    m += M * (beta * T);                                          // :237
}

// ---- the input gradients (the formulas: aggregate_input_gradients of the Python package, term by term) ----
// mixture: dvar' of an entry -- a clamped variance is a constant (a NaN one stays NaN).  The gradient is read only where it
// counts: loading it for every entry cost 7 % of agg_grad_partial_kernel and 30 % of agg_columns_grad_kernel on the headline model.
__device__ __forceinline__ double agg_mix_dvar(double v, const double* dvar) { return v <= 0.0 ? 0.0 : *dvar; }

// c = mu_l - the aggregated mean, so that a large offset of y cancels per term; dv = agg_mix_dvar
__device__ __forceinline__ void agg_mix_grad_term(double w, double c, double dm, double dv, double& s0, double& s1, double& s2) {
    s0 += w * dm;
    s1 += w * dv;
    s2 += w * (c * dm);
}

// dT = -sum b dvar / sigma^4, dP = sum b (dmu / sigma^2 - mu_l dvar / sigma^4); b as in agg_prod_term, but divided (b / v,
// where the moments multiply by 1 / v)
__device__ __forceinline__ void agg_prod_grad_term(double b, double m, double v, double dm, double dv, double& dT, double& dP) {
    const double t = b / v;
    dT -= (t / v) * dv;
    dP += t * dm - (t * m / v) * dv;
}

__device__ __forceinline__ void agg_mix_grad_finish(double s0, double s1, double s2, int plain, double& dmu, double& dvar) {
    dmu = s0;
    dvar = plain ? s1 : fma(2.0, s2, s1);
}

// PoE / gPoE on (P, T, dP, dT); rBCM on (m, C, dm, dC)
__device__ __forceinline__ void agg_prod_grad_finish(double P, double T, double dP, double dT, double& dmu, double& dvar) {
    const double mu = P / T;
    dmu = (dP - mu * dT) / T;
    dvar = -dT / (T * T);
}

// rBCM, gradients form (see agg_rbcm_group): N input dimensions at once; ds = ds/dx of the prior (prior_var_dx), ds_s2 = ds / s^2;
// dC starts at -ds_s2 and dm at 0
template <int N>
__device__ __forceinline__ void agg_rbcm_group_grad(double s, const double (&ds)[N], const double (&ds_s2)[N], double P, double T,
                                                    const double (&dP)[N], const double (&dT)[N], double& C, double& m,
                                                    double (&dC)[N], double (&dm)[N]) {
    if (T == 0.0) return;
    const double beta = 0.5 * (log(s) + log(T));
    C += beta * (T - 1.0 / s);
    m += beta * P;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const double dbeta = 0.5 * (ds[k] / s + dT[k] / T);
        // two products and a sum: written with the fma the compiler chose in both kernels that had these lines (the second product
        // fused, the first rounded), so that the rounding does not depend on where the rule is inlined
        dC[k] += fma(beta, dT[k] + ds_s2[k], dbeta * (T - 1.0 / s));
        dm[k] += fma(beta, dP[k], dbeta * P);
    }
}

// ---- the partial sums and their finish step ----
// One thread per test row; planes: mixture S0 | S1 | S2; PoE / gPoE P | T; rBCM P_g | T_g per root child g.
__global__ __launch_bounds__(256) void agg_partial_kernel(AggArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_t) return;
    double* part = a.out + r;
    const size_t n_t = a.n_t;
    if (a.family == AGG_MIXTURE) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) { agg_mix_term(a.coef[leaf], a.mu[pos], a.var[pos], s0, s1, s2); });
        part[0] = s0;
        part[n_t] = s1;
        part[2 * n_t] = s2;
    } else if (a.family == AGG_RBCM) {
        for (int g = 0; g < 2 * a.G; ++g) part[g * n_t] = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) {
            const size_t g = a.group[leaf];
            agg_prod_term(1.0, a.mu[pos], a.var[pos], part[2 * g * n_t], part[(2 * g + 1) * n_t]);
        });
    } else {
        double P = 0.0, T = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) { agg_prod_term(a.coef[leaf], a.mu[pos], a.var[pos], P, T); });
        part[0] = P;
        part[n_t] = T;
    }
}

// Finish step on the (summed) partial sums: mu / var of predict(model, x), left in HBM for agg_scores_kernel.
__global__ __launch_bounds__(256) void agg_finish_kernel(const double* __restrict__ part, int64_t n_t, int family, int G,
                                                         int plain, const KParam* __restrict__ kp, int prior_kid,
                                                         const double* __restrict__ Xt, int D,
                                                         double* __restrict__ mu_out, double* __restrict__ var_out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_t) return;
    if (family == AGG_MIXTURE) {
        agg_mix_finish(part[r], part[n_t + r], part[2 * n_t + r], plain, mu_out[r], var_out[r]);
    } else if (family == AGG_RBCM) {
        const KParam p = kp[prior_kid];
        const double s = prior_var(p, Xt, r, n_t, D) + p.noise;
        double C = 1.0 / s, m = 0.0;
        for (int g = 0; g < G; ++g) agg_rbcm_group(s, part[(size_t)(2 * g) * n_t + r], part[(size_t)(2 * g + 1) * n_t + r], C, m);
        agg_prod_finish(m, C, mu_out[r], var_out[r]);
    } else {
        agg_prod_finish(part[r], part[n_t + r], mu_out[r], var_out[r]);
    }
}

// Input gradients of the aggregated prediction (dsmgp_aggregate_gradients*): the same gather-reduce on dmu | dvar of every entry
// (pred_inputgrad_finish_kernel).  One thread per (test row, input dimension), blockIdx.y = d.  Partial sums in [k][row] planes,
// additive over contexts once every holder has the TOTAL moments (agg_mu is the aggregated mean of the finish step; T, P of the
// products are read by the finish step only):
//   mixture   k = d: sum W dmu_d;  D + d: sum W dvar'_d;  2 D + d: sum W (mu_l - mu) dmu_d
//   PoE/gPoE  k = d: dT_d;  D + d: dP_d
//   rBCM      k = 2 g D + d: dT_gd;  (2 g + 1) D + d: dP_gd, per root child g
__global__ __launch_bounds__(256) void agg_grad_partial_kernel(AggArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_t) return;
    const int d = blockIdx.y;
    const double* dmu = a.dmu + (size_t)d * a.ld;
    const double* dvar = a.dvar + (size_t)d * a.ld;
    const size_t Dn = (size_t)a.D * a.n_t;                      // planes k, D + k, ...: Dn apart
    double* part = a.out + (size_t)d * a.n_t + r;
    if (a.family == AGG_MIXTURE) {
        const double mbar = a.agg_mu[r];
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) {
            agg_mix_grad_term(a.coef[leaf], a.mu[pos] - mbar, dmu[pos], agg_mix_dvar(a.var[pos], dvar + pos), s0, s1, s2);
        });
        part[0] = s0;
        part[Dn] = s1;
        part[2 * Dn] = s2;
    } else if (a.family == AGG_RBCM) {
        for (int g = 0; g < 2 * a.G; ++g) part[g * Dn] = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) {
            const size_t g = a.group[leaf];
            agg_prod_grad_term(1.0, a.mu[pos], a.var[pos], dmu[pos], dvar[pos], part[2 * g * Dn], part[(2 * g + 1) * Dn]);
        });
    } else {
        double dT = 0.0, dP = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) {
            agg_prod_grad_term(a.coef[leaf], a.mu[pos], a.var[pos], dmu[pos], dvar[pos], dT, dP);
        });
        part[0] = dT;
        part[Dn] = dP;
    }
}

// Finish step on the (summed) gradient sums `gpart` and the total moment sums `part` of agg_finish_kernel.  One thread per
// (row, dimension); dmu_out / dvar_out are n_t x D planes.
__global__ __launch_bounds__(256) void agg_grad_finish_kernel(const double* __restrict__ gpart, const double* __restrict__ part,
                                                              int64_t n_t, int D, int family, int G, int plain,
                                                              const KParam* __restrict__ kp, int prior_kid,
                                                              const double* __restrict__ Xt, double* __restrict__ dmu_out,
                                                              double* __restrict__ dvar_out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_t) return;
    const int d = blockIdx.y;
    const size_t o = (size_t)d * n_t + r, Dn = (size_t)D * n_t;
    if (family == AGG_MIXTURE) {
        agg_mix_grad_finish(gpart[o], gpart[Dn + o], gpart[2 * Dn + o], plain, dmu_out[o], dvar_out[o]);
    } else if (family == AGG_RBCM) {
        const KParam p = kp[prior_kid];
        const double s = prior_var(p, Xt, r, n_t, D) + p.noise;
        const double ds[1] = {prior_var_dx(p, Xt[o], d)}, ds_s2[1] = {ds[0] / (s * s)};
        double C = 1.0 / s, m = 0.0, dC[1] = {-ds_s2[0]}, dm[1] = {0.0};
        for (int g = 0; g < G; ++g) {
            const double dT[1] = {gpart[(size_t)(2 * g) * Dn + o]}, dP[1] = {gpart[(size_t)(2 * g + 1) * Dn + o]};
            agg_rbcm_group_grad(s, ds, ds_s2, part[(size_t)(2 * g) * n_t + r], part[(size_t)(2 * g + 1) * n_t + r], dP, dT, C, m, dC,
                                dm);
        }
        agg_prod_grad_finish(m, C, dm[0], dC[0], dmu_out[o], dvar_out[o]);
    } else {
        agg_prod_grad_finish(part[r], part[n_t + r], gpart[Dn + o], gpart[o], dmu_out[o], dvar_out[o]);
    }
}

// The same aggregation for every resident target column (dsmgp_aggregate_columns, dsmgp_aggregate_columns_gradients): the leaf
// variance and its gradient are shared by the columns.  One thread per (test row, column), blockIdx.y = q, walks the row's
// entries and finishes in registers: no partial sums in memory, and column q never reads another column, so it is the same bits
// whatever Q is.  An rBCM row walks its entries once per group (the groups' sums in registers instead of G planes).
__global__ __launch_bounds__(256) void agg_columns_kernel(AggArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_t) return;
    const int q = blockIdx.y;
    const double* mu = a.mu + (size_t)q * a.ld;
    const size_t o = (size_t)q * a.n_t + r;
    if (a.family == AGG_MIXTURE) {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) { agg_mix_term(a.coef[leaf], mu[pos], a.var[pos], s0, s1, s2); });
        agg_mix_finish(s0, s1, s2, a.plain, a.out[o], a.out_v[o]);
    } else if (a.family == AGG_RBCM) {
        const KParam p = a.kp[a.prior_kid];
        const double s = prior_var(p, a.Xt, r, a.n_t, a.D) + p.noise;
        double C = 1.0 / s, m = 0.0;
        for (int g = 0; g < a.G; ++g) {
            double P = 0.0, T = 0.0;
            agg_walk(a.rows, r, [&](int pos, int leaf) {
                if (a.group[leaf] == g) agg_prod_term(1.0, mu[pos], a.var[pos], P, T);
            });
            agg_rbcm_group(s, P, T, C, m);
        }
        agg_prod_finish(m, C, a.out[o], a.out_v[o]);
    } else {
        double P = 0.0, T = 0.0;
        agg_walk(a.rows, r, [&](int pos, int leaf) { agg_prod_term(a.coef[leaf], mu[pos], a.var[pos], P, T); });
        agg_prod_finish(P, T, a.out[o], a.out_v[o]);
    }
}

// Gradients: chunks of AGG_DC input dimensions in registers, so that an entry's indices, coefficient, mu and var are read once
// per chunk and not once per dimension (once in all for D <= 8).  A chunk's dimensions past D hold zeros and are not stored.
constexpr int AGG_DC = 8;

__global__ __launch_bounds__(256) void agg_columns_grad_kernel(AggArgs a) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.n_t) return;
    const int q = blockIdx.y, D = a.D;
    const double* mu = a.mu + (size_t)q * a.ld;
    const double* dmq = a.dmu + (size_t)q * a.ld * D;
    double* om = a.out + (size_t)q * a.n_t * D + r;
    double* ov = a.out_v + (size_t)q * a.n_t * D + r;
    double mbar = 0.0;                                          // the aggregated mean: S0 as agg_mix_term sums it
    if (a.family == AGG_MIXTURE) agg_walk(a.rows, r, [&](int pos, int leaf) { mbar += a.coef[leaf] * mu[pos]; });
    for (int d0 = 0; d0 < D; d0 += AGG_DC) {
        const int nd = min(AGG_DC, D - d0);
        const auto ent = [&](int pos, int k) { return pos + (size_t)(d0 + k) * a.ld; };    // entry pos, dimension d0 + k
        const auto res = [&](int k) { return (size_t)(d0 + k) * a.n_t; };                  // its plane of the results
        if (a.family == AGG_MIXTURE) {
            double s0[AGG_DC] = {}, s1[AGG_DC] = {}, s2[AGG_DC] = {};
            // (the walk written out: through agg_walk's lambda this arm was scheduled otherwise -- 13 % faster than the loop at
            // Q = 1 and 25 % slower at Q = 64 on the depth-4 model -- and the speed of this kernel is to stay what it was)
            for (int64_t e = a.rows.row_ptr[r], e1 = a.rows.row_ptr[r + 1]; e < e1; ++e) {
                const int pos = a.rows.row_ent[e];
                const int leaf = a.rows.ent_leaf[pos];
                const double w = a.coef[leaf], c = mu[pos] - mbar, v = a.var[pos];
#pragma unroll
                for (int k = 0; k < AGG_DC; ++k)
                    if (k < nd)
                        agg_mix_grad_term(w, c, dmq[ent(pos, k)], agg_mix_dvar(v, a.dvar + ent(pos, k)), s0[k], s1[k], s2[k]);
            }
#pragma unroll
            for (int k = 0; k < AGG_DC; ++k)
                if (k < nd) agg_mix_grad_finish(s0[k], s1[k], s2[k], a.plain, om[res(k)], ov[res(k)]);
        } else if (a.family == AGG_RBCM) {
            const KParam p = a.kp[a.prior_kid];
            const double s = prior_var(p, a.Xt, r, a.n_t, D) + p.noise;
            double C = 1.0 / s, m = 0.0, ds[AGG_DC], ds_s2[AGG_DC], dC[AGG_DC], dm[AGG_DC];
#pragma unroll
            for (int k = 0; k < AGG_DC; ++k) {
                ds[k] = k < nd ? prior_var_dx(p, a.Xt[r + res(k)], d0 + k) : 0.0;
                ds_s2[k] = ds[k] / (s * s);
                dC[k] = -ds_s2[k];
                dm[k] = 0.0;
            }
            for (int g = 0; g < a.G; ++g) {
                double T = 0.0, P = 0.0, dT[AGG_DC] = {}, dP[AGG_DC] = {};
                agg_walk(a.rows, r, [&](int pos, int leaf) {
                    if (a.group[leaf] != g) return;
                    const double ml = mu[pos], v = a.var[pos];
                    agg_prod_term(1.0, ml, v, P, T);
#pragma unroll
                    for (int k = 0; k < AGG_DC; ++k)
                        if (k < nd)
                            agg_prod_grad_term(1.0, ml, v, dmq[ent(pos, k)], a.dvar[ent(pos, k)], dT[k], dP[k]);
                });
                agg_rbcm_group_grad(s, ds, ds_s2, P, T, dP, dT, C, m, dC, dm);
            }
#pragma unroll
            for (int k = 0; k < AGG_DC; ++k)
                if (k < nd) agg_prod_grad_finish(m, C, dm[k], dC[k], om[res(k)], ov[res(k)]);
        } else {
            double T = 0.0, P = 0.0, dT[AGG_DC] = {}, dP[AGG_DC] = {};
            agg_walk(a.rows, r, [&](int pos, int leaf) {
                // P, T as the moments form them (beta (1 / v)), the gradient terms as agg_grad_partial_kernel does (beta / v):
                // the two round differently, as in the two kernel pairs above
                const double b = a.coef[leaf], ml = mu[pos], v = a.var[pos];
                agg_prod_term(b, ml, v, P, T);
#pragma unroll
                for (int k = 0; k < AGG_DC; ++k)
                    if (k < nd)
                        agg_prod_grad_term(b, ml, v, dmq[ent(pos, k)], a.dvar[ent(pos, k)], dT[k], dP[k]);
            });
#pragma unroll
            for (int k = 0; k < AGG_DC; ++k)
                if (k < nd) agg_prod_grad_finish(P, T, dP[k], dT[k], om[res(k)], ov[res(k)]);
        }
    }
}

// Score sums (src/scorefunctions.jl:6-16) in two passes for the standard errors: pass 0 sums se, ae and the nlpd
// terms; pass 1 sums (se - mean se)^2 and (ae - mean ae)^2.  Per-block tree reduction, blocks combined in block order
// by the host: fixed summation order.
__global__ __launch_bounds__(256) void agg_scores_kernel(const double* __restrict__ y, const double* __restrict__ mu,
                                                         const double* __restrict__ var, int64_t n_t, int pass,
                                                         double mean_se, double mean_ae, double* __restrict__ out) {
    __shared__ double red[3][256];
    const int t = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * 256 + t;
    double a = 0.0, b = 0.0, c = 0.0;
    if (r < n_t) {
        const double d = y[r] - mu[r];
        const double se = d * d, ae = fabs(d);
        if (pass == 0) {
            a = se;
            b = ae;
            const double sd = sqrt(var[r]);                       // Normal(mu, sqrt(var)), :16
            const double zz = d / sd;
            c = 0.5 * (zz * zz + 1.8378770664093454835606594728112) + log(sd);
        } else {
            a = (se - mean_se) * (se - mean_se);
            b = (ae - mean_ae) * (ae - mean_ae);
        }
    }
    red[0][t] = a;
    red[1][t] = b;
    red[2][t] = c;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[0][t] += red[0][t + o];
            red[1][t] += red[1][t + o];
            red[2][t] += red[2][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[3 * (size_t)blockIdx.x] = red[0][0];
        out[3 * (size_t)blockIdx.x + 1] = red[1][0];
        out[3 * (size_t)blockIdx.x + 2] = red[2][0];
    }
}

}  // namespace dsmgp
