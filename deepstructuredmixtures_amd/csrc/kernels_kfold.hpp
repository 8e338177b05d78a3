// k-fold cross-validation of every leaf GP from one fit (dsmgp_kfold; not a call of the reference).  With G = K_y^-1 = Xt Xt^T
// (Xt = L^-T, the arena dsmgp_loo reads), alpha = G (y - m) and F the positions a fold holds out of a leaf, the leaf fitted
// without those rows -- mean and hyper-parameters as they are -- predicts them jointly as
//   mu_F = y_F - G_FF^-1 alpha_F,   Sigma_F = G_FF^-1,   lpd_F = -1/2 alpha_F^T G_FF^-1 alpha_F + 1/2 log det G_FF - (m / 2) log 2 pi
// (the multiple-fold residuals, e.g. Ginsbourger & Schaerer 2021; singletons are GPML 5.10-5.12, dsmgp_loo's formulas).
// Device work, per label round and then for all blocks together:
//   1. kfold_pack_kernel: the rows of a block out of the owner's Xt into a contiguous mpad x npad panel (zero padding rows, zero
//      left of the row's own 128-column block, where the arena holds nothing), so that the tuned main loop reads whole row tiles.
//   2. kfold_gff_kernel: lower tile (i, j) of G_FF = panel row tile i times row tile j on gemm_mainloop_v2, over the columns from
//      the 128-column block of tile i's first position on (left of it every product is zero) -- one task per tile over its whole
//      K range: a fixed order that depends on the block's rows only.  Zero outside the m valid rows and columns, ones on the padded
//      diagonal (the identity padding chol_diag_packed_kernel expects).
//   3. the blocked Cholesky C = chol(G_FF) of every block (chol_blocks in dsmgp_hip.cpp: the recipe of dsmgp_predict_sample).
//   4. with variances: Xc = C^-T by the blocked inversion that makes L^-T (transposed inverted diagonal blocks, a left-looking
//      sweep on tile_gemm_kernel_v2 / tile_trsm_kernel).
//   5. kfold_moments_kernel: one workgroup per (leaf, label): w = C^-1 alpha_F, v = C^-T w by blocked substitution (every factor
//      tile read once per sweep), mu = y - v, lpd = -1/2 |w|^2 + sum log C_ii - (m / 2) log 2 pi, var_i = |row i of Xc|^2.
#pragma once
#include "kernels.hpp"

namespace dsmgp {

struct KfoldPackTask {
    const double* X;        // the owner's Xt = L^-T, ld = ldx
    double* P;              // the block's panel at this tile's first row, ld = ldp (= mpad)
    const int32_t* pos;     // positions of the tile's rows inside the owner (nrows entries)
    int ldx, ldp;
    int nrows;              // rows of the tile that hold data
    int col0, col1;         // the task's columns: [col0, col1) within [128 * (first position / 128), npad)
};

__global__ __launch_bounds__(256) void kfold_pack_kernel(const KfoldPackTask* __restrict__ tasks) {
    const KfoldPackTask tk = tasks[blockIdx.x];
    const int r = threadIdx.x & (TB - 1), h = threadIdx.x >> 7;
    const int p = (r < tk.nrows) ? tk.pos[r] : -1;
    const int cstart = p & ~(TB - 1);       // the row's own 128-column block: Xt holds nothing left of it
    const double* src = tk.X + (p < 0 ? 0 : p);
    double* dst = tk.P + r;
    for (int c = tk.col0 + h; c < tk.col1; c += 2)
        dst[(size_t)c * tk.ldp] = (p >= 0 && c >= cstart) ? src[(size_t)c * tk.ldx] : 0.0;
}

struct KfoldGffTask {
    TileTask gemm;          // A = panel row tile i, B = panel row tile j <= i, K range [128 * (first position of tile i / 128), npad);
                            // C = tile (i, j) of the block's slot in the factor arena, ldc = mpad
    int na, nb;             // valid rows / columns
    int diag;
    int pad;
};

__global__ __launch_bounds__(256, 2) void kfold_gff_kernel(const KfoldGffTask* __restrict__ tasks) {
    __shared__ __attribute__((aligned(16))) double smem[2 * NRING * KC2 * LDP];
    double (*sA)[KC2 * LDP] = reinterpret_cast<double (*)[KC2 * LDP]>(smem);
    double (*sB)[KC2 * LDP] = reinterpret_cast<double (*)[KC2 * LDP]>(smem + NRING * KC2 * LDP);
    const KfoldGffTask g = tasks[blockIdx.x];
    d4 acc[4][4];
    gemm_mainloop_v2<false>(g.gemm, acc, sA, sB, nullptr);
    const int t = threadIdx.x;
    const int lane = t & 63, w = t >> 6;
    const int wr = w & 1, wc = w >> 1, l15 = lane & 15, l4 = lane >> 4;
    const size_t ldc = (size_t)g.gemm.ldc;
#pragma unroll
    for (int rn = 0; rn < 4; ++rn) {
        const int r = wr * 64 + 16 * rn + l15;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int c = wc * 64 + 16 * (i >> 2) + l4 + 4 * (i & 3);
            const double v = (r < g.na && c < g.nb) ? acc[i >> 2][rn][i & 3] : ((g.diag && r == c) ? 1.0 : 0.0);
            AS_GLOBAL_F64(g.gemm.C)[r + (size_t)c * ldc] = v;
        }
    }
}

struct KfoldMomTask {
    const double* C;        // chol(G_FF) of the owner's block, ld = mpad (lower; rows >= m are identity padding)
    const double* Xc;       // C^-T of the block, ld = mpad, or NULL: no variances
    const int32_t* pos;     // the block's m positions, ascending
    const double* alpha;    // the leaf's alpha, or its source's (COPY leaf with the same mean: LooTask's rule)
    const int* info;        // the block's flag: not zero = G_FF was not positive definite, NaN throughout
    double* work;           // 2 mpad doubles of the task's own: w | v
    double* lpd;            // the (leaf, label) slot
    long long off;          // the leaf's first entry in obs_idx = its first slot in mu / var
    int m, mpad;
};

__global__ __launch_bounds__(256) void kfold_moments_kernel(const KfoldMomTask* __restrict__ tasks, const int64_t* __restrict__ obs_idx,
                                                            const double* __restrict__ y, double* __restrict__ mu,
                                                            double* __restrict__ var) {
    __shared__ double rs[TB];
    __shared__ double part[256];
    const KfoldMomTask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, i = t & (TB - 1), h = t >> 7;
    const int lane = t & 63, wave = t >> 6;
    const int m = tk.m, nt = tk.mpad / TB;
    const size_t ld = (size_t)tk.mpad;
    double* w = tk.work;
    double* v = tk.work + tk.mpad;
    // forward: w = C^-1 alpha_F, row tile by row tile; the columns left of the tile in two halves, joined in a fixed order
    for (int tt = 0; tt < nt; ++tt) {
        const int row = tt * TB + i;
        const int c_lo = h ? tt * (TB / 2) : 0, c_hi = h ? tt * TB : tt * (TB / 2);
        double s = 0.0;
        for (int c = c_lo; c < c_hi; ++c) s += tk.C[row + (size_t)c * ld] * w[c];
        part[t] = s;
        __syncthreads();
        if (t < TB) rs[t] = ((row < m) ? tk.alpha[tk.pos[row]] : 0.0) - (part[t] + part[t + TB]);
        __syncthreads();
        const int nv = min(TB, m - tt * TB);
        const double* D = tk.C + (size_t)tt * TB + (size_t)tt * TB * ld;
        double mine = 0.0;
        for (int j = 0; j < nv; ++j) {      // column-oriented substitution inside the diagonal tile
            const double wj = rs[j] / D[j + (size_t)j * ld];
            if (t == j) mine = wj;          // (rs[j] itself is not written in step j: one barrier per column)
            if (t > j && t < nv) rs[t] -= D[t + (size_t)j * ld] * wj;
            __syncthreads();                // rs[j + 1] is final
        }
        if (t < TB) w[row] = mine;
        __syncthreads();
    }
    // backward: v = C^-T w.  Column c of the tiles below: a wave per column, lanes along the rows, butterfly sum (a fixed order)
    for (int tt = nt - 1; tt >= 0; --tt) {
        for (int q = 0; q < TB / 4; ++q) {
            const int cc = wave * (TB / 4) + q, col = tt * TB + cc;
            double p = 0.0;
            for (int r = (tt + 1) * TB + lane; r < m; r += 64) p += tk.C[r + (size_t)col * ld] * v[r];
            for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o);
            if (lane == 0) rs[cc] = w[col] - p;
        }
        __syncthreads();
        const int nv = min(TB, m - tt * TB);
        const double* D = tk.C + (size_t)tt * TB + (size_t)tt * TB * ld;
        double mine = 0.0;
        for (int j = nv - 1; j >= 0; --j) {
            const double vj = rs[j] / D[j + (size_t)j * ld];
            if (t == j) mine = vj;
            if (t < j) rs[t] -= D[j + (size_t)t * ld] * vj;
            __syncthreads();
        }
        if (t < TB) v[tt * TB + t] = mine;
        __syncthreads();
    }
    const bool bad = *tk.info != 0;
    const double qnan = __builtin_nan("");
    const double log2pi = 1.8378770664093454835606594728112;
    double s = 0.0;
    for (int r = t; r < m; r += 256) {
        const long long e = tk.off + tk.pos[r];
        mu[e] = bad ? qnan : y[obs_idx[e]] - v[r];
        s += log(tk.C[r + (size_t)r * ld]) - 0.5 * w[r] * w[r];
    }
    part[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) part[t] += part[t + o];
        __syncthreads();
    }
    if (t == 0) *tk.lpd = bad ? qnan : part[0] - 0.5 * (double)m * log2pi;
    if (tk.Xc == nullptr) return;
    // var_i = |row i of C^-T|^2 over the columns from the row's tile on (left of it the arena holds nothing), ascending, the
    // columns of a row in two halves
    for (int tt = 0; tt < nt; ++tt) {
        __syncthreads();
        const int row = tt * TB + i;
        const int c0 = tt * TB, mid = c0 + (m - c0 + 1) / 2;
        const int c_lo = h ? mid : c0, c_hi = h ? m : mid;
        double q = 0.0;
        if (row < m)
            for (int c = c_lo; c < c_hi; ++c) {
                const double x = tk.Xc[row + (size_t)c * ld];
                q += x * x;
            }
        part[t] = q;
        __syncthreads();
        if (t < TB && row < m) var[tk.off + tk.pos[row]] = bad ? qnan : part[t] + part[t + TB];
    }
}

}  // namespace dsmgp
