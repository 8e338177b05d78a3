// Joint posterior draws of every leaf GP over its routed test rows (dsmgp_predict_sample; not a call of the reference, whose
// posterior draws are a host product of prediction(gp, xtest), src/gaussianprocess.jl:110-137):
//   A_l = Sigma_l + jitter I,   C_l = chol(A_l),   out = mu + C_l E_l        per leaf l, E_l = the caller's normals of its entries.
// Three pieces of device work:
//   1. predsample_sigma_kernel: the lower tiles of Sigma_l of EVERY leaf in one launch, into the factor arena (ntpad_l^2 doubles per
//      leaf, cleared first).  The body is tile_predcov_kernel's (predcov_tile_body): the same values as dsmgp_predict_cov, bit for
//      bit, `jitter` more on the real diagonal, ones on the padded diagonal (the identity padding of the training factor), no
//      mirror above the block diagonal.
//   2. the blocked Cholesky, one round of launches per 128-column block step for all leaves that still have that step, left
//      looking: tile_gemm_kernel_v2 (block column k minus the product of the finished columns, the whole K range in one task: a
//      fixed order), chol_diag_packed_kernel (the diagonal tile, its inverse, and the first bad pivot with its absolute order in
//      the leaf's flag), tile_trsm_kernel (the tiles below against that inverse, with one step of refinement -- residual against
//      L_kk, its solve, the sum -- as three more launches of the same two kernels: Sigma + 1e-8 I is as ill-conditioned as the
//      jitter allows, and the product with an explicit inverse alone left 3.4e-15 of ||A|| where 4e-15 is the criterion).  The
//      tasks are plain TileTask / DiagTask without Gram epilogue, z or riders; nothing here is new device code.  A leaf whose
//      pivot fails goes on through its later steps on NaN / Inf data inside its own part of the arena: no trap, and no other leaf
//      reads it.
//   3. predsample_draw_kernel (below): out = mu + C E on the f64 matrix cores.
#pragma once
#include "kernels.hpp"

namespace dsmgp {

__global__ __launch_bounds__(256, 2) void predsample_sigma_kernel(const PredCovTask* __restrict__ tasks,
                                                                  const KParam* __restrict__ kp, int D, double jitter) {
    __shared__ __attribute__((aligned(16))) double smem[PREDCOV_LDS_DOUBLES];
    const PredCovTask g = tasks[blockIdx.x];
    predcov_tile_body<true>(g, kp, D, smem, jitter);
}

// One task = a 128-row tile of one leaf x a group of 16 draw columns.  E lives in a staging buffer of route_total rows and S
// rounded up to 16 columns (the columns past S are zero), the result in one of the same shape.  Wave w owns rows 32 w .. 32 w + 31
// of the tile, two 16 x 16 accumulators of v_mfma_f64_16x16x4_f64 (lane l supplies A[i = l & 15][k = l >> 4] = C and
// B[k = l >> 4][j = l & 15] = E, and receives D[(l >> 4) + 4 r][l & 15]).  The block columns j <= i of C are added in ascending
// order, each in ascending k, into the same accumulators: one fixed order, and a result column depends on its own column of E
// only -- column s is the same bits whatever S is and whatever the other columns hold.  The 128 x 16 tile of E of a block column
// goes through LDS (rows >= nt read as zero), C comes straight from memory (16 lanes = 16 consecutive rows = one 128-byte line;
// every element of the tile row is read once), the diagonal tile masked to its lower triangle on load.  Rows >= nt are neither
// read from E nor written.  A leaf whose flag is not zero gets NaN.
struct SampleDrawTask {
    const double* C;        // the leaf's factor, ntpad x ntpad (ld = ntpad)
    const double* eps;      // staged normals at (the leaf's first entry, the group's first column), ld = lde
    const double* mu;       // the leaf's means
    double* out;            // as eps
    const int* info;        // the leaf's flag
    long long lde;
    int ntpad, nt;
    int ti;                 // row tile
    int pad;
};
constexpr int SAMPLE_COLS = 16;

__global__ __launch_bounds__(256) void predsample_draw_kernel(const SampleDrawTask* __restrict__ tasks) {
    __shared__ __attribute__((aligned(16))) double sE[TB * SAMPLE_COLS];     // [k][column]
    const SampleDrawTask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const size_t ldc = (size_t)tk.ntpad;
    const int row0 = tk.ti * TB + 32 * w;       // first row of this wave
    d4 acc[2] = {{0.0, 0.0, 0.0, 0.0}, {0.0, 0.0, 0.0, 0.0}};
    for (int jt = 0; jt <= tk.ti; ++jt) {
        __syncthreads();        // the previous tile of E is no longer read
        {
            const int r = t & (TB - 1), c0 = (t >> 7) * (SAMPLE_COLS / 2);
            const int gr = jt * TB + r;
#pragma unroll
            for (int c = 0; c < SAMPLE_COLS / 2; ++c)
                sE[r * SAMPLE_COLS + c0 + c] = (gr < tk.nt) ? tk.eps[(size_t)gr + (size_t)(c0 + c) * (size_t)tk.lde] : 0.0;
        }
        __syncthreads();
        const bool diag = jt == tk.ti;
        const double* ca = tk.C + (size_t)(row0 + l15) + (size_t)(jt * TB + l4) * ldc;
#pragma unroll 2
        for (int kc = 0; kc < TB; kc += 16) {
            double a[4][2], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = kc + 4 * q + l4;       // column of the block column
                const double* col = ca + (size_t)(kc + 4 * q) * ldc;
                a[q][0] = col[0];
                a[q][1] = col[16];
                if (diag) {     // lower triangle of the diagonal tile only
                    const int rl = 32 * w + l15;
                    if (rl < k) a[q][0] = 0.0;
                    if (rl + 16 < k) a[q][1] = 0.0;
                }
                b[q] = sE[k * SAMPLE_COLS + l15];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][0], b[q], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[q][1], b[q], acc[1], 0, 0, 0);
            }
        }
    }
    const bool failed = *tk.info != 0;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
    for (int rn = 0; rn < 2; ++rn)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + 16 * rn + l4 + 4 * r;
            if (row < tk.nt) tk.out[(size_t)row + (size_t)l15 * (size_t)tk.lde] = failed ? nan : tk.mu[row] + acc[rn][r];
        }
}

}  // namespace dsmgp
