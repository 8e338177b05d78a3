// Several target columns on one factorisation (dsmgp_solve_targets / dsmgp_predict_targets): gather, multi-column forward
// substitution, per-(leaf, column) log-marginal and predictive means.  Nothing here writes what another entry point reads.
//
// Layout: every leaf has two npad x Qpad column-major blocks (ld = npad), Yc = Y[obs, :] - mean and Z = L^-1 Yc; Qpad = Q
// rounded up to 16, the N width of v_mfma_f64_16x16x4_f64.  Padding rows and padding columns are zero.
//
// Both tile kernels form their products as C^T = B^T A^T: the MFMA's first operand is the 16-column chunk of the targets
// (lane: column l15, k = l4), its second the factor / Vt rows (lane: row l15, k = l4), and register r of the result is
// (column l4 + 4 r, row l15) -- 16 consecutive rows per store.  An output column is a sum over its own target column only, in
// the k order of the instruction sequence: column j's bits do not depend on Q or on what the other columns hold.
#pragma once
#include "kernels.hpp"

namespace dsmgp {

constexpr int TQ = 16;          // target columns per MFMA chunk
constexpr int TLW = TB + 4;     // LDS leading dimension of the 16 x 128 block of W handed to the diagonal solve

// Yc[l] = Y[obs(l), :] - mean[l, :], zero in the padding rows and columns; one thread per row, columns in a loop
__global__ __launch_bounds__(256) void targets_gather_kernel(const LeafDev* __restrict__ leaves, const int64_t* __restrict__ obs_ptr,
                                                             const int64_t* __restrict__ obs_idx, const double* __restrict__ Y,
                                                             int64_t N, int Q, int qpad, const double* __restrict__ mean, int L,
                                                             double* __restrict__ arena, const long long* __restrict__ toff,
                                                             int leaf0) {
    const int l = leaf0 + blockIdx.y;
    const LeafDev lf = leaves[l];
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= lf.npad) return;
    const bool valid = r < lf.n;
    const int64_t g = valid ? obs_idx[obs_ptr[l] + r] : 0;
    double* yc = arena + toff[l];
    for (int q = 0; q < qpad; ++q)
        yc[r + (size_t)q * lf.npad] = (valid && q < Q) ? Y[g + (size_t)q * N] - mean[l + (size_t)q * L] : 0.0;
}

// One task of the right-looking sweep Z = L^-1 Yc, block step k of a leaf:
//   T != null:  W_i = src_i - L[i, k] Z_k   (src = Yc in step 0, Z afterwards: block i is read and written by this task alone)
//   Dinv != null (the task of i = k + 1, whose block is final after this update; and the leaf's first task, T == null, i = 0):
//               Z_i = Dinv_i W_i, lower triangle of Dinv_i only, instead of W_i
// so a launch per block step reads every factor tile of its block column once and the next launch finds Z_{k+1} ready.  The
// sums of a block run over k ascending, one task per (leaf, block, step): fixed order, no atomics, nothing depends on what
// else is in the launch.  Right-looking, not left-looking: step k of one leaf is nb - k - 1 independent tasks instead of one
// workgroup that walks a whole block row of the factor.
// Rows >= nrows of block i (padding of the leaf's last block) are masked on load -- factor rows, Dinv rows and columns -- and
// come out as zeros whatever the arenas hold there.
struct TargetsFwdTask {
    const double* T;        // L[i, k], ld = ldt; null: no update
    const double* Zk;       // Z block k (128 x qpad, ld = ldz)
    const double* src;      // block i of Yc or Z
    double* dst;            // block i of Z
    const double* Dinv;     // Dinv_i (ld 128) or null
    int ldt, ldz, qpad, nrows;
};

__global__ __launch_bounds__(256) void targets_fwd_kernel(const TargetsFwdTask* __restrict__ tasks) {
    __shared__ double sW[TQ * TLW];
    const TargetsFwdTask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const bool upd = tk.T != nullptr, solve = tk.Dinv != nullptr;
    // this wave's rows of the factor tile: (row = 32 w + 16 rn + l15, k = 4 kk + l4), read once for all column chunks
    double ft[2][32];
    if (upd) {
#pragma unroll
        for (int rn = 0; rn < 2; ++rn) {
            const int row = 32 * w + 16 * rn + l15;
            const double* p = tk.T + row + (size_t)l4 * tk.ldt;
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) ft[rn][kk] = row < tk.nrows ? p[(size_t)(4 * kk) * tk.ldt] : 0.0;
        }
    }
    for (int q0 = 0; q0 < tk.qpad; q0 += TQ) {
        d4 acc[2];
        acc[0] = (d4){0.0, 0.0, 0.0, 0.0};
        acc[1] = (d4){0.0, 0.0, 0.0, 0.0};
        if (upd) {
            const double* pz = tk.Zk + l4 + (size_t)(q0 + l15) * tk.ldz;      // (k = 4 kk + l4, column q0 + l15)
#pragma unroll
            for (int kk = 0; kk < 32; ++kk) {
                const double fz = pz[4 * kk];
                acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, ft[0][kk], acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, ft[1][kk], acc[1], 0, 0, 0);
            }
        }
        // register r of acc[rn]: (column q0 + l4 + 4 r, row 32 w + 16 rn + l15)
        double wv[2][4];
#pragma unroll
        for (int rn = 0; rn < 2; ++rn) {
            const int row = 32 * w + 16 * rn + l15;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const size_t at = (size_t)row + (size_t)(q0 + l4 + 4 * r) * tk.ldz;
                wv[rn][r] = row < tk.nrows ? tk.src[at] - acc[rn][r] : 0.0;
            }
        }
        if (!solve) {
#pragma unroll
            for (int rn = 0; rn < 2; ++rn)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    tk.dst[(size_t)(32 * w + 16 * rn + l15) + (size_t)(q0 + l4 + 4 * r) * tk.ldz] = wv[rn][r];
            continue;
        }
        // Z_i = Dinv_i W_i: the 16 x 128 block of W meets in LDS, wave w multiplies rows 32 w .. 32 w + 31 of Dinv_i over
        // k < 32 (w + 1) -- beyond that the triangle is empty
        __syncthreads();        // the block of the chunk before has been read
#pragma unroll
        for (int rn = 0; rn < 2; ++rn)
#pragma unroll
            for (int r = 0; r < 4; ++r) sW[(l4 + 4 * r) * TLW + 32 * w + 16 * rn + l15] = wv[rn][r];
        __syncthreads();
        d4 zz[2];
        zz[0] = (d4){0.0, 0.0, 0.0, 0.0};
        zz[1] = (d4){0.0, 0.0, 0.0, 0.0};
        const int kend = 8 * (w + 1);
        for (int kk = 0; kk < kend; ++kk) {
            const int k = 4 * kk + l4;
            const double fw = sW[l15 * TLW + k];
            double fd[2];
#pragma unroll
            for (int rn = 0; rn < 2; ++rn) {
                const int row = 32 * w + 16 * rn + l15;
                fd[rn] = (k <= row && row < tk.nrows) ? tk.Dinv[row + (size_t)k * TB] : 0.0;
            }
            zz[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fw, fd[0], zz[0], 0, 0, 0);
            zz[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fw, fd[1], zz[1], 0, 0, 0);
        }
#pragma unroll
        for (int rn = 0; rn < 2; ++rn)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                tk.dst[(size_t)(32 * w + 16 * rn + l15) + (size_t)(q0 + l4 + 4 * r) * tk.ldz] = zz[rn][r];
    }
}

// mll[l + j L] = -(|Z[:, j]|^2 + 2 sum log L_ii + n log 2pi) / 2, the sums and the tree of mll_kernel per (leaf, column);
// NaN for a leaf whose fit reported info != 0.  Grid (L, Q).
__global__ __launch_bounds__(256) void targets_mll_kernel(const LeafDev* __restrict__ leaves, const double* __restrict__ arena,
                                                          const long long* __restrict__ toff, int qpad, int L,
                                                          double* __restrict__ mll_out) {
    __shared__ double red[256];
    __shared__ double red2[256];
    const int l = blockIdx.x, j = blockIdx.y;
    const LeafDev lf = leaves[l];
    const double* z = arena + toff[l] + (size_t)lf.npad * qpad + (size_t)j * lf.npad;
    const int t = threadIdx.x;
    double s = 0.0, ld = 0.0;
    for (int i = t; i < lf.n; i += 256) {
        s = fma(z[i], z[i], s);
        ld += log(lf.F[i + (size_t)i * lf.npad]);
    }
    red[t] = s;
    red2[t] = ld;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            red[t] += red[t + o];
            red2[t] += red2[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double log2pi = 1.8378770664093454835606594728112;
        const double v = -(red[0] + 2.0 * red2[0] + log2pi * (double)lf.n) / 2.0;
        mll_out[l + (size_t)j * L] = *lf.info != 0 ? __builtin_nan("") : v;
    }
}

// mu[e, j] = mean[l, j] + sum_{c < n} Vt[e, c] Z[c, j] for a 128-row test tile of one leaf: wave w holds rows 32 w .. 32 w + 31
// and up to TMU_CH column chunks at a time, so Vt is read once per TMU_CH * 16 columns.
// The K_tn arena is not cleared: columns c >= n of Vt (and its rows >= nt) may hold anything, NaN included.  Columns c >= n are
// MASKED ON LOAD here (the operand is 0.0 there, and Z's padding rows are zeros), so they never reach a sum; rows >= nt do
// produce garbage, in their own output rows only, which are not stored.
constexpr int TMU_CH = 4;
struct TargetsMuTask {
    const double* Vt;       // row tile of Vt, ld = ldv
    const double* Z;        // npad x qpad, ld = ldz
    double* out;            // mu of this tile's first row, column 0 (ld = ldo)
    const int* info;
    long long ldo;
    int ldv, ldz, n, nrows, leaf, pad;
};

__global__ __launch_bounds__(256) void targets_mu_kernel(const TargetsMuTask* __restrict__ tasks, const double* __restrict__ mean,
                                                         int L, int Q, int qpad) {
    const TargetsMuTask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const bool failed = *tk.info != 0;
    const int nk = (tk.n + 3) / 4;
    for (int q0 = 0; q0 < qpad; q0 += TMU_CH * TQ) {
        const int nch = min(TMU_CH, (qpad - q0) / TQ);
        d4 acc[TMU_CH][2];
#pragma unroll
        for (int ch = 0; ch < TMU_CH; ++ch) {
            acc[ch][0] = (d4){0.0, 0.0, 0.0, 0.0};
            acc[ch][1] = (d4){0.0, 0.0, 0.0, 0.0};
        }
        const double* pv = tk.Vt + 32 * w + l15;
        const double* pz = tk.Z + (size_t)(q0 + l15) * tk.ldz;
        for (int kk = 0; kk < nk; ++kk) {
            const int c = 4 * kk + l4;
            const bool in = c < tk.n;
            const double v0 = in ? pv[(size_t)c * tk.ldv] : 0.0;
            const double v1 = in ? pv[(size_t)c * tk.ldv + 16] : 0.0;
#pragma unroll
            for (int ch = 0; ch < TMU_CH; ++ch) {
                if (ch >= nch) continue;
                const double fz = in ? pz[c + (size_t)(ch * TQ) * tk.ldz] : 0.0;
                acc[ch][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, v0, acc[ch][0], 0, 0, 0);
                acc[ch][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, v1, acc[ch][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ch = 0; ch < TMU_CH; ++ch) {
            if (ch >= nch) continue;
#pragma unroll
            for (int rn = 0; rn < 2; ++rn) {
                const int row = 32 * w + 16 * rn + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = q0 + ch * TQ + l4 + 4 * r;
                    if (row < tk.nrows && q < Q)
                        tk.out[(size_t)row + (size_t)q * tk.ldo] =
                            failed ? __builtin_nan("") : mean[tk.leaf + (size_t)q * L] + acc[ch][rn][r];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Hyper-parameter gradients of sum_q w_lq mll_lq (dsmgp_mll_columns_gradients).  With A = L^-T Z = K_y^-1 (Y - m), G = K_y^-1 and
// s_l = sum_q w_lq:   sum_q w_lq dmll_lq / dtheta = 1/2 sum_rc (sum_q w_lq a_rq a_cq - s_l G_rc) (dK_y / dtheta)_rc.
//   targets_a_kernel        A of every leaf into an arena of its own (npad x Qpad per leaf, ld = npad)
//   tile_graddot_*<GD_TARGETS>   the contraction, G never stored and the rank-Q term added to the accumulators (kernels.hpp)
//   targets_wsums_kernel    sum_q w_lq |z_q|^2 and sum_q w_lq |a_q|^2 per leaf (the trace identity and dnoise)
//   targets_ardlin_kernel   ArdLinear leaves: sum_q w_lq (a_q . x_d)^2

// A_i = sum_{k >= i} Xt[i, k] Z_k for one 128-row block i of a leaf, Xt = L^-T of the leaf's factor owner: row tile i of the
// arena from column 128 i on (the blocks left of the diagonal are never written and never read here).  Operands as in
// targets_mu_kernel: column j of A is a sum over column j of Z only, in ascending k.  Columns c >= n of Xt are masked on load
// and rows >= nrows are stored as zeros, whatever the arena's padding holds; all Qpad columns are written.
struct TargetsATask {
    const double* Xt;       // row tile i of the owner's L^-T, ld = ldt
    const double* Z;        // the leaf's Z (npad x qpad, ld = ldz)
    double* A;              // block i of the leaf's A (ld = ldz)
    int ldt, ldz, k0, n, nrows, pad;
};

__global__ __launch_bounds__(256) void targets_a_kernel(const TargetsATask* __restrict__ tasks, int qpad) {
    const TargetsATask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int nk = (tk.n - tk.k0 + 3) / 4;
    for (int q0 = 0; q0 < qpad; q0 += TMU_CH * TQ) {
        const int nch = min(TMU_CH, (qpad - q0) / TQ);
        d4 acc[TMU_CH][2];
#pragma unroll
        for (int ch = 0; ch < TMU_CH; ++ch) {
            acc[ch][0] = (d4){0.0, 0.0, 0.0, 0.0};
            acc[ch][1] = (d4){0.0, 0.0, 0.0, 0.0};
        }
        const double* pv = tk.Xt + 32 * w + l15;
        const double* pz = tk.Z + (size_t)(q0 + l15) * tk.ldz;
        for (int kk = 0; kk < nk; ++kk) {
            const int c = tk.k0 + 4 * kk + l4;
            const bool in = c < tk.n;
            const int r0 = tk.k0 + 32 * w + l15;        // L^-T is upper triangular: (row, c) enters for row <= c only
            const double v0 = (in && r0 <= c) ? pv[(size_t)c * tk.ldt] : 0.0;
            const double v1 = (in && r0 + 16 <= c) ? pv[(size_t)c * tk.ldt + 16] : 0.0;
#pragma unroll
            for (int ch = 0; ch < TMU_CH; ++ch) {
                if (ch >= nch) continue;
                const double fz = in ? pz[c + (size_t)(ch * TQ) * tk.ldz] : 0.0;
                acc[ch][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, v0, acc[ch][0], 0, 0, 0);
                acc[ch][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, v1, acc[ch][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ch = 0; ch < TMU_CH; ++ch) {
            if (ch >= nch) continue;
#pragma unroll
            for (int rn = 0; rn < 2; ++rn) {
                const int row = 32 * w + 16 * rn + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = q0 + ch * TQ + l4 + 4 * r;
                    tk.A[(size_t)row + (size_t)q * tk.ldz] = row < tk.nrows ? acc[ch][rn][r] : 0.0;
                }
            }
        }
    }
}

// out[2 l] = sum_q w_lq |z_q|^2, out[2 l + 1] = sum_q w_lq |a_q|^2: thread t adds the rows t, t + 256, ..., each row's columns in
// ascending q, then the tree of mll_kernel -- a fixed order.  One workgroup per leaf.
__global__ __launch_bounds__(256) void targets_wsums_kernel(const LeafDev* __restrict__ leaves, const double* __restrict__ arenaT,
                                                            const long long* __restrict__ toff, const double* __restrict__ arenaA,
                                                            const double* __restrict__ wq, int L, int Q, int qpad,
                                                            double* __restrict__ out) {
    __shared__ double r1[256], r2[256];
    const int l = blockIdx.x;
    const LeafDev lf = leaves[l];
    const double* z = arenaT + toff[l] + (size_t)lf.npad * qpad;
    const double* a = arenaA + toff[l] / 2;
    const int t = threadIdx.x;
    double sz = 0.0, sa = 0.0;
    for (int i = t; i < lf.n; i += 256)
        for (int q = 0; q < Q; ++q) {
            const double wv = wq[l + (size_t)q * L];
            const double zv = z[i + (size_t)q * lf.npad], av = a[i + (size_t)q * lf.npad];
            sz = fma(wv * zv, zv, sz);
            sa = fma(wv * av, av, sa);
        }
    r1[t] = sz;
    r2[t] = sa;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            r1[t] += r1[t + o];
            r2[t] += r2[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * l] = r1[0];
        out[2 * l + 1] = r2[0];
    }
}

// ArdLinear leaves: out[task * D + d] = sum_q w_q (a_q . x_d)^2, one workgroup per (task, d).  Wave w takes the columns
// q = w, w + 4, ...: the dot product over the lanes (fixed butterfly), the columns of a wave added in ascending q, the four
// waves in order.
struct TargetsArdLinTask {
    const double* A;        // the leaf's A (ld = ld)
    const double* x;        // the leaf's inputs (ld = ld)
    const double* wq;       // weight of column q at wq[q * ldw]
    int ld, ldw, n, Q;
};

__global__ __launch_bounds__(256) void targets_ardlin_kernel(const TargetsArdLinTask* __restrict__ tasks, int D,
                                                             double* __restrict__ out) {
    __shared__ double red[4];
    const TargetsArdLinTask tk = tasks[blockIdx.x];
    const int d = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const double* x = tk.x + (size_t)d * tk.ld;
    double s = 0.0;
    for (int q = w; q < tk.Q; q += 4) {
        const double* a = tk.A + (size_t)q * tk.ld;
        double dot = 0.0;
        for (int i = lane; i < tk.n; i += 64) dot = fma(a[i], x[i], dot);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
        s = fma(tk.wq[(size_t)q * tk.ldw] * dot, dot, s);
    }
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (t == 0) out[(size_t)blockIdx.x * D + d] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------
// Leave-one-out moments and gradients of the target columns (dsmgp_loo_columns, dsmgp_loo_columns_gradients; GPML eqs. 5.10-5.13
// per column, summed with weights c_q >= 0).  With G = K_y^-1, d = diag G (the row sums of dsmgp_loo), a_q column q of A:
//   mu_iq = y_iq - a_iq / d_i,  var_i = 1 / d_i,  lpd_q = sum_i -(log 2pi - log d_i + a_iq^2 / d_i) / 2
//   sum_q c_q dlpd_q / dtheta = sum_rc M_rc (dK_y / dtheta)_rc,  M = sum_q c_q (u_q a_q^T + a_q u_q^T) / 2 - H H^T,
//   u_q = G (a_q / d),  H = G diag(sqrt W),  W_i = (s + sum_q c_q a_iq^2 / d_i) / (2 d_i),  s = sum_q c_q:
// the diagonal weight of G diag(w_q) G is linear in the column, so ONE H serves every column.
//   loo_columns_moments_kernel   the moments and the lpd table, one workgroup per (leaf, column)
//   loo_columns_weights_kernel   per leaf [d | sqrt W | 1 / (d sqrt W)] and the two sums of tr(M K_y)
//   tile_ginv_kernel             H, as dsmgp_loo_gradients forms it, with sqrt W in place of sqrt w
//   loo_columns_u_kernel         U = H (A / (d sqrt W)) per 128-row tile on the f64 MFMA
//   loo_columns_rowsums_kernel   |H|_F^2 and sum_q c_q u_q . a_q per row tile (tr M)
//   tile_graddot_*<GD_LOO_COLUMNS>   the contraction (kernels.hpp)
//   loo_columns_ardlin_kernel, ardlin_quad_kernel<true>   ArdLinear: sum_q c_q (x_d . u_q)(x_d . a_q) and |H^T x_d|^2
// The row sums of the factor owner and the leaf's place in obs_idx come from dsmgp_loo's own list (LooTask: P, ldp, off).
struct LooColsTask {
    const double* A;        // the leaf's A (npad x qpad, ld = npad)
    double* vec;            // [d | sqrt W | 1 / (d sqrt W)], 3 npad doubles, zero from row n on; null: no gradient work for this leaf
    const double* wq;       // weight of column q at wq[q * ldw]
    double s;               // sum_q c_q
    int npad, ldw, Q, pad;
};

// d_i as loo_moments_kernel adds it: the slices of the row in ascending column order
__device__ __forceinline__ double loo_columns_d(const LooTask& tk, int n, int i) {
    const int nparts = (n - (i & ~(TB - 1)) + ROWNORM_COLS - 1) / ROWNORM_COLS;
    double d = 0.0;
    for (int k = 0; k < nparts; ++k) d += tk.P[(size_t)k * tk.ldp + i];
    return d;
}

// Grid (L, Q).  mu (may be null) is nobs x Q with leading dimension ldmu, var (may be null) nobs long and written by column 0;
// lpd[l + q L].  The sum of a column: thread t adds rows t, t + 256, ..., then the tree of mll_kernel.  A column's results read
// that column of A and Y only.  NaN for a leaf whose fit failed.
__global__ __launch_bounds__(256) void loo_columns_moments_kernel(const LeafDev* __restrict__ leaves, const LooTask* __restrict__ loo,
                                                                  const LooColsTask* __restrict__ tasks,
                                                                  const int64_t* __restrict__ obs_idx, const double* __restrict__ Y,
                                                                  int64_t N, int L, double* __restrict__ mu, long long ldmu,
                                                                  double* __restrict__ var, double* __restrict__ lpd) {
    __shared__ double red[256];
    const int l = blockIdx.x, q = blockIdx.y;
    const LeafDev lf = leaves[l];
    const LooColsTask tk = tasks[l];
    const LooTask lt = loo[l];
    const int t = threadIdx.x;
    const bool bad = *lf.info != 0;
    const double log2pi = 1.8378770664093454835606594728112;
    const double qnan = __builtin_nan("");
    const double* a_q = tk.A + (size_t)q * tk.npad;
    double s = 0.0;
    for (int i = t; i < lf.n; i += 256) {
        const double d = loo_columns_d(lt, lf.n, i);
        const double a = a_q[i];
        const double r = a / d;
        if (mu) mu[lt.off + i + (size_t)q * ldmu] = bad ? qnan : Y[obs_idx[lt.off + i] + (size_t)q * N] - r;
        if (var && q == 0) var[lt.off + i] = bad ? qnan : 1.0 / d;
        s += -0.5 * ((log2pi - log(d)) + a * r);
    }
    red[t] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) lpd[l + (size_t)q * L] = bad ? qnan : red[0];
}

// out[2 l] = sum_i sum_q c_q a_iq^2 / d_i, out[2 l + 1] = sum_i W_i d_i: a row's columns in ascending q, thread t adds rows
// t, t + 256, ..., then a fixed tree.  One workgroup per leaf.
__global__ __launch_bounds__(256) void loo_columns_weights_kernel(const LeafDev* __restrict__ leaves, const LooTask* __restrict__ loo,
                                                                  const LooColsTask* __restrict__ tasks, double* __restrict__ out) {
    __shared__ double r1[256], r2[256];
    const LooColsTask tk = tasks[blockIdx.x];
    if (!tk.vec) return;
    const LooTask lt = loo[blockIdx.x];
    const LeafDev lf = leaves[blockIdx.x];
    const int t = threadIdx.x;
    const size_t np = (size_t)tk.npad;
    double s1 = 0.0, s2 = 0.0;
    for (int i = t; i < tk.npad; i += 256) {
        double d = 0.0, sw = 0.0, tq = 0.0;
        if (i < lf.n) {
            d = loo_columns_d(lt, lf.n, i);
            double S = 0.0;
            for (int q = 0; q < tk.Q; ++q) {
                const double a = tk.A[i + (size_t)q * np];
                S = fma(tk.wq[(size_t)q * tk.ldw] * a, a / d, S);
            }
            const double W = (tk.s + S) / (2.0 * d);
            sw = sqrt(W);
            tq = 1.0 / (d * sw);
            s1 += S;
            s2 = fma(W, d, s2);
        }
        tk.vec[i] = d;
        tk.vec[np + i] = sw;
        tk.vec[2 * np + i] = tq;
    }
    r1[t] = s1;
    r2[t] = s2;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            r1[t] += r1[t + o];
            r2[t] += r2[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * blockIdx.x] = r1[0];
        out[2 * blockIdx.x + 1] = r2[0];
    }
}

// U_i = sum_{c < n} H[i, c] (A[c, :] tq_c) for one 128-row block i of a leaf: targets_a_kernel on a full square (H is stored
// whole, nothing is triangular) with the scale 1 / (d_c sqrt W_c) folded into the column operand on load, so A / (d sqrt W) is
// never stored.  Columns c >= n are masked on load and rows >= nrows stored as zeros; all Qpad columns are written.
struct LooColsUTask {
    const double* H;        // row tile i of the leaf's H, ld = ld
    const double* A;        // the leaf's A (ld = ld)
    const double* tq;       // 1 / (d sqrt W), n entries
    double* U;              // block i of the leaf's U (ld = ld)
    int ld, n, nrows, pad;
};

__global__ __launch_bounds__(256) void loo_columns_u_kernel(const LooColsUTask* __restrict__ tasks, int qpad) {
    const LooColsUTask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int nk = (tk.n + 3) / 4;
    for (int q0 = 0; q0 < qpad; q0 += TMU_CH * TQ) {
        const int nch = min(TMU_CH, (qpad - q0) / TQ);
        d4 acc[TMU_CH][2];
#pragma unroll
        for (int ch = 0; ch < TMU_CH; ++ch) {
            acc[ch][0] = (d4){0.0, 0.0, 0.0, 0.0};
            acc[ch][1] = (d4){0.0, 0.0, 0.0, 0.0};
        }
        const double* pv = tk.H + 32 * w + l15;
        const double* pz = tk.A + (size_t)(q0 + l15) * tk.ld;
        for (int kk = 0; kk < nk; ++kk) {
            const int c = 4 * kk + l4;
            const bool in = c < tk.n;
            const double v0 = in ? pv[(size_t)c * tk.ld] : 0.0;
            const double v1 = in ? pv[(size_t)c * tk.ld + 16] : 0.0;
            const double sc = in ? tk.tq[c] : 0.0;
#pragma unroll
            for (int ch = 0; ch < TMU_CH; ++ch) {
                if (ch >= nch) continue;
                const double fz = in ? pz[c + (size_t)(ch * TQ) * tk.ld] * sc : 0.0;
                acc[ch][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, v0, acc[ch][0], 0, 0, 0);
                acc[ch][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(fz, v1, acc[ch][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ch = 0; ch < TMU_CH; ++ch) {
            if (ch >= nch) continue;
#pragma unroll
            for (int rn = 0; rn < 2; ++rn) {
                const int row = 32 * w + 16 * rn + l15;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int q = q0 + ch * TQ + l4 + 4 * r;
                    tk.U[(size_t)row + (size_t)q * tk.ld] = row < tk.nrows ? acc[ch][rn][r] : 0.0;
                }
            }
        }
    }
}

// One 128-row tile of a leaf: out[2 task] = sum_r sum_{c < n} H(r, c)^2 (the column halves and partial sums of loo_hvec_kernel),
// out[2 task + 1] = sum_r sum_q c_q U(r, q) A(r, q) (half h of the workgroup takes q = h, h + 2, ...), both through a fixed tree.
struct LooColsRowTask {
    const double* H;        // the leaf's H (ld = ld)
    const double* A;        // the leaf's A and U (ld = ld)
    const double* U;
    const double* wq;
    int ld, ldw, n, Q, row0, nrows;
};

__global__ __launch_bounds__(256) void loo_columns_rowsums_kernel(const LooColsRowTask* __restrict__ tasks, double* __restrict__ out) {
    __shared__ double ru[256], rf[256];
    const LooColsRowTask tk = tasks[blockIdx.x];
    const int t = threadIdx.x, r = t & 127, h = t >> 7;
    double su = 0.0, sf[4] = {0.0, 0.0, 0.0, 0.0};
    if (r < tk.nrows) {
        const double* Hr = tk.H + tk.row0 + r;
        for (int c = h; c < tk.n; c += 8) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (c + 2 * j < tk.n) {
                    const double v = Hr[(size_t)(c + 2 * j) * tk.ld];
                    sf[j] = fma(v, v, sf[j]);
                }
        }
        for (int q = h; q < tk.Q; q += 2) {
            const size_t at = (size_t)tk.row0 + r + (size_t)q * tk.ld;
            su = fma(tk.wq[(size_t)q * tk.ldw] * tk.U[at], tk.A[at], su);
        }
    }
    ru[t] = su;
    rf[t] = (sf[0] + sf[1]) + (sf[2] + sf[3]);
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            ru[t] += ru[t + o];
            rf[t] += rf[t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        out[2 * blockIdx.x] = rf[0];
        out[2 * blockIdx.x + 1] = ru[0];
    }
}

// ArdLinear leaves: out[task * D + d] = sum_q c_q (u_q . x_d)(a_q . x_d), one workgroup per (task, d), the order of
// targets_ardlin_kernel: wave w takes q = w, w + 4, ..., dot products over the lanes by a fixed butterfly, the waves in order.
struct LooColsArdLinTask {
    const double* A;        // the leaf's A and U (ld = ld)
    const double* U;
    const double* x;        // the leaf's inputs (ld = ld)
    const double* wq;
    int ld, ldw, n, Q;
};

__global__ __launch_bounds__(256) void loo_columns_ardlin_kernel(const LooColsArdLinTask* __restrict__ tasks, int D,
                                                                 double* __restrict__ out) {
    __shared__ double red[4];
    const LooColsArdLinTask tk = tasks[blockIdx.x];
    const int d = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const double* x = tk.x + (size_t)d * tk.ld;
    double s = 0.0;
    for (int q = w; q < tk.Q; q += 4) {
        const double* a = tk.A + (size_t)q * tk.ld;
        const double* u = tk.U + (size_t)q * tk.ld;
        double da = 0.0, du = 0.0;
        for (int i = lane; i < tk.n; i += 64) {
            da = fma(a[i], x[i], da);
            du = fma(u[i], x[i], du);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            da += __shfl_xor(da, o, 64);
            du += __shfl_xor(du, o, 64);
        }
        s = fma(tk.wq[(size_t)q * tk.ldw] * du, da, s);
    }
    if (lane == 0) red[w] = s;
    __syncthreads();
    if (t == 0) out[(size_t)blockIdx.x * D + d] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------------------------------------
// Input gradients of the predictive means of the target columns (dsmgp_predict_columns_gradients): for every (leaf, routed test
// row t), dimension d and column q
//   dmu[t, d, q] = sum_{i < n} A[i, q] g_d(t, i),   g_d(t, i) = dk(x_t, x_i) / dx_{t,d},   A = K_y^-1 (Y - m) (targets_a_kernel),
// the per-kind derivatives of pred_inputgrad_kernel (kernels.hpp), built from the same helpers.  For Q columns this is the matrix
// product G_d A per dimension, on the f64 matrix cores with the operands of targets_mu_kernel: the 16-column chunk of A is the
// first operand (lane: column l15, k = l4), g_d(test row 32 w + l15 (+ 16), training row c0 + 4 kk + l4) the second, and the
// lane that needs an entry of G_d computes it in registers -- G_d is never stored.  Within a wave every (test row, training row)
// pair of a K-slice belongs to exactly one lane, so for the kinds whose derivative carries the kernel value (IsoSE, ArdSEProduct,
// Matern, RQ) the pair factor -- the exponent summed over ALL D dimensions, then exp_nonpos / rq_value -- is evaluated once and
// serves the TIG_DC dimensions of the chunk and the TIG_CH 16-column chunks held in accumulators (TIG_DC x TIG_CH x 2 MFMAs per
// two factors).
// One task = a 128-row test tile of one leaf x a slab of TIG_SLAB training rows; its sums go to planes of its own (plane
// d * qpad + q, 128 rows), which targets_inputgrad_finish_kernel adds in ascending slab order: no atomics, and column q is a sum
// over column q of A only, in an order that depends on constants alone -- the same bits whatever Q is and whatever the other
// columns hold, and the same for a test row wherever it stands in a tile.
// Training rows c >= c1 (<= n) are MASKED ON LOAD: both operands are 0.0 there, whatever the padding of Xg and A holds.  Rows
// >= nrows of the test tile compute on zeros and are not stored.
constexpr int TIG_SLAB = 1024;      // training rows per task
constexpr int TIG_DC = PGRAD_DC;    // dimensions per chunk
constexpr int TIG_CH = 2;           // 16-column chunks of A per pass: TIG_DC x TIG_CH x 2 accumulators of 4 doubles per lane

struct TargetsInputGradTask {
    const double* xt;       // gathered test inputs, offset to the tile's first row (ld = ldt)
    const double* xg;       // gathered training inputs of the leaf (ld = ldg)
    const double* A;        // the leaf's A (npad x qpad, ld = ldg)
    double* part;           // this task's sums: plane d * qpad + q, 128 rows each
    int ldt, ldg;
    int nrows;              // valid test rows of the tile
    int c0, c1;             // training rows [c0, c1), c1 <= n
    int kid;
};

template <int KIND>
__device__ __forceinline__ void targets_inputgrad_body(const TargetsInputGradTask& tk, const KParam& p, int D, int qpad) {
    constexpr int DC = TIG_DC;
    constexpr bool PAIR = (KIND == 0 || KIND == 4 || KIND == 5 || KIND == 6);   // the derivative carries the kernel value of the pair
    const int t = threadIdx.x, lane = t & 63;
    const int w = __builtin_amdgcn_readfirstlane(t >> 6);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int r0 = 32 * w + l15, r1 = r0 + 16;
    const bool live0 = r0 < tk.nrows, live1 = r1 < tk.nrows;
    const double c2 = (KIND == 5) ? matern_c2(p) : 0.0;
    const double c1 = (c2 != 0.0) ? c2 : 1.0;
    const int nk = (tk.c1 - tk.c0 + 3) / 4;
    const bool one_round = D <= DC;
    // the pair factor from the exponent's sum
    auto factor = [&](double f) {
        if (KIND == 0) return -(p.sigma2 * exp_nonpos(f * p.nh0)) * p.il2;
        if (KIND == 4) return p.sigma2 * exp_nonpos(f);
        if (KIND == 6) return -(rq_value(f, p) / (1.0 + f)) * (2.0 * rq_alpha(p));
        const double s = sqrt(f);
        return -(p.sigma2 * exp_nonpos(-s) * fma(c2, s, c1));
    };
    for (int e0 = 0; e0 < D; e0 += DC) {
        const int en = min(DC, D - e0);
        double xa0[DC], xa1[DC], nhd[DC];
#pragma unroll
        for (int d = 0; d < DC; ++d) {
            xa0[d] = (live0 && d < en) ? tk.xt[r0 + (size_t)(e0 + d) * tk.ldt] : 0.0;
            xa1[d] = (live1 && d < en) ? tk.xt[r1 + (size_t)(e0 + d) * tk.ldt] : 0.0;
            nhd[d] = (kind_reads_nh(KIND) && d < en) ? p.nh[e0 + d] : 0.0;
        }
        for (int q0 = 0; q0 < qpad; q0 += TIG_CH * TQ) {
            const int nch = min(TIG_CH, (qpad - q0) / TQ);
            d4 acc[DC][TIG_CH][2];
#pragma unroll
            for (int d = 0; d < DC; ++d)
#pragma unroll
                for (int ch = 0; ch < TIG_CH; ++ch) {
                    acc[d][ch][0] = (d4){0.0, 0.0, 0.0, 0.0};
                    acc[d][ch][1] = (d4){0.0, 0.0, 0.0, 0.0};
                }
            const double* pa = tk.A + (size_t)(q0 + l15) * tk.ldg;
            for (int kk = 0; kk < nk; ++kk) {
                const int c = tk.c0 + 4 * kk + l4;
                const bool in = c < tk.c1;
                double xc[DC], av[TIG_CH];
#pragma unroll
                for (int d = 0; d < DC; ++d) xc[d] = (in && d < en) ? tk.xg[c + (size_t)(e0 + d) * tk.ldg] : 0.0;
#pragma unroll
                for (int ch = 0; ch < TIG_CH; ++ch) av[ch] = (in && ch < nch) ? pa[c + (size_t)(ch * TQ) * tk.ldg] : 0.0;
                double f0 = 0.0, f1 = 0.0;
                if (PAIR) {
                    if (one_round) {
#pragma unroll
                        for (int d = 0; d < DC; ++d)
                            if (d < en) {
                                const double u0 = xa0[d] - xc[d], u1 = xa1[d] - xc[d];
                                f0 = (KIND == 0) ? fma(u0, u0, f0) : fma(u0 * u0, nhd[d], f0);
                                f1 = (KIND == 0) ? fma(u1, u1, f1) : fma(u1 * u1, nhd[d], f1);
                            }
                    } else {
                        for (int d = 0; d < D; ++d) {
                            const double b = in ? tk.xg[c + (size_t)d * tk.ldg] : 0.0;
                            const double u0 = (live0 ? tk.xt[r0 + (size_t)d * tk.ldt] : 0.0) - b;
                            const double u1 = (live1 ? tk.xt[r1 + (size_t)d * tk.ldt] : 0.0) - b;
                            const double h = (KIND == 0) ? 0.0 : p.nh[d];
                            f0 = (KIND == 0) ? fma(u0, u0, f0) : fma(u0 * u0, h, f0);
                            f1 = (KIND == 0) ? fma(u1, u1, f1) : fma(u1 * u1, h, f1);
                        }
                    }
                    f0 = factor(f0);
                    f1 = factor(f1);
                }
#pragma unroll
                for (int d = 0; d < DC; ++d)
                    if (d < en) {
                        double g0, g1;
                        if (KIND == 0) {
                            g0 = f0 * (xa0[d] - xc[d]);
                            g1 = f1 * (xa1[d] - xc[d]);
                        } else if (KIND == 4) {
                            g0 = f0 * ((xa0[d] - xc[d]) * (2.0 * nhd[d]));
                            g1 = f1 * ((xa1[d] - xc[d]) * (2.0 * nhd[d]));
                        } else if (KIND == 5 || KIND == 6) {
                            g0 = f0 * ((xa0[d] - xc[d]) * nhd[d]);
                            g1 = f1 * ((xa1[d] - xc[d]) * nhd[d]);
                        } else if (KIND == 1) {
                            const double u0 = xa0[d] - xc[d], u1 = xa1[d] - xc[d];
                            g0 = (p.sigma2 * exp_nonpos((u0 * u0) * nhd[d])) * (u0 * (2.0 * nhd[d]));
                            g1 = (p.sigma2 * exp_nonpos((u1 * u1) * nhd[d])) * (u1 * (2.0 * nhd[d]));
                        } else if (KIND == 2) {
                            g0 = g1 = xc[d] * p.il2;
                        } else {
                            g0 = g1 = xc[d] * nhd[d];
                        }
                        g0 = in ? g0 : 0.0;
                        g1 = in ? g1 : 0.0;
#pragma unroll
                        for (int ch = 0; ch < TIG_CH; ++ch) {
                            if (ch >= nch) continue;
                            acc[d][ch][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ch], g0, acc[d][ch][0], 0, 0, 0);
                            acc[d][ch][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ch], g1, acc[d][ch][1], 0, 0, 0);
                        }
                    }
            }
            // register r of acc[d][ch][rn]: (column q0 + 16 ch + l4 + 4 r, test row 32 w + 16 rn + l15)
#pragma unroll
            for (int d = 0; d < DC; ++d) {
                if (d >= en) continue;
#pragma unroll
                for (int ch = 0; ch < TIG_CH; ++ch) {
                    if (ch >= nch) continue;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        double* pp = tk.part + ((size_t)(e0 + d) * qpad + (size_t)(q0 + ch * TQ + l4 + 4 * r)) * TB;
                        if (live0) pp[r0] = acc[d][ch][0][r];
                        if (live1) pp[r1] = acc[d][ch][1][r];
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void targets_inputgrad_kernel(const TargetsInputGradTask* __restrict__ tasks,
                                                                const KParam* __restrict__ kp, int D, int qpad) {
    const TargetsInputGradTask tk = tasks[blockIdx.x];
    const KParam p = kp[tk.kid];
    DSMGP_KIND_DISPATCH_NON_RQ(p.kind, K, targets_inputgrad_body<K>(tk, p, D, qpad));
}

// the tasks of rational quadratic leaves (kinds 9, 10), over the same list, as pred_inputgrad_rq_kernel: launched only while a
// kernel id has such a kind; each of the two kernels leaves the other's tasks alone
__global__ __launch_bounds__(256) void targets_inputgrad_rq_kernel(const TargetsInputGradTask* __restrict__ tasks,
                                                                   const KParam* __restrict__ kp, int D, int qpad) {
    const TargetsInputGradTask tk = tasks[blockIdx.x];
    const KParam p = kp[tk.kid];
    if (p.kind < 9) return;
    targets_inputgrad_body<6>(tk, p, D, qpad);
}

// The slabs of a test tile in ascending order; NaN for a leaf whose factorisation failed.  Grid (tiles, Q), one thread per row:
// only rows < nrows and columns < Q are written.
struct TargetsInputGradFinTask {
    const double* part;     // the tile's first slab; slab s at part + s * pstride
    double* out;            // dmu of the tile's first entry: (d, q) at out + (d + q D) * ldo
    const int* info;
    long long pstride, ldo;
    int nslab, nrows;
};

__global__ __launch_bounds__(128) void targets_inputgrad_finish_kernel(const TargetsInputGradFinTask* __restrict__ tasks, int D,
                                                                       int qpad) {
    const TargetsInputGradFinTask tk = tasks[blockIdx.x];
    const int r = threadIdx.x, q = blockIdx.y;
    if (r >= tk.nrows) return;
    const bool bad = *tk.info != 0;
    for (int d = 0; d < D; ++d) {
        double s = 0.0;
        if (!bad)
            for (int k = 0; k < tk.nslab; ++k) s += tk.part[(size_t)k * tk.pstride + ((size_t)d * qpad + q) * TB + r];
        tk.out[r + ((size_t)d + (size_t)q * D) * tk.ldo] = bad ? __builtin_nan("") : s;
    }
}

}  // namespace dsmgp
