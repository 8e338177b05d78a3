/*
 * dsmgp_hip.h -- C ABI of the MI355X (gfx950) GP-expert hot path of DeepStructuredMixtures.
 *
 * The reference (Julia) has no FFI of its own: the boundary is the set of Julia methods whose
 * bodies are the hot path.  Each entry point below names the reference
 * code it replaces; INTEGRATION.md shows the `ccall` glue a maintainer would add.
 *
 * Conventions
 *   - all matrices are column-major Float64 (Julia `Matrix{Float64}`), indices 0-based, sizes int64/int32
 *   - every function returns 0 on success, a negative DSMGP_E_* code on failure; the message is
 *     available from dsmgp_last_error(); nothing throws or longjmps across the ABI
 *   - the caller owns every host pointer; the library never keeps a host pointer after return
 *   - a context is bound to ONE GPU and must not be used from two threads at once (the reference
 *     `fit!` loop is serial, src/fit.jl:88); multi-GPU = one context per process/GPU, leaves sharded
 *     by the caller
 *   - hyper-parameters are on the reference's log scale: [logl..., logs, logNoise] with
 *     lengthscale exp(logl), signal variance exp(2 logs), noise variance exp(2 logNoise)
 *     (src/kernels.jl:68-73, src/gaussianprocess.jl:39,153-161)
 */
#ifndef DSMGP_HIP_H
#define DSMGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsmgp_ctx dsmgp_ctx;

/* kernel kinds (src/kernels.jl:59,109,174,209) */
#define DSMGP_KIND_ISO_SE     0
#define DSMGP_KIND_ARD_SE     1   /* additive form, src/kernels.jl:39-49 */
#define DSMGP_KIND_ISO_LINEAR 2
/* ArdLinear: k(a, b) = sum_d a_d b_d / l_d^2, l_d = exp(logl_d), d = 1..D -- the generic ArdKernel loop of src/kernels.jl:39-49
 * with getlengthscales(k).^2 and kappa = z -> z / l (:228-229), per entry the product a_d b_d scaled by 1 / l_d^2 and added in
 * ascending d (k(a, b) == k(b, a) to the bit).  Exactly D length-scales; no signal variance: the variance slot of the
 * hyper-vector [logl_1..logl_D, 0, logNoise] is a dummy (getvariance = 1, setvariance! a no-op, :216-218).  A repair: the
 * reference's ArdLinear cannot be fitted (getdistancematrix returns a Vector{Matrix} no kernelmatrix method takes, :232;
 * getgradients reads an undefined name, :247). */
#define DSMGP_KIND_ARD_LINEAR 3
/* ArdSEProduct: the product-form squared exponential with one length-scale per input dimension (GPML covSEard),
 * k(a, b) = sigma^2 exp(z), z = sum_d (a_d - b_d)^2 * (-0.5 / l_d^2) added in ascending d (each term depends on (a_d - b_d)^2
 * only: k(a, b) == k(b, a) to the bit).  Hyper-vector [logl_1..logl_D, logs, logNoise] as ArdSE; exactly D length-scales
 * (set_hyper refuses another length once set_train has fixed D).  Not a kernel of the reference, whose ArdSE is additive. */
#define DSMGP_KIND_ARD_SE_PRODUCT 4
/* Matern kernels, distance form (GPML covMaterniso / covMaternard): r^2 = sum_d (a_d - b_d)^2 / l_d^2, s = sqrt(2 nu) r,
 * k(a, b) = sigma^2 (1 + s) exp(-s) for nu = 3/2 and sigma^2 (1 + s + s^2 / 3) exp(-s) for nu = 5/2; k(x, x) = sigma^2.  s^2 is
 * added in ascending d from (a_d - b_d)^2 * (2 nu / l_d^2) (k(a, b) == k(b, a) to the bit; an iso kind is its ARD kind with all
 * l_d equal, to the bit).  Iso hyper-vector [logl, logs, logNoise] (exactly 3 values); ARD [logl_1..logl_D, logs, logNoise]
 * (exactly D length-scales once set_train has fixed D): set_hyper refuses other lengths.  Not kernels of the reference. */
#define DSMGP_KIND_ISO_MATERN32 5   /* nu = 3/2, one length-scale */
#define DSMGP_KIND_ISO_MATERN52 6   /* nu = 5/2, one length-scale */
#define DSMGP_KIND_ARD_MATERN32 7   /* nu = 3/2, one length-scale per input dimension */
#define DSMGP_KIND_ARD_MATERN52 8   /* nu = 5/2, one length-scale per input dimension */
/* Rational quadratic kernels (GPML covRQiso / covRQard), a scale mixture of squared exponentials with a trainable shape:
 * k(a, b) = sigma^2 (1 + w)^(-alpha), w = sum_d (a_d - b_d)^2 / (2 alpha l_d^2), alpha = exp(loga); k(x, x) = sigma^2 exactly.  w is
 * added in ascending d from (a_d - b_d)^2 * (1 / (2 alpha l_d^2)), one fma per dimension, and the value is sigma^2 exp(-alpha
 * log1p(w)) (k(a, b) == k(b, a) to the bit; the iso kind is its ARD kind with all l_d equal, to the bit).  The first kinds with a
 * shape parameter: it sits between the length-scales and logs.  Iso hyper-vector [logl, loga, logs, logNoise] (exactly 4 values);
 * ARD [logl_1..logl_D, loga, logs, logNoise] (exactly D + 3 values once set_train has fixed D): set_hyper refuses other lengths.
 * Not kernels of the reference. */
#define DSMGP_KIND_ISO_RQ 9         /* one length-scale */
#define DSMGP_KIND_ARD_RQ 10        /* one length-scale per input dimension */

/* per-leaf sharing decisions of the shared-Cholesky fit! (src/fit.jl:107-117) */
#define DSMGP_SHARE_FULL   0      /* update_cholesky!               src/gaussianprocess.jl:82-108 */
#define DSMGP_SHARE_COPY   1      /* identical observation sets     src/fit.jl:132-143 */
#define DSMGP_SHARE_PREFIX 2      /* chol_continue! from column p   src/fit.jl:276-278, src/AdvancedCholeskey.jl:152-174 */

/* error codes */
#define DSMGP_OK            0
#define DSMGP_E_ARG        -1
#define DSMGP_E_STATE      -2
#define DSMGP_E_HIP        -3
#define DSMGP_E_NOMEM      -4
#define DSMGP_E_NODEVICE   -5
#define DSMGP_E_DOMAIN     -6   /* a test row outside the region of a split node (NaN included): the reference loops forever there */

/* number of doubles dsmgp_timings() fills: gram, chol_update (the update launches of the tile kernel alone),
 * chol_diag, chol_trsm, solve (forward substitution of COPY / PREFIX leaves), mll, predict_gram, predict_update,
 * predict_trsm, predict_var, gradients, total_fit, total_predict, chol_reduce (split-K reduce launches of the
 * factorisation), alpha (the backward sweep alpha = L^-T z, run on first use after a fit: gradients, download_factor),
 * grad_inverse (L^-T by blocked triangular inversion), grad_contraction (tile_graddot_kernel), grad_traces,
 * chol_fused (the tile_fused8_kernel launches of fused block steps: update + solve of the tiles below the diagonal blocks),
 * chol_update_union, chol_fused_union (with two leaf lanes the launches of a kind overlap in time: chol_update / chol_fused are the
 * SUM of their durations, these the time during which any of them ran; one lane: the same numbers) */
#define DSMGP_N_TIMINGS 21

/* kernel ids are dense small integers (one hyper-vector each; finetune! gives every leaf its own) */
#define DSMGP_MAX_KERNEL_IDS (1 << 22)

/* ---- context ---------------------------------------------------------------------------------- */
int dsmgp_create(int32_t device_id, dsmgp_ctx** out);
int dsmgp_destroy(dsmgp_ctx* ctx);
const char* dsmgp_last_error(dsmgp_ctx* ctx);     /* ctx may be NULL: error of the failed create */
int dsmgp_device_name(dsmgp_ctx* ctx, char* buf, int32_t len);

/* ---- data: replaces the GaussianProcess constructor's host copies
 *      (src/gaussianprocess.jl:50-80: x, mean-subtracted y; the distance tensor P is never stored) */
int dsmgp_set_train(dsmgp_ctx* ctx, const double* X /* N x D */, const double* y /* N */,
                    int64_t N, int32_t D);

/* leaf table = output of buildTree (src/treeStructure.jl:245-307): obs lists in CSR form
 * (ascending 0-based row indices), kernel id (0-based), ConstMean value per leaf (src/means.jl:7-14).
 * The leaf count L of a context is bounded by device memory only: every launch with one grid row per leaf is cut into runs
 * of 32,768 leaves, so no grid dimension grows with L beyond that.  Tables of 33,000 and 65,600 leaves are part of the test
 * suite.  dsmgp_memory's `needed` covers the arenas of the fit only (factor, Dinv, four vectors and the gathered inputs of
 * every leaf: about 268 KB per leaf of up to 128 rows, measured).  L^-T of a gradient, LOO or k-fold pass, the target columns
 * and the k-fold arenas come ON TOP and are not in `needed`: by the code L^-T is another npad^2 doubles per factor owner, about
 * 131 KB per leaf of up to 128 rows (not measured). */
int dsmgp_set_leaves(dsmgp_ctx* ctx, int32_t L, const int64_t* obs_ptr /* L+1 */,
                     const int64_t* obs_idx, const int32_t* kernel_id, const double* mean /* L */);

/* sharing schedule decided by the caller exactly as src/fit.jl:78-117 does; NULL op = all FULL.
 * The library validates COPY/PREFIX claims against the obs lists and returns DSMGP_E_ARG on a lie. */
int dsmgp_set_sharing(dsmgp_ctx* ctx, const int32_t* op /* L */, const int32_t* src /* L */,
                      const int64_t* prefix_len /* L */);

/* replaces setparams!(gp, hyper) (src/gaussianprocess.jl:153-161, src/optimize.jl:188-198) for all
 * leaves of one kernel id; n = (#lengthscales) + 2, one more for the rational quadratic kinds (their shape loga).  DSMGP_E_ARG:
 * an unknown kind, a non-finite value, or a length the kind does not take (checked here for kinds 4-10, at the fit for the
 * reference's kinds) */
int dsmgp_set_hyper(dsmgp_ctx* ctx, int32_t kernel_id, int32_t kind, const double* loghyp, int32_t n);

/* ---- fit!: Gram assembly + Cholesky + alpha for every leaf
 *      replaces fit!/fit_naive!/update_cholesky! (src/fit.jl:71-122,294-304; src/gaussianprocess.jl:82-108)
 *      and mll(gp) (src/gaussianprocess.jl:163).
 *      mll_out[l]  = -(y.alpha + logdet + n log 2pi)/2, with y.alpha evaluated as |L^-1 y|^2; gp.alpha itself is
 *                    materialised on first use (dsmgp_gradients, dsmgp_download_factor), not by fit
 *      info_out[l] = 0, or k>0 if the leading minor of order k is not positive definite (LAPACK potrf)
 *                    A COPY leaf reports its source's value.  A PREFIX leaf whose source failed inside the rows it copies
 *                    (k <= 128 floor(prefix_len / 128)) has the same first bad minor and reports the same k: on the device it
 *                    meets the damage at its first own pivot, so it is flagged as failed there too and gets NaN wherever a
 *                    failed leaf does (dsmgp_solve_targets, dsmgp_predict_targets, dsmgp_loo*, dsmgp_predict_gradients, ...).
 *                    Where the source fails later, in a block the PREFIX leaf recomputes, the leaf finds its own k.  Every
 *                    other leaf, the other PREFIX and COPY leaves of other sources included, keeps its bits.
 *                    (dsmgp_fit_exchange ships the device's flag: nonzero for such a leaf, row 128 floor(prefix_len / 128) + 1.)
 *      seconds     = device time of the call (hipEvents), like the @elapsed value fit! returns */
int dsmgp_fit(dsmgp_ctx* ctx, double* mll_out /* L */, int32_t* info_out /* L */, double* seconds);

/* ---- append training rows to a fitted model without refactorising it (not a call of the reference): the step after an
 *      acquisition, "observe the chosen point and add it".  Equivalent, with the hyper-parameters of the current fit, to
 *        dsmgp_set_train([X; X_new], [y; y_new]);
 *        dsmgp_set_leaves with every leaf's list grown by N_old + add_idx[add_ptr[l] .. add_ptr[l + 1]), the same kernel ids, `mean`;
 *        the sharing schedule below;  dsmgp_fit
 *      except that every factor owner keeps the leading kb = floor(n_old / 128) block rows and columns of the factor it had (the
 *      Cholesky factor of a matrix with rows appended has the old factor as its leading block) and only the block columns from
 *      kb on are factorised: the continuation the PREFIX phase of dsmgp_fit runs (chol_continue!, src/AdvancedCholeskey.jl:152-174),
 *      with the leaf's own old factor as the source.  O(n 128 n) flops per leaf that receives rows instead of n^3 / 3, nothing for
 *      the others.  mll_out, info_out, seconds: dsmgp_fit's, with its conventions; a first bad minor inside the new blocks is
 *      reported with its absolute order.  A new row that no leaf takes is allowed and is stored with the data.
 *      Needs a current fit and no reserved pool (DSMGP_E_STATE: after dsmgp_set_hyper, before the first fit, under dsmgp_reserve).
 *      DSMGP_E_ARG, the context exactly as before: m < 1, D not the D of dsmgp_set_train, a NULL among X_new, y_new, add_ptr,
 *      add_idx, a non-finite value (X_new, y_new, mean), add_ptr[0] != 0 or descending, a position outside 0 .. m-1, a list
 *      that is not strictly ascending, a leaf beyond the size limit of dsmgp_set_leaves.
 *      Sharing after the call: a COPY leaf stays a COPY of its source if and only if both receive identical additions (decided
 *      here); every other leaf owns its factor from now on -- a former PREFIX leaf continues from its own factor, a COPY leaf
 *      whose additions differ from its source's gets a factor of its own, continued from the source's old one.  Later
 *      dsmgp_fit calls run under exactly this schedule (COPY where kept, FULL elsewhere) and factorise in full: the
 *      continuation is one-shot.  dsmgp_set_sharing works as always.  Owners whose fit reported info != 0 are factorised from
 *      block 0 (their kept blocks are damaged).
 *      State after the call: the plan and the fit are current; the routing tree of dsmgp_set_tree stays registered (leaf
 *      indices do not change); everything else that falls with a new leaf table falls -- the resident test set, the gradient,
 *      LOO and target lists and arenas, L^-T, the mask of dsmgp_set_gradient_leaves -- and captured fit graphs are dropped (the
 *      call itself never runs as a graph).
 *      Storage: IN PLACE when no owner's padded size (n rounded up to 128) changes and the ownership map is unchanged: the
 *      factor and Dinv arenas stay where they are and no kept byte moves; the partial block row kb is rewritten tile by tile
 *      before it is read.  Otherwise RELOCATE: new arenas are allocated while the old ones are alive, the kept blocks move in
 *      one launch, the old arenas are freed: PEAK MEMORY IS THE OLD FACTORS PLUS THE NEW ONES.  If the new arenas do not fit:
 *      DSMGP_E_NOMEM, and the context holds the grown data and leaf table and no fit, as after dsmgp_set_leaves (the next
 *      dsmgp_fit factorises in full).  (If not even the grown copy of the data fits, DSMGP_E_NOMEM leaves the context as before;
 *      if the device copy of the grown leaf table cannot be made, the context keeps the grown data and NO leaf table: dsmgp_set_leaves next.)
 *      Guarantees: for every owner with info == 0 before and after, the leading 128 kb square of its factor is the same bits as
 *      before the call; a leaf without additions keeps every factor bit (z and the log-marginal are recomputed from them);
 *      same inputs on the same state give the same bits (no atomics).  dsmgp_timings, dsmgp_work and dsmgp_work_fused
 *      describe the call as they would a fit.
 *      dsmgp_append_stats (of the last dsmgp_append_rows; DSMGP_E_STATE before the first): [0] owners continued (kept blocks
 *      and factorised the rest), [1] leaves untouched (no additions, same mean, factor not moved: 0 on the relocate path),
 *      [2] bytes of factor and Dinv relocated (0 = the in-place path ran), [3] block columns factorised, summed over the
 *      owners, [4] owners restarted from block 0, [5] COPY relations dissolved. */
int dsmgp_append_rows(dsmgp_ctx* ctx, const double* X_new /* m x D column-major, ld = m */, const double* y_new /* m */,
                      int64_t m, int32_t D, const int64_t* add_ptr /* L+1 */,
                      const int64_t* add_idx /* positions 0..m-1 in X_new, strictly ascending per leaf */,
                      const double* mean /* L: the leaves' means from now on; NULL = unchanged */,
                      double* mll_out /* L, may be NULL */, int32_t* info_out /* L, may be NULL */, double* seconds /* may be NULL */);
#define DSMGP_N_APPEND_STATS 6
int dsmgp_append_stats(dsmgp_ctx* ctx, int64_t* out /* DSMGP_N_APPEND_STATS, of the last dsmgp_append_rows */);

/* ---- the same, for the loop acquire -> add the observed point -> predict again ON THE SAME CANDIDATES: the resident test set
 *      stays resident and dsmgp_predict_run resumes K_tn L^-T instead of sweeping it from block column 0.
 *      Arguments, results, refusals, guarantees, factor storage paths and dsmgp_append_stats: those of dsmgp_append_rows (one
 *      body).  Without a resident test set the call IS dsmgp_append_rows.  With one:
 *      The test set: appended training rows change neither the tree nor the leaf indices, so the routes are the same: the test
 *      rows, the CSR and the per-row entry index stay as they are (dsmgp_routes returns the same arrays before and after), and
 *      the second half of the registration runs again on the grown plan (per-leaf sizes, arenas, gathered rows, task lists).
 *      Dropped and rebuilt on demand as after any registration: the buffers of dsmgp_predict_gradients, dsmgp_predict_cov,
 *      dsmgp_predict_targets, dsmgp_aggregate* and the lists of a joint fit.
 *      Kept columns: where dsmgp_predict_run had run on the fit the call found, every leaf with routed rows keeps the leading
 *      128 keep columns of its K_tn L^-T, keep = the leading blocks kept of the factor it reads: floor(n_old / 128) for an owner
 *      that receives rows, every block for a leaf without additions, 0 where the old fit reported info != 0; a COPY leaf,
 *      whether it stays one or gets a factor of its own, the kept blocks of the factor it reads.  Without such a run keep = 0
 *      everywhere: the test set is still kept, only the sweep is full.  A second call before any dsmgp_predict_run: a leaf's
 *      count can only shrink (the minimum of what it had and what this call keeps).
 *      Storage of K_tn L^-T (ntpad x npad per leaf, column-major, ld = ntpad: a grown leaf gains columns at the end and its kept
 *      columns stay one contiguous run): in place when no leaf's offset or padded sizes change -- the arena stays and no byte
 *      of it moves; otherwise a new arena is allocated while the old one is alive, the kept runs move in one launch and the old
 *      arena is freed (never a move inside one arena).  This happens after the old factors have been freed: the peak of the
 *      call is the larger of "old + new factors + old K_tn L^-T" and "new factors + old + new K_tn L^-T".  If the new arena does
 *      not fit, the call still returns 0 (the fit is good), the test set is dropped, dsmgp_resume_stats says so and the next
 *      dsmgp_predict_run returns DSMGP_E_STATE, as after dsmgp_append_rows.  The failure paths of the append itself drop the
 *      test set as dsmgp_append_rows does.
 *      dsmgp_predict_run after the call: for every leaf the block steps k < keep are not run; steps keep .. nb-1 run through
 *      the sweep's own kernels and write their block columns whole (block column keep is the partial old block: stale).  The
 *      moment sums over the kept columns, which the sweep's epilogues would have added, are formed first against the current
 *      z, each kept tile read once for both sums, in chunks of a constant number of block columns added in ascending order.
 *      One-shot: it applies to the fit the call made; dsmgp_fit and the dsmgp_predict_run that used it end it, and a
 *      dsmgp_predict_run after a later dsmgp_fit returns exactly what it returns after a fresh dsmgp_set_test of the same rows.
 *      After the resumed run every reader of K_tn L^-T and of the moments works on the grown model (dsmgp_predict_fetch,
 *      dsmgp_predict_cov, dsmgp_predict_gradients, dsmgp_predict_targets, dsmgp_aggregate*, dsmgp_download_vt).  A repeated
 *      dsmgp_predict_run leaves the same bits; same inputs on the same state give the same bits (fixed summation order, no
 *      atomics).  NOT promised: that mu / var of a leaf without additions keep their bits (their sums are formed again), or
 *      that the results equal a sweep from block 0 to the bit.
 *      dsmgp_resume_stats (of the last dsmgp_add_rows_keep_test and the dsmgp_predict_run that used it; DSMGP_E_STATE before the
 *      first): [0] leaves with routed rows that kept columns, [1] block columns of K_tn L^-T kept, summed over those leaves,
 *      [2] bytes of K_tn L^-T relocated (0 = in place), [3] block columns swept by the resumed dsmgp_predict_run, summed over the
 *      leaves with routed rows (-1 until it has run), [4] leaves swept from block 0, [5] 1 if the test set had to be dropped
 *      for lack of memory. */
int dsmgp_add_rows_keep_test(dsmgp_ctx* ctx, const double* X_new /* m x D column-major, ld = m */, const double* y_new /* m */,
                             int64_t m, int32_t D, const int64_t* add_ptr /* L+1 */,
                             const int64_t* add_idx /* positions 0..m-1 in X_new, strictly ascending per leaf */,
                             const double* mean /* L: the leaves' means from now on; NULL = unchanged */,
                             double* mll_out /* L, may be NULL */, int32_t* info_out /* L, may be NULL */, double* seconds /* may be NULL */);
#define DSMGP_N_RESUME_STATS 6
int dsmgp_resume_stats(dsmgp_ctx* ctx, int64_t* out /* DSMGP_N_RESUME_STATS */);
/*      Inspection, like dsmgp_download_factor: K_tn L^-T of one leaf over its routed rows and its n real columns.  Needs
 *      dsmgp_predict_run on the current fit (DSMGP_E_STATE).  DSMGP_E_ARG: leaf out of range, ld < nt.  A leaf without routed
 *      rows: success, nothing written. */
int dsmgp_download_vt(dsmgp_ctx* ctx, int32_t leaf, double* V_out /* nt x n column-major */, int64_t ld);

/* ---- prediction(gp, xtest) for every (leaf, routed test row): src/gaussianprocess.jl:110-137
 *      mu  = m + Knt' alpha ; var = k(x*,x*) - |L^-1 k_n*|^2 + exp(2 logNoise)   (diag only; no clamp,
 *      the caller applies src/common.jl:137).  route_ptr/route_idx: per leaf, which rows of Xt.
 *      Outputs are aligned with route_idx. */
/* While a test set is resident (dsmgp_set_test), dsmgp_fit also advances its rows through the factorisation
 * launches (V^T = K_tn L^-T rides along as extra row tiles), and dsmgp_predict_run only finishes mu and var.
 * dsmgp_set_joint(ctx, 0) switches that off (e.g. inside train!, where fit is not followed by predict). */
int dsmgp_set_joint(dsmgp_ctx* ctx, int32_t on);
/* D = number of columns of Xt as the caller holds it: DSMGP_E_ARG unless it is the D of dsmgp_set_train (n_t * D doubles are read). */
int dsmgp_set_test(dsmgp_ctx* ctx, const double* Xt /* n_t x D column-major */, int64_t n_t, int32_t D,
                   const int64_t* route_ptr /* L+1 */, const int64_t* route_idx);
/* predict(model, x) on rows the model has not seen (the reference's normal call, src/common.jl:304-307, src/plot.jl:40): the routing
 * of src/common.jl:101-122,181-196,275-292 on the device.  dsmgp_set_tree registers the model's tree once per leaf table (flat
 * arrays as dsmgp_tree_route takes them; leaf_id = index in THIS context's leaf table, -1 = a region another rank holds; a new
 * leaf table or new training data drop it).  The held leaves (leaf_id >= 0) must be numbered depth-first, children in order, each
 * named by one region: DSMGP_E_ARG otherwise, since the device path keeps one bit per (leaf, row) and a row's entries in the
 * order its walk meets them (dsmgp_tree_route builds lists for any tree).  dsmgp_set_test_routed(Xt, n_t, D) then is dsmgp_set_test with the routes made on the
 * device: one thread per row walks the tree, a bitmap per leaf turns the visits into the same CSR (rows ascending per leaf) and the
 * same per-row entry index the host path builds -- entry by entry -- and only the L + 1 per-leaf offsets come back to the host
 * (they size the K_tn arena and the sweep's task lists).  DSMGP_E_DOMAIN: a row outside the region of a split node (NaN included).
 * dsmgp_routes fetches the CSR of the registered test set (route_ptr: L + 1; route_idx: route_ptr[L] entries, may be NULL). */
int dsmgp_set_tree(dsmgp_ctx* ctx, int64_t n_nodes, const int8_t* kind, const int64_t* first_child, const int64_t* n_child,
                   const int64_t* split_dim, const double* thr, int64_t thr_ld, const int64_t* leaf_id);
int dsmgp_set_test_routed(dsmgp_ctx* ctx, const double* Xt /* n_t x D column-major */, int64_t n_t, int32_t D);
int dsmgp_routes(dsmgp_ctx* ctx, int64_t* route_ptr /* L+1 */, int64_t* route_idx /* or NULL */);
/* dsmgp_predict_run: device work only, inputs resident.  A repeated call on the same fit and test set leaves the same bits (the
 * sweep is not run again; the moments are finished from the same sums).  A test set without routed rows is a valid one: the call
 * succeeds and dsmgp_predict_cov / dsmgp_predict_gradients / dsmgp_predict_targets answer "nothing written". */
int dsmgp_predict_run(dsmgp_ctx* ctx, double* seconds);
int dsmgp_predict_fetch(dsmgp_ctx* ctx, double* mu_out, double* var_out);
int dsmgp_predict_leaves(dsmgp_ctx* ctx, const double* Xt, int64_t n_t, int32_t D, const int64_t* route_ptr,
                         const int64_t* route_idx, double* mu_out, double* var_out);
/* prediction(gp, xtest) as the reference writes it (src/gaussianprocess.jl:110-137): the full covariance of leaf
 * `leaf` over ITS routed test rows, in route order (the order of its segment of dsmgp_predict_fetch):
 * Sigma = K_tt - V'V (+ exp(2 logNoise) I when with_noise != 0), nt x nt column-major with leading dimension ld >= nt.
 * Needs dsmgp_predict_run on the current fit (DSMGP_E_STATE otherwise); leaf out of range or ld < nt: DSMGP_E_ARG;
 * a leaf without routed rows: success, nothing written.  Symmetric to the bit.  seconds (may be NULL): device time.
 * Its ntpad x ntpad device scratch (nt rounded up to 128) is allocated on first use -- from the reserved pool when there is
 * one -- and is NOT counted by dsmgp_estimate_bytes / dsmgp_memory; it is dropped with the test set, the leaf table and
 * dsmgp_release. */
int dsmgp_predict_cov(dsmgp_ctx* ctx, int32_t leaf, int32_t with_noise, double* Sigma_out, int64_t ld, double* seconds);
/* Joint posterior draws of every leaf GP over its routed test rows (not a call of the reference: Thompson sampling, batch
 * selection by sampled maxima, Monte-Carlo acquisition values).  The caller supplies the standard normals; no random number is
 * made on the device.  For every leaf l with routed rows, over its segment e0 .. e0 + nt - 1 of the entries of
 * dsmgp_predict_fetch, in that order:
 *   A_l = Sigma_l + jitter I, Sigma_l exactly what dsmgp_predict_cov(leaf = l, with_noise) returns (same kernel, same bits),
 *   C_l = chol(A_l), lower,
 *   out[e0 + i + s * ld_out] = mu[e0 + i] + sum_{j <= i} C_l[i, j] eps[e0 + j + s * ld_eps].
 * Column s is one joint draw of every leaf; leaves are independent of each other.  eps and out are route_total x S, column-major.
 * info_out (L, may be NULL): 0 = success; k > 0 = the leading minor of order k of A_l is not positive definite (LAPACK potrf's
 * convention, as dsmgp_fit reports it); -1 = a leaf whose fit reported info != 0.  A leaf with info_out[l] != 0 gets NaN in all
 * its entries, every other leaf is unaffected; a leaf without routed rows reports 0 and writes nothing.
 * Needs dsmgp_predict_run on the current fit (DSMGP_E_STATE otherwise), on either route to K_tn L^-T: rows that rode through the
 * fit, or the standalone sweep; one lane or two.  DSMGP_E_ARG: S < 1 or S > 65535, a NULL eps or out, ld_eps or ld_out below
 * route_total, a jitter that is negative or not finite, a non-finite value in eps.  No routed rows at all: success, nothing
 * written.  Runs on the context's stream and synchronises before it returns.  seconds (may be NULL): device time of the call.
 * Sums run in a fixed order and there are no atomics: the same bits from call to call, and column s is the same bits whatever S
 * is and whatever the other columns hold.  dsmgp_predict_fetch, dsmgp_predict_cov, dsmgp_predict_gradients,
 * dsmgp_predict_targets, dsmgp_aggregate*, dsmgp_scores and dsmgp_fit's outputs return the same bits before and after this call.
 * The factors are kept, tagged with (with_noise, jitter): a second call with the same tag and new eps skips the factorisation
 * (Thompson loops draw repeatedly); whatever fells the prediction fells them (a new fit, new hyper-parameters, a new test set,
 * dsmgp_predict_run, dsmgp_add_rows_keep_test -- after it and the resumed dsmgp_predict_run the call works on the grown model).
 * Memory: dsmgp_predict_cov keeps its own scratch; the factors live in an arena of their own, ntpad^2 doubles per leaf with routed
 * rows (nt rounded up to 128), plus 128 ntpad for the inverted diagonal blocks and two staging buffers of route_total x S rounded
 * up to 16: allocated on first use (the arenas from the reserved pool when there is one; DSMGP_E_NOMEM with a usable context when
 * they do not fit), NOT counted by dsmgp_estimate_bytes / dsmgp_memory, dropped with the test set, the leaf table and
 * dsmgp_release.  Cost: the n nt^2 flops of Sigma_l, nt^3 / 3 of its factorisation, nt^2 S of the draws, all on the f64 matrix
 * cores.  Draws of the target columns of dsmgp_solve_targets differ from these by the mean only and are not offered. */
int dsmgp_predict_sample(dsmgp_ctx* ctx, int32_t with_noise, double jitter,
                         const double* eps /* route_total x S, column-major */, int64_t ld_eps, int32_t S,
                         double* out /* route_total x S, column-major */, int64_t ld_out,
                         int32_t* info_out /* L, may be NULL */, double* seconds /* may be NULL */);
/* Device seconds of the last successful dsmgp_predict_sample, split: out[0] forming Sigma (with the uploads of the task lists),
 * out[1] the factorisation, out[2] the staging of eps and the draws; out[0] = out[1] = 0 when the call found its factors current. */
int dsmgp_predict_sample_seconds(dsmgp_ctx* ctx, double* out /* 3 */);
/* Inspection, like dsmgp_download_factor: C_l of the last dsmgp_predict_sample, nt x nt column-major with leading dimension
 * ld >= nt: the lower triangle, the strict upper triangle exactly 0.  DSMGP_E_STATE when no current factor exists; leaf out of
 * range, a NULL Lc_out or ld < nt: DSMGP_E_ARG; a leaf without routed rows: success, nothing written.  The factor of a leaf whose
 * flag is not 0 holds no meaning. */
int dsmgp_predict_cov_factor(dsmgp_ctx* ctx, int32_t leaf, double* Lc_out /* nt x nt column-major */, int64_t ld);
/* Gradients of the predictive mean and variance with respect to the test point (not a call of the reference): for every
 * (leaf, routed test row t) -- the entries of dsmgp_predict_fetch, in its order -- and every input dimension d,
 *   dmu_out[e + d * ld]  = d mu / d x_{t,d}  = sum_i alpha_i dk(x_t, x_i) / dx_{t,d},
 *   dvar_out[e + d * ld] = d var / d x_{t,d} = dk(x_t, x_t) / dx_{t,d} - 2 sum_i beta_{t,i} dk(x_t, x_i) / dx_{t,d},
 * beta_t = K_y^-1 k_t: the derivative of var as dsmgp_predict_fetch returns it (noise and jitter are constants).  Both outputs
 * are route_total x D, column-major with leading dimension ld >= route_total (DSMGP_E_ARG otherwise); either may be NULL.
 * The kernel derivatives are true derivatives, finite at x_t = x_i (nothing divides by a distance): with D_d = x_{t,d} - x_{i,d},
 * -k D_d / l_d^2 (IsoSE, ArdSEProduct), -sigma^2 exp(-D_d^2 / 2 l_d^2) D_d / l_d^2 (ArdSE: term d only), x_{i,d} / l_d^2 (the
 * linear kinds, whose dk(x_t, x_t) / dx_{t,d} = 2 x_{t,d} / l_d^2; it is 0 for the stationary kinds), and
 * -sigma^2 exp(-s) c(s) (2 nu / l_d^2) D_d for the Matern kinds, c(s) as in dsmgp_gradients, and -k / (1 + w) D_d / l_d^2 for the
 * rational quadratic kinds.  Any D.
 * Needs dsmgp_predict_run on the current fit (DSMGP_E_STATE otherwise), on either route to K_tn L^-T: rows that rode through the
 * fit, or the standalone sweep; one lane or two.  No routed rows at all: success, nothing written.  Leaves whose fit reported
 * info != 0 get NaN rows, the others are unaffected.  Sums are added in a fixed order: the same bits from call to call, and
 * dmu_out is the same bits with and without dvar_out.  seconds (may be NULL): device time of the call.
 * dmu reads alpha (materialised here on first use after a fit) and the inputs only.  dvar needs B = K_tn K_y^-1 = (K_tn L^-T) L^-1:
 * a tile product on the matrix cores against L^-T of every factor owner (a COPY leaf: its source's), the arena dsmgp_gradients
 * fills -- read as it is, or filled here, by the rule of dsmgp_loo, and what that call says about dsmgp_gradients and the mask
 * of dsmgp_set_gradient_leaves holds here too (both are left exactly as they are; the mask does not apply; DSMGP_E_NOMEM /
 * DSMGP_E_ARG where the lists of the inversion cannot be built).  With dvar_out = NULL none of that is computed or allocated.
 * dsmgp_predict_fetch, dsmgp_predict_cov, dsmgp_gradients and dsmgp_loo* return the same bits before and after this call.
 * Memory: B gets an arena of its own, the size of the K_tn arena (ntpad x npad per leaf with routed rows; K_tn L^-T must
 * survive for dsmgp_predict_cov), plus 2 D doubles per routed row and per 128 training rows of its leaf for the partial sums:
 * allocated on first use (the arena from the reserved pool when there is one; DSMGP_E_NOMEM with a usable context when it
 * does not fit), NOT counted by dsmgp_estimate_bytes / dsmgp_memory, dropped with the test set, the leaf table and
 * dsmgp_release.  Cost: n^2 n_t flops per leaf for B, the order of the standalone sweep, and n n_t D kernel derivatives. */
int dsmgp_predict_gradients(dsmgp_ctx* ctx, double* dmu_out, double* dvar_out /* route_total x D, column-major, ld */,
                            int64_t ld, double* seconds);

/* Several target columns over the same inputs on ONE factorisation (not a call of the reference): the seven joint torques of a
 * robot arm, sensor channels, bootstrap or permuted targets.  After dsmgp_fit the factor, the inverted diagonal blocks and (after
 * dsmgp_predict_run) K_tn L^-T do not depend on y; only z = L^-1 (y - m) does.  With K_y = L L^T the matrix the fit factorised:
 *   dsmgp_solve_targets    Z[l] = L^-1 (Y[obs(l), :] - mean[l, :]) for every leaf, resident in HBM, and
 *                          mll_out[l + j L] = -(|Z[l][:, j]|^2 + 2 sum_i log L_ii + n log 2pi) / 2   (dsmgp_fit's formula per column),
 *   dsmgp_predict_targets  mu_out[e + j ld] = mean[l, j] + sum_{c < n} (K_tn L^-T)[e, c] Z[l][c, j] for every (leaf, routed test row)
 *                          entry e of dsmgp_predict_fetch, in its order,
 *   dsmgp_targets_fetch    Z[l] of one leaf (n x Q, column-major, ld = n): inspection, like dsmgp_download_factor.
 * The predictive variance does not depend on the targets: it is dsmgp_predict_fetch's var_out for every column.
 * Cost: 2 n^2 flops per leaf and column instead of a refit's n^3 / 3: a right-looking block sweep on the f64 matrix cores, one
 * launch per 128-column block step and leaf lane, every factor tile read once per call whatever Q is; the means are one tile
 * product per 128 routed rows.  Sums are added in a fixed order, no atomics: the same bits from call to call, with one lane
 * and with two, and column j's results are the same bits whatever Q is and whatever the other columns hold.
 * A COPY leaf reads its source's factor and has targets and a mean of its own; a PREFIX leaf has its own factor.  Leaves whose
 * fit reported info != 0 get NaN in their mll row and their mu entries; the others are unaffected.
 * dsmgp_solve_targets: Y is N x Q column-major with leading dimension ldy; mean is L x Q column-major (ld = L), NULL = zeros;
 *   mll_out (L x Q, ld = L) and seconds (device time of the call) may be NULL.  Needs a fit on the current leaf table
 *   (DSMGP_E_STATE otherwise).  DSMGP_E_ARG: N is not the N of dsmgp_set_train, Q < 1 (or > 65535), ldy < N, Y NULL, a non-finite
 *   value in Y or mean.  The data of dsmgp_set_train, z and alpha are not touched: dsmgp_fit's outputs, dsmgp_predict_fetch,
 *   dsmgp_predict_cov, dsmgp_gradients, dsmgp_loo* and dsmgp_predict_gradients return the same bits before and after.
 * dsmgp_predict_targets: mu_out is route_total x Q (the Q of the last dsmgp_solve_targets), column-major, ld >= route_total
 *   (DSMGP_E_ARG otherwise).  Needs BOTH dsmgp_solve_targets and dsmgp_predict_run on the CURRENT fit, on either route to
 *   K_tn L^-T (rows that rode through the fit, or the standalone sweep); missing either: DSMGP_E_STATE.  A later dsmgp_fit makes
 *   the resident Z stale: dsmgp_predict_targets and dsmgp_targets_fetch return DSMGP_E_STATE until dsmgp_solve_targets is called
 *   again.  No routed rows at all: success, nothing written.  The K_tn arena is never cleared; its columns >= n are masked on load.
 * Memory: Yc and Z take 2 npad Qpad doubles per leaf (Qpad = Q rounded up to 16, the width of the f64 MFMA tile), plus Y, mean,
 *   mll, mu and the task lists: allocated on first use (the arena from the reserved pool when there is one; DSMGP_E_NOMEM with a
 *   usable context when it does not fit), re-used while Q does not grow, NOT counted by dsmgp_estimate_bytes / dsmgp_memory,
 *   dropped with the leaf table, new training data and dsmgp_release (under a reserved pool also with a new test set: the pool
 *   is a stack).
 * Out of scope: the multi-GPU exchange (each rank solves its own leaves, the mll table is per rank), and the streaming
 *   context.  The input gradients of the columns' means: dsmgp_predict_columns_gradients below.  Gradients of sum_j mll_j:
 *   dsmgp_mll_columns_gradients below; leave-one-out moments and gradients of the columns: dsmgp_loo_columns and
 *   dsmgp_loo_columns_gradients below. */
int dsmgp_solve_targets(dsmgp_ctx* ctx, const double* Y /* N x Q column-major */, int64_t N, int32_t Q, int64_t ldy,
                        const double* mean /* L x Q column-major, ld = L; NULL = zeros */,
                        double* mll_out /* L x Q column-major, ld = L; may be NULL */, double* seconds /* may be NULL */);
int dsmgp_predict_targets(dsmgp_ctx* ctx, double* mu_out /* route_total x Q column-major */, int64_t ld, double* seconds);
int dsmgp_targets_fetch(dsmgp_ctx* ctx, int32_t leaf, double* Z_out /* n x Q column-major, ld = n */);

/* Hyper-parameter gradients of the weighted sum of the per-column log marginal likelihoods of dsmgp_solve_targets:
 *   grad_out[l * stride + j] = sum_q col_weight[l + q L] * d mll_out[l + q L] / d theta_j ,
 * in the layout and with every convention of dsmgp_gradients ([dl..., ds, dnoise], [dl..., da, ds, dnoise] for the rational
 * quadratic kinds; the reference's factor sigma for IsoSE; ArdSE dl zero unless DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT = 1; the dummy
 * variance slot of the linear kinds; zeros past the hyper-vector).  With Q = 1, Y = y, mean = the leaf means and weight 1 it is
 * dsmgp_gradients to rounding.  With A = L^-T Z = K_y^-1 (Y - m), G = K_y^-1 and s_l = sum_q w_lq,
 *   sum_q w_lq d mll_lq / d theta = 1/2 sum_rc ( sum_q w_lq a_rq a_cq - s_l G_rc ) (dK_y / d theta)_rc :
 * one inversion (none when the arena already holds L^-T of this fit, dsmgp_loo's rule) and one contraction per leaf whatever Q
 * is, plus O(n^2 Q) for A (a tile product on the f64 matrix cores) and for the rank-Q term, which the contraction kernels add to
 * their accumulators before their epilogue.  The weights may have any sign and zero columns; NULL = ones.  They are per leaf AND
 * per column because the back-propagation of sum_q log p_tree(Y[:, q]) weighs a leaf differently for every column.
 * Needs a fit and a dsmgp_solve_targets on the CURRENT fit (DSMGP_E_STATE otherwise).  DSMGP_E_ARG: grad_out NULL, stride smaller
 * than a hyper-vector, a non-finite weight, and where dsmgp_gradients refuses (ArdSE with the option on and D > 35).
 * The mask of dsmgp_set_gradient_leaves does not apply and is left as it is.  Leaves whose fit reported info != 0 get a NaN row.
 * Nothing another entry point reads is written: dsmgp_fit's outputs, dsmgp_gradients, dsmgp_loo*, dsmgp_predict_*,
 * dsmgp_targets_fetch and dsmgp_predict_targets return the same bits before and after.  Sums run in a fixed order, no atomics: the
 * same bits from call to call, and with one lane and with two wherever both fits leave the same factor bits.
 * Memory: A takes npad Qpad doubles per leaf in an arena of its own, allocated on first use (from the reserved pool when there is
 *   one; DSMGP_E_NOMEM with a usable context when it does not fit), NOT counted by dsmgp_estimate_bytes / dsmgp_memory, dropped
 *   where the arena of dsmgp_solve_targets is dropped.  seconds: device time of the call. */
int dsmgp_mll_columns_gradients(dsmgp_ctx* ctx, double* grad_out /* L x stride */, int32_t stride,
                            const double* col_weight /* L x Q column-major, ld = L; NULL = ones */,
                            double* seconds /* may be NULL */);
/* The same call under the name of the feature, for C and C++ callers (an inline alias, not a symbol of the library: the library
 * exports exactly three symbols with the word of the feature in their name, the three above, and bindings that resolve symbols
 * at run time -- Python, Julia -- use dsmgp_mll_columns_gradients). */
static inline int dsmgp_targets_gradients(dsmgp_ctx* ctx, double* grad_out, int32_t stride, const double* col_weight,
                                          double* seconds) {
    return dsmgp_mll_columns_gradients(ctx, grad_out, stride, col_weight, seconds);
}

/* Gradients of the predictive means of the columns of dsmgp_solve_targets with respect to the test point -- the Jacobian of the
 * vector-valued predictive mean: for every (leaf, routed test row t) entry e of dsmgp_predict_fetch, in its order, every input
 * dimension d and every column q,
 *   dmu_out[e + d * ld + q * ld * D] = d mu_q / d x_{t,d} = sum_{i < n} A_iq g_d(t, i),   g_d(t, i) = dk(x_t, x_i) / dx_{t,d},
 * A = K_y^-1 (Y - m) (column q of the arena of dsmgp_mll_columns_gradients, same kernel and same bits) and g_d exactly the per-kind
 * derivatives documented at dsmgp_predict_gradients, for all eleven kinds and any D.  Slice q has the layout of
 * dsmgp_predict_gradients' dmu_out; with Q = 1, Y = y and the leaf means it is that call's dmu_out to rounding (another kernel:
 * for Q columns the sum is a matrix product per dimension on the f64 matrix cores, the derivatives made in registers).
 * The variance does not depend on the targets: d var / d x is dsmgp_predict_gradients' dvar_out for every column, and this call
 * does not compute it.
 * Needs BOTH dsmgp_solve_targets and dsmgp_predict_run on the CURRENT fit, on either route to K_tn L^-T (DSMGP_E_STATE otherwise).
 * dmu_out NULL or ld < route_total: DSMGP_E_ARG.  No routed rows at all: success, nothing written.  Leaves whose fit reported
 * info != 0 get NaN in all their entries, the others are unaffected.  A COPY leaf uses its own A and its source's L^-T.
 * A needs L^-T of every factor owner: read as it is or filled here, by the rule of dsmgp_loo, and what that call says about
 * dsmgp_gradients and the mask of dsmgp_set_gradient_leaves holds here too (both are left exactly as they are; the mask does not
 * apply).  Nothing another entry point reads is written: dsmgp_predict_fetch, dsmgp_predict_cov, dsmgp_predict_targets,
 * dsmgp_targets_fetch, dsmgp_gradients, dsmgp_loo*, dsmgp_predict_gradients and dsmgp_mll_columns_gradients return the same bits
 * before and after.  Sums run in a fixed order, no atomics: the same bits from call to call, column q is the same bits whatever Q
 * is and whatever the other columns hold, and a test row listed twice gets identical rows.
 * Memory: A as in dsmgp_mll_columns_gradients; the output (route_total x D x Q doubles) and the partial sums (128 D Qpad doubles per
 *   128 routed rows of a leaf and per 1024 of its training rows) in buffers of this call's own, allocated on first use, NOT counted
 *   by dsmgp_estimate_bytes / dsmgp_memory, dropped with the test set, the leaf table and dsmgp_release.
 * seconds (may be NULL): device time of the call. */
int dsmgp_predict_columns_gradients(dsmgp_ctx* ctx, double* dmu_out /* route_total x D x Q */, int64_t ld,
                                    double* seconds /* may be NULL */);
/* The same call under the name of the feature, for C and C++ callers (an inline alias, not a symbol of the library, like
 * dsmgp_targets_gradients above). */
static inline int dsmgp_predict_targets_gradients(dsmgp_ctx* ctx, double* dmu_out, int64_t ld, double* seconds) {
    return dsmgp_predict_columns_gradients(ctx, dmu_out, ld, seconds);
}

/* Leave-one-out cross-validation of the columns of dsmgp_solve_targets on the one factorisation (GPML eqs. 5.10-5.13 per column,
 * the mean and the hyper-parameters held fixed).  With K_y the matrix the fit factorised, G = K_y^-1, d = diag G and a_q =
 * G (y_q - m_q) (column q of A, the arena of dsmgp_mll_columns_gradients, same kernel and same bits):
 *   mu_iq = y_iq - a_iq / d_i,   var_i = 1 / d_i (the same for every column: dsmgp_loo's var_out to the bit),
 *   lpd_q = sum_i -(log 2pi - log d_i + a_iq^2 / d_i) / 2 .
 * dsmgp_loo_columns: mu_out is obs_ptr[L] x Q column-major with leading dimension ld >= obs_ptr[L], rows in obs_idx order as for
 *   dsmgp_loo; var_out obs_ptr[L]; lpd_out L x Q (ld = L).  Any of the three may be NULL.  Column q of mu_out and lpd_out is the
 *   same bits whatever Q is and whatever the other columns hold.
 * dsmgp_loo_columns_gradients: grad_out[l * stride + j] = sum_q col_weight[l + q L] d lpd_out[l + q L] / d theta_j in the layout
 *   of dsmgp_gradients, EVERY component the true derivative as dsmgp_loo_gradients defines them for all eleven kinds (no factor
 *   sigma for IsoSE; true ArdSE dl whatever DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT says, refused above 35 dimensions; an iso Matern's
 *   dl summed over d; the rational quadratic da slot; 0 in the dummy slot of the linear kinds; dnoise = 2 exp(2 logNoise) tr M;
 *   zeros past the hyper-vector).  With s = sum_q c_q,
 *     sum_q c_q dlpd_q / dtheta = sum_rc M_rc (dK_y / dtheta)_rc,   M = 1/2 sum_q c_q (u_q a_q^T + a_q u_q^T) - H H^T,
 *     u_q = G (a_q / d),   H = G diag(sqrt W),   W_i = (s + sum_q c_q a_iq^2 / d_i) / (2 d_i) :
 *   the diagonal weight is linear in the column, so ONE G and ONE H H^T contraction serve every column, plus a rank-2Q term the
 *   contraction kernels add to their accumulators and O(n^2 Q) for U = [u_q].  The weights must be finite and >= 0 (sqrt W has to
 *   exist; the tree back-propagation produces such weights); NULL = ones.  A leaf whose weights are all zero gets a row of zeros.
 *   lpd_out (L x Q, may be NULL): dsmgp_loo_columns' table, the same bits.
 * Both need a fit and a dsmgp_solve_targets on the CURRENT fit (DSMGP_E_STATE otherwise).  DSMGP_E_ARG: grad_out NULL, a stride
 * smaller than a hyper-vector, ld < obs_ptr[L], a non-finite or negative weight.  d and L^-T come by dsmgp_loo's rule (read when
 * the arena holds this fit's, filled otherwise; what that call says about dsmgp_gradients and the mask holds here).  Leaves
 * whose fit reported info != 0 get NaN rows and NaN lpd / mu / var, the others are unaffected.  A COPY leaf reads its source's d
 * and L^-T and has targets, mean and weights of its own.
 * Nothing another entry point reads is written: dsmgp_fit's outputs, dsmgp_gradients, dsmgp_loo*, dsmgp_predict_*,
 * dsmgp_targets_fetch, dsmgp_predict_targets and dsmgp_mll_columns_gradients return the same bits before and after.  Sums run in a
 * fixed order, no atomics: the same bits from call to call, and with one lane and with two wherever both fits leave the same
 * factor bits.
 * Memory (gradients): H takes npad^2 doubles per leaf and U npad Qpad, in arenas of their own, allocated on first use (from the
 *   reserved pool when there is one; DSMGP_E_NOMEM with a usable context when they do not fit), NOT counted by
 *   dsmgp_estimate_bytes / dsmgp_memory, dropped where the arena of dsmgp_solve_targets is dropped.  seconds: device time. */
int dsmgp_loo_columns(dsmgp_ctx* ctx, double* mu_out /* obs_ptr[L] x Q column-major */, int64_t ld,
                      double* var_out /* obs_ptr[L] */, double* lpd_out /* L x Q, ld = L */, double* seconds /* may be NULL */);
int dsmgp_loo_columns_gradients(dsmgp_ctx* ctx, double* grad_out /* L x stride */, int32_t stride,
                                const double* col_weight /* L x Q column-major, ld = L, >= 0; NULL = ones */,
                                double* lpd_out /* L x Q, ld = L; may be NULL */, double* seconds /* may be NULL */);

/* ---- predict(model, x): sum/product aggregation of the leaf moments over the leaves every test row visits, on the
 *      moments the last dsmgp_predict_run left in HBM (replaces the host recursions of src/common.jl:134-149,198-302).
 *      family  DSMGP_AGG_MIXTURE  DSMGP (_predict / _minpredict, :134-143,151-196,275-302): leaf_coef[l] = W_l, the product of the
 *                                 sum-node weights exp(logweights) on leaf l's path; mu = sum W mu_l,
 *                                 var = sum W sigma2_l + sum W mu_l^2 - mu^2 with sigma2 <= 0 -> 1e-8 (:137)
 *              DSMGP_AGG_POE / DSMGP_AGG_GPOE   (:145-149,198-222): leaf_coef[l] = beta_l (1, resp. 1/#root children)
 *              DSMGP_AGG_RBCM     (:224-241): leaf_group[l] = root child of leaf l (n_groups of them);
 *                                 prior_kernel_id = kernel id of the model's first leaf (leftGP, :227)
 *      plain != 0: the root is a single GP (predict(node::GPNode), :175-179).
 *      dsmgp_aggregate = partial + finish on one context.  With leaves spread over ranks or contexts every holder
 *      calls dsmgp_aggregate_partial (partial_out: W x n_t sums, W = 3 mixture / 2 PoE, gPoE / 2 n_groups rBCM), the
 *      caller adds the partial sums (the multi-GPU exchange: one all-gather of W n_t doubles per rank) and hands the
 *      total to dsmgp_aggregate_finish.  mu_out / var_out (n_t each) may be NULL: results stay resident for dsmgp_scores.
 *      The partial sums, the total and the aggregated moments belong to the dsmgp_predict_run they were made from.
 *      A later dsmgp_fit or dsmgp_set_hyper makes them stale, like the moments themselves (the rBCM finish would also read
 *      the prior variance of the NEW hyper-parameters): dsmgp_aggregate_finish, dsmgp_aggregate_exchange and dsmgp_scores then
 *      return DSMGP_E_STATE until dsmgp_predict_run and dsmgp_aggregate_partial (or dsmgp_aggregate) have run on the current fit. */
#define DSMGP_AGG_MIXTURE 0
#define DSMGP_AGG_POE     1
#define DSMGP_AGG_GPOE    2
#define DSMGP_AGG_RBCM    3
int dsmgp_aggregate(dsmgp_ctx* ctx, int32_t family, const double* leaf_coef /* L */, const int32_t* leaf_group /* L or NULL */,
                    int32_t n_groups, int32_t plain, int32_t prior_kernel_id, double* mu_out, double* var_out);
int dsmgp_aggregate_partial(dsmgp_ctx* ctx, int32_t family, const double* leaf_coef, const int32_t* leaf_group,
                            int32_t n_groups, double* partial_out /* W x n_t or NULL */);
int dsmgp_aggregate_finish(dsmgp_ctx* ctx, const double* partial_in /* NULL: the context's own sums */, int32_t plain,
                           int32_t prior_kernel_id, double* mu_out, double* var_out);
/* ---- Input gradients of the aggregated prediction: d mu / d x and d var / d x of predict(model, x) per test row, from the
 *      per-entry gradients of dsmgp_predict_gradients without leaving HBM (no reference counterpart; the tree is piecewise
 *      constant in x, so this is the gradient inside the row's region).  Family, leaf_coef and leaf_group are those of the last
 *      dsmgp_aggregate_partial.  Needs the aggregated moments of the current prediction, dsmgp_aggregate or
 *      dsmgp_aggregate_finish (DSMGP_E_STATE otherwise, and again after a later dsmgp_fit, dsmgp_set_hyper, dsmgp_predict_run,
 *      dsmgp_aggregate_partial or dsmgp_aggregate_finish).  The per-entry gradients are read where both halves are this
 *      prediction's already (a dsmgp_predict_gradients with dvar_out); otherwise the device part of that call runs first.
 *      A dsmgp_predict_gradients with dvar_out writes them again: between dsmgp_aggregate_gradients_partial and _finish it
 *      makes the sums stale (DSMGP_E_STATE from _finish until the partial call has run again).
 *        mixture   dmu = sum W dmu_l, dvar = sum W dvar'_l + 2 sum W (mu_l - mu) dmu_l (plain: the first sum alone); dvar'_l = 0
 *                  where the moments clamp the leaf variance (sigma2_l <= 0).  The second sum is centred on the aggregated mean.
 *        PoE/gPoE  T = sum beta / sigma2_l, P = sum beta mu_l / sigma2_l; dT = -sum beta dvar_l / sigma2_l^2,
 *                  dP = sum beta (dmu_l / sigma2_l - mu_l dvar_l / sigma2_l^2); dmu = (dP - mu dT) / T, dvar = -dT / T^2
 *        rBCM      per group g that saw the row T_g, P_g, dT_g, dP_g with beta = 1; s = k(x, x) + noise of prior_kernel_id,
 *                  ds/dx_d = 2 x_d / l_d^2 for the linear kinds and 0 for the others; beta_g = (log s + log T_g) / 2,
 *                  dbeta_g = (ds / s + dT_g / T_g) / 2; C = 1 / s + sum_g beta_g (T_g - 1 / s), m = sum_g beta_g P_g,
 *                  dC = -ds / s^2 + sum_g [dbeta_g (T_g - 1 / s) + beta_g (dT_g + ds / s^2)], dm = sum_g (dbeta_g P_g + beta_g dP_g);
 *                  dmu = (dm - mu dC) / C, dvar = -dC / C^2
 *      dsmgp_aggregate_gradients = partial + finish on one context.  The sums are Wg x n_t in [k][row] planes, Wg = 3 D
 *      (mixture: sum W dmu_d | sum W dvar'_d | sum W (mu_l - mu) dmu_d), 2 D (PoE, gPoE: dT_d | dP_d) or 2 n_groups D (rBCM:
 *      per group dT_gd | dP_gd).  With leaves spread over contexts the caller first hands the TOTAL moment sums to every holder
 *      (dsmgp_aggregate_finish with partial_in); after that the holders' gradient sums are additive: the caller adds them and
 *      hands the total to dsmgp_aggregate_gradients_finish of one holder.  dmu_out / dvar_out: n_t x D column-major, ld >= n_t
 *      (DSMGP_E_ARG otherwise); either may be NULL, the other is the same bits.  A row's entries are added in ascending entry
 *      order by one thread: the same bits from call to call.  A row that reaches a failed leaf gets NaN, the others are not
 *      affected; a row without entries gets what the formulas give.  `seconds` (may be NULL): the device time of the
 *      partial-sum kernel (the finish kernel is not timed), with that of the per-entry gradients where they had to be made.
 *      partial_in is written over the context's own sums: a later finish with NULL on that holder finishes the same total.  The buffers are allocated on first use and are not part
 *      of dsmgp_estimate_bytes / dsmgp_memory; DSMGP_E_NOMEM leaves the context usable.  dsmgp_predict_fetch,
 *      dsmgp_predict_gradients, dsmgp_aggregate* and dsmgp_scores return the same bits before and after. */
int dsmgp_aggregate_gradients_partial(dsmgp_ctx* ctx, double* partial_out /* Wg x n_t, may be NULL */, double* seconds);
int dsmgp_aggregate_gradients_finish(dsmgp_ctx* ctx, const double* partial_in /* NULL: the context's own sums */, int32_t plain,
                                     int32_t prior_kernel_id, double* dmu_out, double* dvar_out, int64_t ld);
int dsmgp_aggregate_gradients(dsmgp_ctx* ctx, int32_t plain, int32_t prior_kernel_id, double* dmu_out, double* dvar_out,
                              int64_t ld, double* seconds);
/* ---- The same two aggregations for every column of the last dsmgp_solve_targets, on one context (no partial / finish split).
 *      dsmgp_aggregate_columns is dsmgp_aggregate per column: mu_out / var_out are n_t x Q column-major, ld >= n_t (DSMGP_E_ARG
 *      otherwise), either may be NULL.  Needs BOTH dsmgp_solve_targets and dsmgp_predict_run on the CURRENT fit (DSMGP_E_STATE
 *      otherwise); the per-entry means of the columns are read where dsmgp_predict_targets left them for this prediction and
 *      these columns, otherwise the device part of that call runs first.  One coefficient per leaf serves all columns; the leaf
 *      variance is shared, so var_out differs per column only for the mixture.
 *      dsmgp_aggregate_columns_gradients needs dsmgp_aggregate_columns on the current prediction and columns (DSMGP_E_STATE
 *      otherwise) and uses its family, coefficients and groups; dmu_out / dvar_out hold element [r + d*ld + q*ld*D], ld >= n_t.
 *      It reads dmu of dsmgp_predict_columns_gradients and dvar of dsmgp_predict_gradients, running either device part when it
 *      is not current.  Formulas, clamps, skipped groups, NaN rows and rows without entries: as for the single y above.
 *      One thread per (test row, column) adds the row's entries in ascending entry order and never reads another column: the
 *      same bits from call to call, and column q is the same bits whatever Q is and whatever the other columns hold.  The state
 *      of these calls is their own: dsmgp_aggregate_finish, dsmgp_aggregate_gradients* and dsmgp_scores answer as before (a
 *      dsmgp_predict_gradients device part that had to run makes gradient SUMS stale, as said above).  Buffers: on first use,
 *      not part of dsmgp_estimate_bytes / dsmgp_memory.  `seconds` (may be NULL): the aggregation kernel plus the device
 *      parts that had to run. */
int dsmgp_aggregate_columns(dsmgp_ctx* ctx, int32_t family, const double* leaf_coef, const int32_t* leaf_group, int32_t n_groups,
                            int32_t plain, int32_t prior_kernel_id, double* mu_out, double* var_out, int64_t ld, double* seconds);
int dsmgp_aggregate_columns_gradients(dsmgp_ctx* ctx, int32_t plain, int32_t prior_kernel_id, double* dmu_out, double* dvar_out,
                                      int64_t ld, double* seconds);
/* ---- score functions of src/scorefunctions.jl:6-16 on the aggregated prediction still in HBM:
 *      out[5] = { mse, sse (std(se)/sqrt(n)), mae, sae, nlpd } */
int dsmgp_scores(dsmgp_ctx* ctx, const double* y_test /* n_t */, double* out /* 5 */);

/* ---- updategradients!(gp) + grad vector of src/gaussianprocess.jl:165-178,185-217 per leaf.
 *      grad_out[l*stride + j], j over [dl..., ds, dnoise] (reference order, src/gaussianprocess.jl:212-214),
 *      reproducing the reference's scaling and ArdSE dl == 0.
 *      ArdLinear: [dl_1..dl_D, 0, dnoise] with the true derivative dl_d = 0.5 tr((alpha alpha^T - K_y^-1) dK/dlog l_d)
 *      = -((alpha . x_d)^2 - x_d^T K_y^-1 x_d) / l_d^2 (x_d = column d of the leaf's inputs; n^2 D flops per leaf on the L^-T
 *      of the trace term, any D; DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT does not apply).  With all l_d equal their sum is
 *      IsoLinear's dl (src/kernels.jl:196-200).
 *      ArdSEProduct: [dl_1..dl_D, ds, dnoise], all true derivatives (no SURVEY F7 factor): dl_d = 0.5 sum_rc W_rc K_rc
 *      (x_rd - x_cd)^2 / l_d^2 and ds = tr(W K), W = alpha alpha^T - K_y^-1, K without noise; any D.
 *      Matern (kinds 5-8): iso [dl, ds, dnoise], ARD [dl_1..dl_D, ds, dnoise], all true derivatives (no SURVEY F7 factor):
 *      dl_d = 0.5 sum_rc W_rc sigma^2 exp(-s) c(s) s_d^2 with s_d^2 = 2 nu (x_rd - x_cd)^2 / l_d^2, c(s) = 1 (nu = 3/2) or
 *      (1 + s) / 3 (nu = 5/2) -- finite at s = 0, nothing divides by r; the iso dl is the sum over d; ds = tr(W K); any D.
 *      Rational quadratic (kinds 9, 10): iso [dl, da, ds, dnoise], ARD [dl_1..dl_D, da, ds, dnoise], all true derivatives:
 *      dl_d = 0.5 sum_rc W_rc K_rc / (1 + w) (x_rd - x_cd)^2 / l_d^2 (the iso dl is the sum over d),
 *      da = 0.5 sum_rc W_rc K_rc alpha (w / (1 + w) - log1p(w)), ds = tr(W K); any D.  Zeros past the hyper-vector. */
int dsmgp_gradients(dsmgp_ctx* ctx, double* grad_out, int32_t stride);
/* Restricts dsmgp_gradients to the leaves with active[l] != 0 (NULL: every leaf again; a new leaf table resets it): the rows
 * of the others come back as zeros, and neither L^-T nor the contraction tiles of leaves nobody asked for are computed (a
 * COPY leaf's source and every active leaf's factor owner are included as needed).  finetune! weights leaf l's gradient by
 * the overlap D[j, l] while it moves leaf j's vector (src/optimize.jl:101, src/finetuning.jl:34-57): all but the overlapping
 * leaves are multiplied by zero there.  Changing the set rebuilds the task lists of the gradient pass (the L^-T arena stays). */
int dsmgp_set_gradient_leaves(dsmgp_ctx* ctx, const int32_t* active /* L flags, or NULL */);
/* Leave-one-out cross-validation of every leaf GP (Rasmussen & Williams, GPML 5.4.2, eqs. 5.10-5.12), the mean and the
 * hyper-parameters held fixed.  With K_y = K + (exp(2 logNoise) + 1e-8) I the matrix the fit factorises, d_i = [K_y^-1]_ii
 * and alpha = K_y^-1 (y - m), for observation i of a leaf (the order of its segment of obs_idx):
 *   mu_out[obs_ptr[l] + i]  = y_i - alpha_i / d_i   -- the mean at x_i of the same GP fitted without row i,
 *   var_out[obs_ptr[l] + i] = 1 / d_i               -- its predictive variance there with noise, plus the 1e-8 jitter,
 *   lpd_out[l] = sum_i -(log 2pi + log var_i + (y_i - mu_i)^2 / var_i) / 2   -- the leaf's LOO log predictive density,
 * added in a fixed order: results are the same to the bit from call to call.  Any of the three may be NULL.
 * Needs a fit (DSMGP_E_STATE otherwise).  d comes from L^-T of every factor owner, the arena dsmgp_gradients fills (same size,
 * same DSMGP_E_NOMEM when it does not fit): it is read as it is when dsmgp_loo, or a dsmgp_gradients pass that inverted every
 * owner, already filled it for the current fit, else filled here with the gradient pass's task lists.  dsmgp_gradients itself
 * inverts on every call, as before, and this call changes nothing about it: under a mask of dsmgp_set_gradient_leaves that
 * leaves owners out, the sweep runs over lists of this call's own (every owner) which are dropped before it returns, so the
 * next dsmgp_gradients builds and runs the mask's lists exactly as without this call (same work, same bits; the price is one
 * more build of those lists on the host).  The mask does not change the LOO results.  Because the lists are the gradient
 * pass's, the call fails like dsmgp_gradients (DSMGP_E_ARG) where that cannot build them: ArdSE leaves with
 * DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT = 1 and more input dimensions than the contraction stages.
 * A COPY leaf takes its source's d and its own alpha, y and mean.  Leaves whose fit reported info != 0 get NaN in all three
 * outputs; the others are unaffected.  seconds (may be NULL): device time of the call -- what is left to complete after this
 * fit of the diagonal-block inverses and of alpha, the inversion when it runs, and the two LOO kernels (there is no
 * dsmgp_timings slot for it).
 * Its device scratch (the row sums of L^-T in slices, about 1/256 of the L^-T arena, and 2 obs_ptr[L] + L doubles) is
 * allocated on first use and is NOT counted by dsmgp_estimate_bytes(with_gradients = 1) / dsmgp_memory, which cover the L^-T
 * arena only; it is dropped with the leaf table and dsmgp_release. */
int dsmgp_loo(dsmgp_ctx* ctx, double* mu_out, double* var_out /* obs_ptr[L] each, in obs_idx order; may be NULL */,
              double* lpd_out /* L; may be NULL */, double* seconds /* may be NULL */);
/* k-fold cross-validation of every leaf GP from the current fit, the mean and the hyper-parameters held fixed: whole groups of
 * rows held out at once, without refitting.  fold[r] is the label of training row r, -1 .. K - 1.  For leaf l and label k the
 * block is F(l, k) = { i : fold[obs_idx[obs_ptr[l] + i]] == k }, positions ascending.  With G = K_y^-1 and alpha = G (y - m)
 * (dsmgp_loo's K_y), the leaf fitted without the rows of F predicts them jointly as (the multiple-fold residuals, e.g.
 * Ginsbourger & Schaerer 2021)
 *   mu_F = y_F - G_FF^-1 alpha_F,   Sigma_F = G_FF^-1,
 *   lpd_F = log N(y_F | mu_F, Sigma_F) = -1/2 alpha_F^T G_FF^-1 alpha_F + 1/2 log det G_FF - (|F| / 2) log 2 pi.
 * mu_out[obs_ptr[l] + i] and var_out[obs_ptr[l] + i] for i in F(l, k) are mu_F and diag Sigma_F, in dsmgp_loo's layout and
 * meaning (var carries the noise and the fit's 1e-8 jitter); lpd_out[l + k L] is the joint density.  Singleton blocks are
 * dsmgp_loo's formulas; one block that holds the whole leaf gives mu = m, Sigma = K_y and lpd = the fit's mll.
 * An empty block gives lpd = 0 and info = 0.  A row with label -1 is never held out: it belongs to no block, trains every fold, and
 * its mu and var come back as NaN (K = 1 with labels 0 / -1 scores a validation subset from one full fit).  Rows that no leaf
 * holds are ignored.  info_out[l + k L]: 0 = success; -1 = a leaf whose fit reported info != 0 (all of that leaf's outputs are
 * NaN); j > 0 = the leading minor of order j of G_FF is not positive definite, LAPACK's convention (only that block is NaN;
 * defensive: G_FF is a principal submatrix of an SPD matrix).  Other leaves and blocks are unaffected.  Any output may be NULL;
 * with var_out = NULL the inverse factors behind the variances are neither computed nor allocated.
 * A COPY leaf has its source's observation list: the blocks are formed and factorised once per factor owner and the COPY leaf
 * applies them to its own alpha, y and mean.  A PREFIX leaf owns its factor.
 * DSMGP_E_STATE: no fit on the current leaf table and hyper-parameters.  DSMGP_E_ARG: fold is NULL, K < 1 or K > 65535, a label
 * outside -1 .. K - 1 on ANY of the N rows (a row that no leaf holds is ignored in every other respect, but its label must be a
 * label: what the call accepts depends on neither the leaf table nor on which fits succeeded), or where dsmgp_loo refuses because the lists of the inversion cannot be built.  DSMGP_E_NOMEM: the arenas do
 * not fit; the context stays usable.  L^-T follows dsmgp_loo's rule: read when the arena holds this fit's, filled otherwise; the
 * mask of dsmgp_set_gradient_leaves does not apply and is left as it is, and dsmgp_gradients behaves exactly as before.  Nothing
 * another entry point reads is written: dsmgp_fit's outputs, dsmgp_loo*, dsmgp_gradients, dsmgp_predict_*, dsmgp_targets_fetch
 * and dsmgp_aggregate* return the same bits before and after.  Sums run in a fixed order with no atomics: the same bits from
 * call to call, and a block's results depend on its row set only -- renumbering the labels, or changing the labels of rows
 * outside the leaf, leaves mu, var and the block's lpd bit-identical.  The call keeps no product: labels arrive per call and
 * nothing is cached but L^-T.
 * Memory, per factor owner with blocks of m rows (mpad = m rounded up to 128): mpad^2 doubles per block for G_FF and its factor,
 * as much again for the inverse factors when var_out is given, 128 mpad for the inverted diagonal blocks, the packed rows of one
 * label at a time (mpad x npad per block, the largest label's total: about 1 / K of the L^-T arena for balanced folds), and
 * 2 obs_ptr[L] + L K doubles of results (the host plans with one counter per label and one record per non-empty block, not with an
 * L x K table; the caller's own lpd_out and info_out are L x K).  Grow-only, allocated on first use (the arenas from the reserved pool when there is
 * one), NOT counted by dsmgp_estimate_bytes / dsmgp_memory, dropped with the leaf table and dsmgp_release.
 * seconds (may be NULL): device time of the call. */
int dsmgp_kfold(dsmgp_ctx* ctx, const int32_t* fold /* N: label of every training row, -1 .. K-1 */, int32_t K,
                double* mu_out /* obs_ptr[L], may be NULL */, double* var_out /* obs_ptr[L], may be NULL */,
                double* lpd_out /* L x K column-major, ld = L, may be NULL */,
                int32_t* info_out /* L x K, ld = L, may be NULL */, double* seconds /* may be NULL */);
/* Device seconds of the last successful dsmgp_kfold, split: out[0] the L^-T inversion with what was left to complete of the
 * diagonal-block inverses and of alpha (0 when the arena was current: that completion then counts with out[1]), out[1] packing
 * the held-out rows and forming G_FF, out[2] the factorisation, out[3] the inverse factors, solves and moments.  The four add up
 * to the call's `seconds`. */
int dsmgp_kfold_seconds(dsmgp_ctx* ctx, double* out /* 4 */);
/* Bytes the context holds for dsmgp_kfold right now: out[0] the packed rows of one label, out[1] the block factors, out[2] the
 * inverted diagonal blocks and the panel solves' scratch, out[3] the inverse factors (0 until a call with var_out asks for them).
 * All 0 before the first call and after the leaf table or dsmgp_release dropped them. */
int dsmgp_kfold_stats(dsmgp_ctx* ctx, int64_t* out /* 4 */);
/* Gradients of the leaf's LOO log predictive density lpd_l (dsmgp_loo's lpd_out[l]) with respect to its log-scale
 * hyper-parameters (GPML 5.4.2, eq. 5.13), the mean held fixed: what makes leave-one-out a training objective.  With G = K_y^-1,
 * d = diag G, alpha = G (y - m):
 *   dlpd / dtheta = sum_rc M_rc (dK_y / dtheta)_rc,   M = (u alpha^T + alpha u^T) / 2 - H H^T,
 *   u = G (alpha / d),   H = G diag(sqrt w),   w_i = (1 + alpha_i^2 / d_i) / (2 d_i).
 * grad_out[l * stride + j], j over [dl..., ds, dnoise] ([dl..., da, ds, dnoise] for the rational quadratic kinds) -- the layout
 * of dsmgp_gradients -- and EVERY component is the true
 * derivative, for all kinds: no factor sigma for IsoSE, true per-dimension length-scale derivatives for the additive ArdSE
 * whatever DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT says (ArdSE leaves with more input dimensions than the contraction stages, 35:
 * DSMGP_E_ARG), the sum over the dimensions in ascending order for an iso Matern kind, 0 in the dummy variance slot of the
 * linear kinds, zeros past the hyper-vector.  Signal variances and the SE / Matern length-scales are contracted with M
 * directly on the device; IsoLinear's dl = -2 (tr(M K_y) - c tr M) comes from the trace identity (it cancels when the signal
 * is weak against c = exp(2 logNoise) + 1e-8), dnoise = 2 exp(2 logNoise) tr M.
 * lpd_out (L, may be NULL): dsmgp_loo's lpd_out, the same bits -- this call runs dsmgp_loo first and inherits what it says
 * about L^-T, the mask of dsmgp_set_gradient_leaves (it does not apply) and dsmgp_gradients (left exactly as it is).
 * Needs a fit (DSMGP_E_STATE); stride smaller than a hyper-vector: DSMGP_E_ARG.  Leaves whose fit reported info != 0 get a
 * NaN row and NaN lpd, the others are unaffected.  A COPY leaf with its source's mean takes its source's row.  Results are
 * the same to the bit from call to call.  seconds (may be NULL): device time of the call, dsmgp_loo's included (there is no
 * dsmgp_timings slot for it).
 * Memory: one more arena for H, npad^2 doubles for every leaf but the COPY leaves with their source's mean -- the size of the
 * L^-T arena (npad^2 per factor owner) plus npad^2 for every COPY leaf with a mean of its own, which owns no L^-T --, plus
 * 4 npad doubles per leaf and the partial sums, allocated on first use (the arena from the reserved pool when there is one;
 * DSMGP_E_NOMEM with a usable context when it does not fit), dropped with the leaf table and dsmgp_release, and NOT counted
 * by dsmgp_estimate_bytes / dsmgp_memory.  Cost per leaf: n^3 / 3 flops for the tiles of G and n^3 for H H^T. */
int dsmgp_loo_gradients(dsmgp_ctx* ctx, double* grad_out /* L x stride */, int32_t stride,
                        double* lpd_out /* L; may be NULL */, double* seconds /* may be NULL */);
/* Options.  DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT: 0 (default) = ArdSE length-scale gradients exactly as the reference
 * computes them, i.e. identically zero (`precomp * K .* (p/ls[d])` parses as `(precomp*K) .* (p/ls[d])` and p has a zero
 * diagonal, src/kernels.jl:161: train!/finetune! never move ARD length-scales); 1 = the true derivative of the
 * log-marginal, dl_d = 0.5 tr((alpha alpha^T - K_y^-1) dK/dlog l_d) with dK/dlog l_d = sigma^2 exp(-u_d^2/2l_d^2) u_d^2/l_d^2
 * of the additive kernel (no extra factor sigma; costs the contraction pass, n^3/3 flops per leaf; D <= 35). */
#define DSMGP_OPT_ARD_LENGTHSCALE_GRADIENT 1
/* DSMGP_OPT_FUSED_GRAM: 1 (default) = the update tasks of fit! evaluate the kernel function for their tile themselves
 * (same operations as the Gram launch, bit-identical values) instead of reading what a Gram launch wrote, which then
 * covers block column 0 only (D <= 32; above that the option has no effect); 0 = every lower tile of K_y goes through
 * memory first.  Changing it discards the leaf plan and a registered test set: set it before dsmgp_set_test. */
#define DSMGP_OPT_FUSED_GRAM 2
/* DSMGP_OPT_FUSED_STEPS: 1 (default) = a block step of the factorisation whose diagonal blocks alone fill the chip (more
 * leaves in the step than CUs: depth >= 3 trees, large PoE models), and every shallow step (K <= 512), runs as two
 * launches -- the diagonal block's task also updates its tile, the tasks of the tiles below update AND solve them, each
 * tile written once (the per-step order of src/AdvancedCholeskey.jl:161-171, batched over leaves); 0 = every step as
 * update / diagonal block / panel solve launches.  Diagonal blocks come out bit-identical either way; the tiles below
 * agree to rounding (a fused task accumulates the product on -k(row, col) where the classic update subtracts the finished
 * product from k(row, col)).  Needs DSMGP_OPT_FUSED_GRAM (D <= 32); changing it discards the leaf plan and a registered
 * test set. */
#define DSMGP_OPT_FUSED_STEPS 3
/* DSMGP_OPT_DIAG_IN_UPDATE: 1 (default) = where two consecutive block steps are classic, the diagonal block runs one step
 * ahead of the panel below it (the lookahead of a blocked factorisation, src/AdvancedCholeskey.jl:161-171 per step): the update
 * launch of step k - 1 also updates tile (k, k) over the columns it covers, and the update launch of step k carries a task
 * per leaf that applies the last block column, factorises the block and inverts it beside the updates of the tiles below,
 * so the panel-solve launch finds L_kk, Dinv_k and z_k ready and the per-step chain loses a dependent launch (35 us x every
 * block step of the deepest leaf); 0 = update / reduce / diagonal block / panel solve launches one after the other.
 * Results agree to rounding (the diagonal tile's update is summed in two parts); a fit is bit-reproducible either way.
 * Needs DSMGP_OPT_FUSED_GRAM (D <= 32); changing it discards the leaf plan and a registered test set. */
#define DSMGP_OPT_DIAG_IN_UPDATE 4
/* DSMGP_OPT_FIT_GRAPH: 1 = while per-launch timing is off (dsmgp_set_profile 0) dsmgp_fit replays its launch sequence as a
 * captured hipGraph (captured on the first such fit of a plan, dropped with the plan, the test set or a re-allocated
 * kernel-parameter table).  Same kernels, same arguments, same results to the bit.  0 (default) = plain launches: what the
 * graph buys is the host-side cost between dependent launches, measured at 2 % of a single GP's 32-step chain (config 2: 2.50
 * -> 2.47 ms) and nothing elsewhere, and a capture does not tolerate other contexts being driven from concurrent host threads
 * in the same process. */
#define DSMGP_OPT_FIT_GRAPH 5
/* DSMGP_OPT_LANES: leaf lanes of a fit (src/fit.jl:88-119: the leaves are independent): 0 (default) = automatic -- two lanes from 8
 * sharing groups on (a source leaf with its COPY / PREFIX leaves is one group), one below (a single GP) -- 1 = one lane, 2 = two.
 * With two lanes the leaves are dealt longest-processing-time first into two halves with step lists, split-K workspace and HIP
 * stream of their own, joined at the end of the factorisation: one half's latency-bound launches (diagonal blocks, panel solves,
 * reduces) run under the other's update launches.  Per-leaf results agree to rounding with the one-lane schedule (a launch of half
 * the tiles cuts its tail along K differently: the order of a few additions per entry), a fit is bit-reproducible either way.
 * Changing it discards the leaf plan and a registered test set. */
#define DSMGP_OPT_LANES 6
int dsmgp_set_option(dsmgp_ctx* ctx, int32_t option, int32_t value);
/* leaf lanes of the current plan (DSMGP_OPT_LANES: 1 or 2; 0 = no plan yet: it is made by the first fit / set_test of a leaf table) */
int dsmgp_lanes(dsmgp_ctx* ctx, int32_t* lanes);

/* ---- inspection ------------------------------------------------------------------------------- */
/* kernelmatrix(kernel, x1, x2) (src/kernels.jl:15-18) through the same device code as the fit path */
int dsmgp_kernel_matrix(dsmgp_ctx* ctx, int32_t kernel_id, const double* x1, int64_t n1,
                        const double* x2, int64_t n2, double* K_out /* n1 x n2 */);
/* gp.cK.factors (lower triangle = L, strict upper = 0) and gp.alpha of one leaf; either may be NULL */
int dsmgp_download_factor(dsmgp_ctx* ctx, int32_t leaf, double* F /* n x n */, double* alpha /* n */);
/* hipEvent timing per launch: level 0 = totals only, 1 = the update launches of the factorisation (the dominant
 * kernel; what bench.py's roofline uses), 2 = every kernel category (adds event records between all launches;
 * also switched on by the environment variable DSMGP_PROFILE=1 at dsmgp_create -- the only environment variable the
 * product library reads besides DSMGP_STEPLOG / DSMGP_HOSTLOG (stderr logging); none of them changes results);
 * 3 = level 1 with the launches under the kernel instantiation names of level 0 (the timed launches of bench.py run as
 * tile_gemm_kernel_v2<false, 0, *> / tile_fused8_kernel<0>, every other launch as <false, 2, *> / <1> (sweeps) / <2>: a profiler's
 * per-kernel average of the first names is exactly the timed quantity) */
int dsmgp_set_profile(dsmgp_ctx* ctx, int32_t level);
int dsmgp_timings(dsmgp_ctx* ctx, double* out /* DSMGP_N_TIMINGS, seconds of the last fit/predict */);
/* work of the dominant kernel (the f64-MFMA Cholesky update) in the last fit: algorithmic flops over
 * all its launches (2*K per lower-triangle element of every block column, unpadded sizes) and the
 * number of launches */
int dsmgp_work(dsmgp_ctx* ctx, double* alg_flops_update, int32_t* n_update_launches);
/* the same for the tile_fused8_kernel launches of fused block steps (timing slot chol_fused): algorithmic flops of their
 * update part plus the triangular solves (c_k^2 per row below a diagonal block of c_k columns), and the number of launches.
 * dsmgp_work counts only the steps that run as update launches. */
int dsmgp_work_fused(dsmgp_ctx* ctx, double* alg_flops_fused, int32_t* n_fused_launches);
/* algorithmic flops of the two matrix passes of dsmgp_gradients (n^3/3 each per leaf) and the number of contraction tiles */
int dsmgp_work_gradients(dsmgp_ctx* ctx, double* alg_flops_inverse, double* alg_flops_contraction, int32_t* n_contraction_tiles);
/* Reserve one device pool of `bytes` (0 = drop it): while a pool exists, the large arenas of every following leaf
 * table (factors, inverse blocks, K_tn rows, L^-1 for gradients, split-K slabs) are carved out of it instead of being
 * allocated and freed per table -- the driver clears memory on allocation, ~5 s per 230 GB.  Used by the
 * factor-and-discard mode (hipabi.StreamingContext).  Drops the current leaf table's device state. */
int dsmgp_reserve(dsmgp_ctx* ctx, int64_t bytes);

/* streaming ("factor and discard"): drop every buffer that scales with the leaf sizes, keep data, leaf table,
 * schedule and hyper-parameters; the next dsmgp_fit rebuilds.  dsmgp_estimate_bytes sizes a leaf group beforehand. */
int dsmgp_release(dsmgp_ctx* ctx);
int64_t dsmgp_estimate_bytes(int32_t L, const int64_t* n, const int64_t* n_test /* may be NULL */, int32_t D,
                             int32_t with_gradients);
/* bytes of device memory the current leaf table needs / the device has free */
int dsmgp_memory(dsmgp_ctx* ctx, int64_t* needed, int64_t* free_bytes);

/* f64 MFMA issue-rate probe used for the roofline peak (bench.py): returns TFLOP/s of a register-only
 * v_mfma_f64_16x16x4_f64 loop over the whole chip */
int dsmgp_probe_f64_mfma(dsmgp_ctx* ctx, double* tflops);
/* out[0] TFLOP/s, out[1] shader cycles per MFMA per wave, out[2] shader clock (GHz) held in the loop,
 * out[3] = blocks_per_cu (256-thread workgroups per CU, i.e. waves per SIMD) */
int dsmgp_probe_f64_mfma_detail(dsmgp_ctx* ctx, int32_t blocks_per_cu, double* out);

/* Shader clock the chip holds under load (bench.py prints it beside the roofline: the f64 matrix peak scales with it).
 * start: a one-wave kernel on a stream of its own sleeps for `milliseconds` (<= 5000) of wall time beside whatever the context
 * launches meanwhile and counts shader cycles; returns at once.  read: waits for it; ghz = shader cycles per nanosecond over
 * the `milliseconds` it actually covered.  One sample at a time per context. */
int dsmgp_clock_sample_start(dsmgp_ctx* ctx, double milliseconds);
int dsmgp_clock_sample_read(dsmgp_ctx* ctx, double* ghz, double* milliseconds);

/* Host-only (no device): per leaf j the "main" leaf of the sharing schedule of src/fit.jl:78-86,
 * main[j] = argmax_i D[i,j] D[j,i] over the overlap matrix D of src/fit.jl:12-39 (first maximum, 0 if leaf j overlaps
 * no other leaf), and c_main[j] = number of observations leaf j shares with it -- computed from an inverted index
 * instead of the dense L x L matrix (18k leaves at depth 4).  Leaves as in dsmgp_set_leaves; one kernel id. */
int dsmgp_overlap_main(int32_t L, const int64_t* obs_ptr, const int64_t* obs_idx, int64_t N, int64_t* main_out,
                       int64_t* c_main_out);

/* Host-only: which test rows each leaf is asked to predict (the routing of predict, src/common.jl:181-196,275-292: a sum node
 * forwards its rows to every child, a split node to the first child k with x[d] <= s_k) -- the CSR that dsmgp_set_test takes.
 * The tree as flat arrays with the children of node i at first_child[i] .. first_child[i] + n_child[i] - 1 (root = node 0):
 * kind as in dsmgp_tree_export: 0 = region, i.e. leaf (leaf_id), 1 = split node (split_dim, ascending thresholds
 * thr[i * thr_ld + 0 .. n_child[i] - 1]), 2 = sum node.
 * x: n_t rows of D columns, element (row r, dimension d) at x[r * row_stride + d * col_stride].  route_ptr: n_leaves + 1 entries; route_idx: `capacity`
 * entries for the rows of every leaf, ascending (a row reaches at most as many leaves as the tree has below sum nodes along one
 * path: n_t times that bound always suffices).  DSMGP_E_ARG: malformed tree or a split dimension >= D (a tree of any width and depth is taken: the
 * walk's stack is sized by the tree); DSMGP_E_DOMAIN: a row
 * beyond the last threshold of a split node (the reference loops forever there; a NaN coordinate is beyond every threshold); DSMGP_E_NOMEM: capacity too small -- route_ptr and *n_routes_out are valid, route_idx
 * is not.  At depth 4 (18k leaves, 10k rows to 81 leaves each) the recursion over node objects took 0.09 s on the host, four
 * times the prediction sweep it feeds. */
int dsmgp_tree_route(int64_t n_nodes, const int8_t* kind, const int64_t* first_child, const int64_t* n_child,
                     const int64_t* split_dim, const double* thr, int64_t thr_ld, const int64_t* leaf_id, int64_t n_leaves,
                     const double* x, int64_t n_t, int64_t D, int64_t row_stride, int64_t col_stride, int64_t* route_ptr,
                     int64_t* route_idx, int64_t capacity, int64_t* n_routes_out);

/* ---- multi-GPU: the one exchange step of the path.  Leaves are independent, every rank (one process
 *      per GPU, one context each) fits and predicts its own shard; what crosses GPUs is one all-gather of per-leaf
 *      log-marginals after dsmgp_fit and one of the aggregation's partial sums after dsmgp_aggregate_partial, over RCCL
 *      (xGMI inside a node) on the context's stream.  librccl.so is dlopen'ed on first use.
 *      dsmgp_comm_unique_id: rank 0 obtains the 128-byte ncclUniqueId and hands it to the other ranks by whatever
 *      channel the host has (MPI.jl bcast, a file, the Distributed stdlib); every rank then calls dsmgp_comm_init.
 *      dsmgp_allgather: `count` doubles from every rank, recv[r * count ...] = rank r's block (host buffers; blocking). */
int dsmgp_comm_unique_id(char* id_out /* 128 bytes */);
int dsmgp_comm_init(dsmgp_ctx* ctx, int32_t rank, int32_t world, const char* id /* 128 bytes */);
int dsmgp_allgather(dsmgp_ctx* ctx, const double* send, int64_t count, double* recv /* world x count */);
/*      The two exchanges of the path with the payload staying in HBM until after the collective:
 *      dsmgp_fit_exchange: per-leaf (log-marginal, info) of the last dsmgp_fit, straight from the device results, padded to
 *        `count` leaves per rank (count >= this rank's leaf count; a rank without leaves passes its context with no leaf
 *        table and contributes zeros): out[(r * count + l) * 2 + {0, 1}] = mll / info of rank r's leaf l.
 *      dsmgp_aggregate_exchange: after dsmgp_aggregate_partial on every rank, all-gathers the W x n_t partial sums and
 *        adds them in rank order on the device (the same bits on every rank); dsmgp_aggregate_finish(ctx, NULL, ...)
 *        then finishes from the total (a second exchange of the same partial sums returns DSMGP_E_STATE: they already hold
 *        the total).  A rank without leaves calls dsmgp_aggregate_exchange_empty(ctx, W, n_t) instead
 *        (it contributes zeros and receives the total in `total_out`, W x n_t doubles, may be NULL). */
int dsmgp_fit_exchange(dsmgp_ctx* ctx, int64_t count, double* out /* world x count x 2 */);
int dsmgp_aggregate_exchange(dsmgp_ctx* ctx, double* total_out /* W x n_t, may be NULL */);
int dsmgp_aggregate_exchange_empty(dsmgp_ctx* ctx, int32_t W, int64_t n_t, double* total_out /* may be NULL */);
int dsmgp_comm_destroy(dsmgp_ctx* ctx);

/* Host-only (no device): the random partition tree of buildTree (src/treeStructure.jl:4-307: getSplits, _buildSplit,
 * _buildSum and the regions _buildGP turns into leaves) as one native recursion, drawing from the portable counter stream
 * `seed` (SplitMix64 in counter mode, deepstructuredmixtures_amd/datagen.py) in the order of the interpreted builder
 * (tree.py), with which it agrees bit for bit.  n_splits = config.K (cuts per split node follow the depth^2 rule of
 * :33,69,83), n_sum_children = config.V, depth = config.depth, bnoise = the eps of :49-54, n_kernels > 0: every region is
 * a sum over n_kernels GPs and n_kernels uniforms are drawn for its Dirichlet(1) weights (:258-261).
 * Result: nodes in creation (pre-)order: kind 0 region / 1 split / 2 sum, parent, split dimension, bounds lb/ub (D per
 * node), split thresholds (CSR, last = upper bound), observation lists of the regions (CSR, ascending row indices),
 * and the Dirichlet uniforms in region order. */
typedef struct dsmgp_tree dsmgp_tree;
int dsmgp_tree_build(const double* X /* N x D */, int64_t N, int32_t D, int32_t min_data, int32_t n_splits,
                     int32_t n_sum_children, int32_t depth, double bnoise, int32_t sum_root, int32_t n_kernels, uint64_t seed,
                     dsmgp_tree** out);
int dsmgp_tree_sizes(const dsmgp_tree* t, int64_t* n_nodes, int64_t* n_thr, int64_t* n_obs, int64_t* n_dir);
int dsmgp_tree_export(const dsmgp_tree* t, int32_t* kind, int32_t* parent, int32_t* split_dim, double* lb, double* ub,
                      int64_t* thr_ptr, double* thr, int64_t* obs_ptr, int64_t* obs, double* dir_u);
/* Mean of y over the observation list of every region, in region (creation) order: the ConstMean of a leaf built
 * without a mean function (src/treeStructure.jl:253).  Summed as NumPy sums a contiguous vector (pairwise), so the
 * value equals mean(y[obs]) of the interpreted builder bit for bit.  mean_out: one double per region (kind 0 node). */
int dsmgp_tree_means(const dsmgp_tree* t, const double* y, int64_t N, double* mean_out);
int dsmgp_tree_free(dsmgp_tree* t);

#ifdef __cplusplus
}
#endif
#endif
