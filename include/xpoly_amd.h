/* xpoly_amd -- MI355X (gfx950) simplex / row-elimination kernels behind xpoly's
 * SIX<Mat,T>, MIP<Mat,T> and Lineq interfaces.  C ABI, no C++ or torch types.
 *
 * The reference (stevenknown/xpoly) has no FFI: its boundary is the C++ template
 * contract of SIX<Mat,T> (src/com/lpsol.h:204-338) over Matrix<T>'s public
 * row-major buffer (src/com/matt.h:152-156).  Each entry point below names the
 * reference member it stands in for; INTEGRATION.md shows the adapter a
 * maintainer would add on the xpoly side.
 *
 * Layouts (identical to the reference's in-memory layout):
 *   f64   : double[rows*cols], row-major                  (FloatMat, xmat.h:140)
 *   rat32 : struct {int32 num; int32 den;}[rows*cols]      (RMat, xmat.h:42; rational.h:66-67)
 *   every matrix of one problem has `cols` columns; the last one is the constant
 *   column (rhs_idx = cols-1, lpsol.h:1527-1552); `vc` is (cols-1) x cols with -1
 *   on the diagonal for x_i >= 0 and an all-zero column for a free variable
 *   (lpsol.h:1322); `eq`/`leq` may have 0 rows (pass NULL).
 *
 * Return values: the reference's own status integers (lpsol.h:198-202,
 * :2082-2085) or a negative XPG_ERR_* code.  No exceptions cross this boundary.
 * All buffers are caller-owned; the library never frees caller memory.
 * Functions with a _dev suffix take DEVICE pointers; the others take HOST
 * pointers and stage through HBM themselves.
 *
 * Threading: a handle (xpg_ctx, and every xpg_lp made from it) is used by ONE host
 * thread at a time -- it owns one HIP stream, grow-only staging areas and a small
 * cache of device blocks (xpg_trim returns them), none of which is locked.  Different
 * handles, on the same device or on different ones, may be used from different
 * threads concurrently (the _multi and _ragged entry points do exactly that inside
 * the library).  The reference itself is single-threaded with per-instance state
 * (lpsol.h:205-209).
 */
#ifndef XPOLY_AMD_H
#define XPOLY_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* SIX status codes -- src/com/lpsol.h:198-202 */
#define XPG_SIX_SUCC                  0
#define XPG_SIX_UNBOUND               1
#define XPG_SIX_NO_PRI_FEASIBLE_SOL   2
#define XPG_SIX_OPTIMAL_IS_INFEASIBLE 3
#define XPG_SIX_TIME_OUT              4
/* MIP status codes -- src/com/lpsol.h:2082-2085 */
#define XPG_IP_SUCC                    0
#define XPG_IP_UNBOUND                 1
#define XPG_IP_NO_PRI_FEASIBLE_SOL     2
#define XPG_IP_NO_BETTER_THAN_BEST_SOL 3
/* library errors (never overlap 0..4) */
#define XPG_ERR_HIP          (-1)  /* a HIP runtime call failed; see xpg_last_error */
#define XPG_ERR_ALLOC        (-2)
#define XPG_ERR_SHAPE        (-3)  /* malformed sizes (reference: ASSERT only, lpsol.h:1517-1558) */
#define XPG_ERR_UNSUPPORTED  (-4)
#define XPG_ERR_NO_DEVICE    (-5)
#define XPG_ERR_REF_UNDEFINED (-7) /* the reference's behaviour is undefined on this input */
#define XPG_ERR_CHAIN_STUCK  (-8)  /* a launch whose workgroups wait for each other stopped making progress (a preempted
                                      or hung queue): the persistent chain launch of the blocked fp64 loop AFTER its roll
                                      call, the fused Rational loop's pick -> staging hand-over (also: a pivot nobody
                                      staged), or a time-sliced batch launch whose queue did not move for 20 s.  A
                                      device LP must be rebuilt (xpg_lp_begin / _two_stage); a batch call returns it as
                                      the CALL's result and none of its outputs is valid (the _dev forms, which only
                                      enqueue, leave it as the status of every LP the launch did not finish) */

typedef struct xpg_ctx xpg_ctx;   /* one device + one HIP stream + scratch; re-entrant per handle */
typedef struct xpg_lp  xpg_lp;    /* one device-resident slack-form LP (tableau, objective, basis) */

typedef struct { int32_t num, den; } xpg_rat32;   /* src/com/rational.h:66-67 */

/* ---- context ---------------------------------------------------------------- */
int         xpg_device_count(void);
int         xpg_create(xpg_ctx ** out, int device);
void        xpg_destroy(xpg_ctx * ctx);
const char *xpg_last_error(const xpg_ctx * ctx);
const char *xpg_version(void);
void *      xpg_stream(const xpg_ctx * ctx);            /* the hipStream_t all work is queued on */
int         xpg_sync(xpg_ctx * ctx);
/* device buffers for hosts without their own allocator (benchmarks, C callers) */
int         xpg_malloc(xpg_ctx * ctx, void ** dptr, size_t bytes);
int         xpg_free(xpg_ctx * ctx, void * dptr);
int         xpg_upload(xpg_ctx * ctx, void * dst_dev, const void * src_host, size_t bytes);
int         xpg_download(xpg_ctx * ctx, void * dst_host, const void * src_dev, size_t bytes);

/* ---- in-library timing of the HBM-bound sweep (K1's update kernel) -------------------
 * Between begin and end every `stride`-th launch of the sweep on this context is
 * bracketed by a pair of HIP events recorded on the context's stream (at most `cap`
 * launches are sampled; an event pair costs ~6 us of stream time, hence the stride).
 * end synchronises the stream and returns the number of sampled launches and the
 * sum of their durations in milliseconds. */
int         xpg_profile_begin(xpg_ctx * ctx, int cap, int stride);
int         xpg_profile_end(xpg_ctx * ctx, int * launches, double * total_ms);

/* ---- K1: one pivot -- SIX::pivot arithmetic, src/com/lpsol.h:1471-1501 ------------
 * tab is m x W with leading dimension ld (elements); obj has W entries.  Row `row`
 * is scaled by 1/tab[row][col], column `col` is eliminated from every other row and
 * the scaled row is folded into obj.  Asynchronous on the context's stream. */
int xpg_pivot_f64_dev(xpg_ctx * ctx, double * tab_dev, int m, int W, int ld,
                      double * obj_dev, int rhs_idx, int row, int col);
int xpg_pivot_rat32_dev(xpg_ctx * ctx, xpg_rat32 * tab_dev, int m, int W, int ld,
                        xpg_rat32 * obj_dev, int rhs_idx, int row, int col);
int xpg_pivot_f64(xpg_ctx * ctx, double * tab, int m, int W, double * obj,
                  int rhs_idx, int row, int col);
int xpg_pivot_rat32(xpg_ctx * ctx, xpg_rat32 * tab, int m, int W, xpg_rat32 * obj,
                    int rhs_idx, int row, int col);

/* ---- device-resident LP: SIX::TwoStageMethod, src/com/lpsol.h:1907-1930 ------------
 * `leq` is m x cols (A | b), x >= 0 for every variable, `tgtf` has cols entries.
 * vc_diag/vc_rhs hold vc(i,i) and vc(i,rhs) (the only cells SIX::is_feasible
 * reads, lpsol.h:798-802); NULL means -1 / 0.  kind: 0 = f64, 1 = rat32.
 * src_on_device: 0 leq / tgtf are host arrays, 1 both are device pointers, 2 leq is a device
 * pointer and tgtf a host array (what SIX::minm's device-built dual hands over). */
int  xpg_lp_create(xpg_ctx * ctx, int kind, const void * leq, int m, int cols,
                   const void * tgtf, const void * vc_diag, const void * vc_rhs,
                   int src_on_device, xpg_lp ** out);
void xpg_lp_destroy(xpg_lp * lp);
/* stage1 + solveSlackForm with SIX::set_param(.., max_iter) (lpsol.h:380-385). */
int  xpg_lp_two_stage(xpg_lp * lp, unsigned max_iter);
/* Only SIX::stage1's slack construction (lpsol.h:1820-1841); then xpg_lp_iterate
 * runs at most `pivots` more iterations of solveSlackForm's loop (lpsol.h:1039-1188)
 * without a host round trip per pivot.  Returns -1000 while still running. */
int  xpg_lp_begin(xpg_lp * lp);
int  xpg_lp_iterate(xpg_lp * lp, unsigned pivots);
#define XPG_RUNNING (-1000)
/* Pivots the handle has made over its LIFETIME (every solve on it, phase 1's included): difference two reads for one solve. */
int  xpg_lp_pivots_done(xpg_lp * lp, unsigned * out);
/* Blocked loop bookkeeping since xpg_lp_begin / xpg_lp_two_stage: sweeps that applied a full batch of
 * staged pivots (32 by default, XPG_BLOCK = 1 .. 32: the batch's stages, the first included, are chosen and
 * staged by one persistent chain launch; lp_chain.hip.h), and sweeps that applied fewer (the tail of an iterate budget, or a batch closed
 * early by a rare branch of SIX::solveSlackForm, src/com/lpsol.h:1138-1151).  Either may be NULL. */
int  xpg_lp_counters(xpg_lp * lp, unsigned * sweeps_full, unsigned * sweeps_partial);
/* Blocked fp64 loop, diagnostics: persistent chain launches of the current solve that were given up at their roll call
 * because not every worker got a compute unit in time (the device is shared with other work), and whether the handle
 * has switched this solve to launch-per-stage kernels because of it; runs (may be NULL) = the launches that passed.
 * Results are the same either way. */
int  xpg_lp_chain_aborts(xpg_lp * lp, unsigned * aborts, int * chain_off, unsigned * runs);
/* ... and how many of the launches that passed did their batch's first stage themselves (no pick / prep launches for it). */
int  xpg_lp_chain_folds(xpg_lp * lp, unsigned * folds);
/* Which loop and which kernel instances the handle runs the LP in its current shape with (evidence for bench.py's `shapes`
 * leg; no reference counterpart).  out[0..n-1], n <= 11: loop (0 pipelined, 3 blocked), pivots per blocked pass,
 * chain form (0 launch-per-stage kernels, 1 one persistent launch on one XCD, 2 the same spread over the chip), columns of
 * the entering column's line kept in LDS (0 / 8 / 16), rows per workgroup of the pass (16 / 32), leading dimension, chain
 * workers, pick workers, prep workers, LDS bytes per chain worker, and for a Rational handle the loop its last iterations
 * ran on (0 none yet, 1 one launch per pivot, 2 two launches per pivot: what xpg_test_r32_loop_plan names for its shape). */
int  xpg_lp_loop_info(xpg_lp * lp, int32_t * out, int n);
/* Test view: SIX::normalize (src/com/lpsol.h:1290-1394, convertEq2Ineq :1197-1278) made both ways for one input -- the cells
 * the HBM route makes on the device (out_dev_cells) and the cells the LDS route makes on the host (out_host_cells), each
 * [rows][n + 1] (kind 0: double, 1: xpg_rat32; cap_cells = room of each buffer in cells).  out_info[0..6] = rows, n,
 * substitutions made, equalities kept as pairs, free variables, the device form's return code, the host form's
 * (XPG_ERR_REF_UNDEFINED where the reference reads past an equality's row, lpsol.h:1232). */
int  xpg_test_normalize(xpg_ctx * ctx, int kind, const void * tgtf, const void * vc, int vc_rows, const void * eq, int eq_rows,
                        const void * leq, int leq_rows, int cols, void * out_dev_cells, void * out_host_cells, long long cap_cells,
                        int32_t * out_info);
/* Launch geometry, host-side views for tests (no device needed).  xpg_test_sweep_tile: the blocked sweep's workgroup ->
 * tile map for a tableau of `strips` 512-column strips and `rowblocks` row blocks: lid < 0 returns the grid size, else
 * 1 / 0 = workgroup lid has / has no tile, written to (*bx, *by).  xpg_test_pick_ld: the leading dimension a device
 * tableau of W live columns gets. */
int  xpg_test_sweep_tile(int strips, int rowblocks, int rev, int lid, int * bx, int * by);
int  xpg_test_pick_ld(int W);
/* The launch rules of the two HBM-resident Rational loops for a tableau of m rows and W columns, host-side view for tests (no
 * device needed): forced = 0 (XPG_R32_LOOP unset), 1 (=fused), 2 (=pipe).  out[0..n-1], n <= 11: loop taken (1 the
 * one-launch-per-pivot loop, 0 the two-launch loop); of the fused launch: pick workgroups N, stager workgroups NP, grid x,
 * grid y, rows per pick lane ceil(m / (64 N)); of the two-launch loop's sweep launch: pick workgroups N, column blocks (the
 * staging launch's grid), grid x, grid y, rows per pick lane ceil(m / (256 N)).  XPG_ERR_SHAPE for m or W <= 0 or another
 * forced. */
int  xpg_test_r32_loop_plan(int m, int W, int forced, int32_t * out, int n);
/* The device's canonical rational forms on n host triples (tests: the sweep's fused a + k * e and the ratio test's
 * b / a must equal the reference's two operations, src/com/rational.cpp:273-397, for canonical operands -- lowest
 * terms, den > 0, below the appro threshold; anything else in the inputs returns XPG_ERR_SHAPE):
 * out_fma[i] = a[i] + k[i] * e[i], out_div[i] = a[i] / k[i] (k[i] = 0: 0/1). Either output may be NULL. */
int  xpg_test_canon_ops_rat32(xpg_ctx * ctx, int n, const xpg_rat32 * a, const xpg_rat32 * k, const xpg_rat32 * e,
                              xpg_rat32 * out_fma, xpg_rat32 * out_div);
/* The device's GENERIC rational forms (any numerators, any denominators above INT32_MIN, zero and negative ones
 * included -- what a problem whose cells are not canonical runs on): out_mul[i] = a[i] * b[i], out_add[i] = a[i] + b[i],
 * out_div[i] = a[i] / b[i] as src/com/rational.cpp:273-397 computes them. Outputs may be NULL. */
int  xpg_test_any_ops_rat32(xpg_ctx * ctx, int n, const xpg_rat32 * a, const xpg_rat32 * b,
                            xpg_rat32 * out_mul, xpg_rat32 * out_add, xpg_rat32 * out_div);
/* OPT-IN, NON-PARITY (results are no longer the reference's bit for bit, and
 * nothing else in this header changes behaviour): before xpg_lp_begin / xpg_lp_two_stage,
 *   pricing = 1        Dantzig's rule -- the largest reduced cost enters -- instead of the reference's
 *                      first positive one (src/com/lpsol.h:1054-1069); the ratio test and the
 *                      anti-cycling pair table stay as they are;
 *   feas_rel_tol > 0   SIX::is_feasible (src/com/lpsol.h:784-822) with this relative tolerance
 *                      instead of Float's 1e-17 '==' (src/com/flty.cpp:41-58), which reports most
 *                      fp64 optima as SIX_OPTIMAL_IS_INFEASIBLE.
 * (0, 0.0) restores the reference's behaviour.  fp64 handles only (XPG_ERR_UNSUPPORTED otherwise). */
int  xpg_lp_set_options(xpg_lp * lp, int pricing, double feas_rel_tol);
/* shape of the live tableau: rows, columns W (= rhs_idx + 1), rhs_idx */
int  xpg_lp_shape(xpg_lp * lp, int * rows, int * W, int * rhs_idx);
/* download the live state; any pointer may be NULL.  tab: rows*W, obj: W,
 * nvset/bvset: rhs_idx bytes, bv2eq: rhs_idx, eq2bv: rows, maxv: 1, sol: W. */
int  xpg_lp_read(xpg_lp * lp, void * tab, void * obj, uint8_t * nvset, uint8_t * bvset,
                 int32_t * bv2eq, int32_t * eq2bv, void * maxv, void * sol);
/* the (entering, leaving) pairs pivoted so far, for parity tests */
int  xpg_lp_trace(xpg_lp * lp, int32_t * pairs, int cap_pairs, int * n_pairs);

/* ---- SIX::maxm / SIX::minm, src/com/lpsol.h:1993-2033 / :1662-1732 -------------------
 * Same argument meaning as the reference: out_v receives the optimum (0 on
 * non-success, lpsol.h:2024), out_sol the cols entries of `res` with a trailing
 * 1 in the constant slot (lpsol.h:1880-1887); out_sol is written only on success. */
int xpg_six_maxm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows,
                     const double * eq, int eq_rows, const double * leq, int leq_rows,
                     int cols, unsigned max_iter, double * out_v, double * out_sol);
int xpg_six_minm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows,
                     const double * eq, int eq_rows, const double * leq, int leq_rows,
                     int cols, unsigned max_iter, double * out_v, double * out_sol);
int xpg_six_maxm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                       int vc_rows, const xpg_rat32 * eq, int eq_rows,
                       const xpg_rat32 * leq, int leq_rows, int cols, unsigned max_iter,
                       xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_six_minm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                       int vc_rows, const xpg_rat32 * eq, int eq_rows,
                       const xpg_rat32 * leq, int leq_rows, int cols, unsigned max_iter,
                       xpg_rat32 * out_v, xpg_rat32 * out_sol);

/* Where the calling thread's last xpg_six_{maxm,minm}_* call spent its time, host clock, milliseconds:
 * out_ms[0..7] = total, host reshaping (SIX::normalize, lpsol.h:1290-1394: nothing but the vc diagonal when there are
 * no equalities and no free variables), handle creation incl. the upload of the system, the dual built on the device
 * (minm: upload + transpose; lpsol.h:1602-1629), stage 1 + pivot loop on the device, read-back, release, and the route
 * taken (1 = the LDS-resident batch kernel, 2 = the HBM-resident loop); out_ms[8] = the pivots the HBM-resident route's last
 * pivot loop made (SIX::solveSlackForm's cnt, lpsol.h:1187).  Evidence for bench.py and the tests; no reference counterpart. */
int xpg_six_last_profile(double * out_ms, int n);

/* ---- batches of independent small LPs (the dependence-test workload) ------------------
 * nb problems of identical shape: leq[nb][m][cols], tgtf[nb][cols], x >= 0, no
 * equalities -- what Lineq::has_solution hands to SIX (src/com/linsys.cpp:852-904).
 * Each LP is solved LDS-resident by one workgroup.  is_max selects maxm / minm.
 * out_status[nb], out_v[nb], out_sol[nb][cols] (rows of failed LPs untouched).
 * The _dev variants take device pointers for every array and are asynchronous. */
int xpg_six_batch_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf,
                      const double * leq, int m, int cols, unsigned max_iter,
                      int32_t * out_status, double * out_v, double * out_sol);
int xpg_six_batch_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf,
                        const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                        int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_six_batch_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf,
                          const double * leq, int m, int cols, unsigned max_iter,
                          int32_t * out_status, double * out_v, double * out_sol,
                          uint32_t * out_pivots);
int xpg_six_batch_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf,
                            const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                            int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol,
                            uint32_t * out_pivots);

/* The same batches for LPs of ANY size the device can hold, not only those whose slack form fits one CU's LDS (the first
 * fp64 shape xpg_six_batch_* refuses is about 100 inequalities x 100 variables).  Arguments, statuses and output rules are
 * those of xpg_six_batch_*: leq[nb][m][cols], tgtf[nb][cols], x >= 0, no equalities; out_status[nb], out_v[nb] (0 unless
 * the status is 0), out_sol[nb][cols] (rows of LPs whose status is not 0 untouched); nb == 0 returns 0.
 * The route is decided by the shape alone, for the whole batch:
 *   - the LP fits LDS (the rule of xpg_six_batch_*): the launch xpg_six_batch_* makes, unchanged;
 *   - otherwise one workgroup per LP with the tableau [R][ld] in a scratch slot in device memory that belongs to the
 *     workgroup (ld = V + R + 2 rounded up to an even number of cells; slots on 256-byte lines; grid x slot <= 256 MB, the
 *     grid is cut to stay under it; the handle keeps the area, xpg_trim returns it) and everything else -- objective row,
 *     basis maps, pair counters, the pivot-pair table -- in LDS;
 *   - XPG_ERR_UNSUPPORTED before any launch, outputs untouched, when those side arrays do not fit 160 KB of LDS (about
 *     R + V > 960) or one slot exceeds the 256 MB.
 * Status, optimum and solution are bit for bit those of xpg_six_batch_* where that accepts the shape and of
 * xpg_six_{maxm,minm}_* with vc = -I everywhere.  The _dev forms take device pointers for every array, only enqueue
 * (results after xpg_sync; a scratch area that has to grow waits for the stream first) and fill out_pivots[nb] (may be
 * NULL) with each LP's pivot count. */
int xpg_six_batch_hbm_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf,
                          const double * leq, int m, int cols, unsigned max_iter,
                          int32_t * out_status, double * out_v, double * out_sol);
int xpg_six_batch_hbm_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf,
                            const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                            int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_six_batch_hbm_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf,
                              const double * leq, int m, int cols, unsigned max_iter,
                              int32_t * out_status, double * out_v, double * out_sol,
                              uint32_t * out_pivots);
int xpg_six_batch_hbm_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf,
                                const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                                int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol,
                                uint32_t * out_pivots);
/* Evidence, no reference counterpart: the route of the calling thread's last xpg_six_batch_hbm_* call.  out[0] LPs solved
 * LDS-resident, out[1] LPs solved on tableaux in device memory, out[2] the grid of the launch (all 0 after a refused or
 * empty call).  Fills min(n, 3) entries. */
int xpg_six_batch_hbm_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): what xpg_six_batch_hbm_* does with nb LPs of kind (0 fp64, 1 rational)
 * solved as R rows x V variables on a device of num_cus compute units -- the function the launch itself asks.  Fills
 * min(n, 7) entries: out[0] route (0 LDS-resident, 1 tableau in device memory, 2 refused); [1] LDS bytes per workgroup
 * (route 0: the whole LP; else the side arrays); [2] bytes of one slot (0 on route 0); [3] ld; [4] threads per
 * workgroup; [5] grid (0 when refused); [6] scratch bytes of the launch, grid x slot. */
int xpg_test_batch_hbm_geometry(int kind, int R, int V, int nb, int num_cus, long long * out, int n);

/* The same batches for problems WITH equalities and free variables -- what SIX::maxm / minm is called with elsewhere
 * (Lineq::has_solution with is_int_sol = false, src/com/linsys.cpp:852-904, under the vc Lineq::initVarConstraint builds,
 * :803-819): nb problems of one shape, tgtf[nb][cols], eq[nb][eq_rows][cols], leq[nb][leq_rows][cols] (either may be NULL
 * with 0 rows, not both), vc[cols-1][cols] SHARED by the batch.  With a vc that is a sign pattern (see xpg_mip_*) and the
 * largest normal form of the shape -- leq_rows + 2 eq_rows inequalities, one more variable per free one -- within 64 KB
 * of LDS in the direction asked, SIX::normalize (src/com/lpsol.h:1290-1394, convertEq2Ineq :1197-1278), the solve and
 * calcFinalSolution (:1851-1899) run on the device for the whole batch, one workgroup per LP in one launch; the call
 * synchronises once.  Any other vc, or a larger shape: xpg_six_{maxm,minm}_* per problem, so the call is defined wherever
 * SIX::maxm / minm is.  Same results on both routes, bit for bit those of the single-problem entry points.
 * out_status[b] = SIX_* status, or XPG_ERR_REF_UNDEFINED for that problem alone (the reference reads past an equality's
 * row, lpsol.h:1232; stage 1's undefined case); out_v[b] = 0 unless the status is 0; out_sol[b][cols] (trailing 1) is
 * written on status 0 only.  Shape errors as the single-problem entry points (XPG_ERR_SHAPE); nb == 0 returns 0.
 * The _dev forms take device pointers for EVERY array, vc included, and only enqueue (results after xpg_sync; a scratch
 * area that has to grow waits for the stream first).  The host never sees vc there, so nothing falls back: the kernel
 * derives the free variables itself, and out_status[b] = XPG_ERR_UNSUPPORTED for every b when vc is no sign pattern or
 * the shape needs more than 64 KB (the call returns XPG_ERR_UNSUPPORTED when no vc could make the shape fit). */
int xpg_six_batch_vc_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc,
                         const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                         unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol);
int xpg_six_batch_vc_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                           const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols,
                           unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_six_batch_vc_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc,
                             const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                             unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol);
int xpg_six_batch_vc_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                               const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols,
                               unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol);
/* Evidence, no reference counterpart: which route the LPs of the calling thread's last xpg_six_batch_vc_* call took
 * (answers are identical on both).  out[0] LPs reshaped and solved on the device, out[1] LPs that took the per-problem
 * fallback, out[2] free variables split per LP on the device route (-1 after a _dev call: only the device has read vc).
 * Fills min(n, 3) entries. */
int xpg_six_batch_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the route rule of xpg_six_batch_vc_* for a vc [vc_rows][cols] of kind
 * (0 fp64, 1 rational) and a shape.  Fills min(n, 5) entries: out[0] 1 for the device route, 0 for the fallback; [1] free
 * variables (columns of vc without a nonzero); [2] rows of the largest normal form, leq_rows + 2 eq_rows; [3] its
 * variables, cols - 1 + out[1]; [4] LDS bytes of that shape in the direction asked.  XPG_ERR_SHAPE unless
 * vc_rows == cols - 1. */
int xpg_test_six_batch_vc_plan(int kind, const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int is_max,
                               long long * out, int n);

/* xpg_six_batch_vc_* for shapes of ANY size: where the largest normal form is past 64 KB of LDS the batch is still one launch.
 * Arguments, statuses and output rules are those of xpg_six_batch_vc_*.  The route is decided for the whole batch:
 *   - vc is a sign pattern and the shape fits 64 KB: the launch xpg_six_batch_vc_* makes, unchanged;
 *   - vc is a sign pattern and the shape is past 64 KB: one workgroup per LP stages eq / leq in a slot in device memory that
 *     belongs to the workgroup, runs SIX::normalize there, solves on a tableau [R][ld] in the same slot (as
 *     xpg_six_batch_hbm_* does: ld = the widest width V + R + 2 rounded up to an even number of cells, everything else of
 *     the solver in LDS) and finishes calcFinalSolution.  Slots start on 256-byte lines; grid x slot <= 256 MB, the grid is
 *     cut to stay under it; the handle keeps the area, xpg_trim returns it.  Taken when eq_rows <= 4096, the solver's side
 *     arrays for the largest normal form fit 160 KB of LDS beside the kernel's own (about R + V <= 960) and one slot fits
 *     the 256 MB;
 *   - anything else (a general vc, a shape beyond those limits): xpg_six_{maxm,minm}_* per problem, as xpg_six_batch_vc_*.
 * Same results on every route, bit for bit those of the single-problem entry points.
 * The _dev forms take device pointers for EVERY array, vc included, and only enqueue (results after xpg_sync; a scratch
 * area that has to grow waits for the stream first).  The host never sees vc there, so everything is sized for every
 * variable being free: a shape that then fits 64 KB takes xpg_six_batch_vc_*_dev's launch untouched, any other takes the
 * device-memory kernel for every LP (same bits at any size); where that kernel's limits are exceeded the call returns
 * XPG_ERR_UNSUPPORTED before any launch and writes nothing.  A vc that turns out to be no sign pattern ends every LP
 * XPG_ERR_UNSUPPORTED.  out_pivots[nb] (may be NULL): each LP's pivot count on the device-memory route; the LDS-resident
 * kernel does not count, so on that route every entry is set to 0xFFFFFFFF, "not counted". */
int xpg_six_batch_vc_hbm_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc,
                             const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                             unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol);
int xpg_six_batch_vc_hbm_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                               const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols,
                               unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_six_batch_vc_hbm_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc,
                                 const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                                 unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol,
                                 uint32_t * out_pivots);
int xpg_six_batch_vc_hbm_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                                   const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols,
                                   unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol,
                                   uint32_t * out_pivots);
/* Evidence, no reference counterpart: the route of the calling thread's last xpg_six_batch_vc_hbm_* call.  out[0] LPs on
 * the LDS-resident kernel, out[1] LPs on tableaux in device memory, out[2] LPs on the per-problem fallback, out[3] free
 * variables split per LP (-1 after a _dev call: only the device has read vc), out[4] the grid of the launch (0 without
 * one).  Fills min(n, 5) entries. */
int xpg_six_batch_vc_hbm_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the route rule of xpg_six_batch_vc_hbm_* for nb problems under a vc
 * [vc_rows][cols] of kind (0 fp64, 1 rational) on a device of num_cus compute units -- the function the launch itself
 * asks.  vc == NULL: the _dev forms' view (every variable taken as free).  Fills min(n, 10) entries: out[0] route (0
 * LDS-resident kernel, 1 device-memory kernel, 2 neither: per-problem fallback / XPG_ERR_UNSUPPORTED from a _dev form);
 * [1] free variables (-1 for vc == NULL, 0 for a general vc); [2], [3] rows and variables the largest normal form is
 * solved with (Rmax, Vmax: under minm the dual's); [4] LDS bytes per workgroup (route 0: the whole LP, else the solver's
 * side arrays); [5] bytes of one slot; [6] ld; [7] threads per workgroup; [8] grid (0 on route 2); [9] scratch bytes of
 * the launch, grid x slot.  XPG_ERR_SHAPE unless vc_rows == cols - 1 (where vc is given), nb > 0, num_cus > 0. */
int xpg_test_six_batch_vc_hbm_plan(int kind, const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int is_max,
                                   int nb, int num_cus, long long * out, int n);

/* The same batches spread over the GPUs of one node from ONE caller thread -- what a C++ xpoly
 * caller of Lineq::has_solution (src/com/linsys.cpp:860-904) gets when it hands a SCoP's worth of
 * problems over at once.  devices[ndev] lists the HIP devices (NULL: 0 .. ndev-1; a device may be
 * listed twice).  Shard g is the contiguous range [g*nb/ndev + min(g, nb%ndev), ...) (sizes differ by
 * at most one, as xpoly_amd/shard.py); each shard runs on a context and host thread of its own and
 * writes straight into the caller's HOST arrays -- there is no collective and no second copy.
 * Returns 0, or the first shard's XPG_ERR_* (XPG_ERR_NO_DEVICE when a listed device is absent). */
int xpg_six_batch_f64_multi(int ndev, const int * devices, int is_max, int nb, const double * tgtf,
                            const double * leq, int m, int cols, unsigned max_iter,
                            int32_t * out_status, double * out_v, double * out_sol);
int xpg_six_batch_rat32_multi(int ndev, const int * devices, int is_max, int nb, const xpg_rat32 * tgtf,
                              const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                              int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol);

/* ---- MIP<Mat,T>::maxm / minm, src/com/lpsol.h:2636-2657 / :2681-2702 ---------------------
 * Depth-first branch and bound exactly as MIP::RecusivePart (lpsol.h:2427-2612): every
 * node is a from-scratch SIX solve (max_iter 10000, lpsol.h:2441) on the GPU; is_bin
 * selects 0-1 programming; rational_indicator (cols bytes, may be NULL) marks entries
 * allowed to stay fractional (lpsol.h:2369-2393).  Returns XPG_IP_* or XPG_ERR_*.
 * With a vc that is a SIGN PATTERN -- zero everywhere but a diagonal of -1 (x_j >= 0) and 0 (x_j free): -I is what the
 * reference's caller PolyTran::FeaSchedule passes (src/eng/poly.cpp:5118-5130), the mixed form is what
 * Lineq::initVarConstraint builds (src/com/linsys.cpp:803-819) --, with or without equalities, and node LPs (one more
 * variable per free one: SIX::normalize's v = v' - v'') within 64 KB of LDS the whole tree walk runs on the device in one
 * launch; any other vc is walked by the host controller (node LPs on the device, lock-step rounds): same results.
 * (The reference cannot instantiate MIP<FloatMat,Float>, lpsol.h:2242-2254; the f64
 * flavour follows the same template text.) */
int xpg_mip_maxm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc, int vc_rows,
                       const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows,
                       int cols, int is_bin, const uint8_t * rational_indicator,
                       xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_mip_minm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc, int vc_rows,
                       const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows,
                       int cols, int is_bin, const uint8_t * rational_indicator,
                       xpg_rat32 * out_v, xpg_rat32 * out_sol);
int xpg_mip_maxm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows,
                     const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                     int is_bin, const uint8_t * rational_indicator, double * out_v, double * out_sol);
int xpg_mip_minm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows,
                     const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                     int is_bin, const uint8_t * rational_indicator, double * out_v, double * out_sol);
/* OPT-IN, NON-PARITY: branch and bound that re-optimises every node from its parent's final
 * tableau with the dual simplex instead of the fresh SIX per node of src/com/lpsol.h:2440-2448.  fp64; maximise (or
 * minimise) tgtf . x subject to leq (A | b), x >= 0 and integral (0/1 bounds are rows of leq, as for the parity MIP).
 * The tableau stays in HBM for the whole tree; a child is its parent's solved state plus one bound row.  Best
 * incumbent, bounding by the relaxation, floor child first -- a different (sane) walk from the reference's, so its
 * answers are checked against the optimum itself (tests/test_gpu_warm_mip.py: scipy / HiGHS;
 * tests/test_gpu_warm_mip_exact.py: exact references, every end state), not against MIP::RecusivePart.  Returns XPG_IP_SUCC,
 * XPG_IP_UNBOUND (the relaxation is unbounded), XPG_IP_NO_PRI_FEASIBLE_SOL, or XPG_ERR_UNSUPPORTED where a path needs more
 * than 2 (cols - 1) + 8 bound rows.  *out_v is the optimum on XPG_IP_SUCC and 0 otherwise; out_sol (may be NULL) is written
 * on XPG_IP_SUCC only.  out_stats (may be NULL): nodes, dual pivots over all nodes, primal pivots of the root, depth. */
int xpg_mip_warm_f64(xpg_ctx * ctx, int is_max, const double * tgtf, const double * leq, int leq_rows,
                     int cols, int is_bin, double * out_v, double * out_sol, long long * out_stats);
/* The same method for a BATCH: nb programs of one shape (tgtf [nb][cols], leq [nb][leq_rows][cols]), each tree walked by ONE
 * WORKGROUP inside one launch with its current tableau in LDS (warm_mip_batch.hip.h) -- the root's two-phase solve, the
 * depth-first stack, snapshots in HBM, bounding -- as the parity walk does it for MIP::RecusivePart (xpg_mip_batch_*).
 * is_bin: the program is 0-1 (its x_j <= 1 rows are rows of leq): a path then appends at most one bound row per variable,
 * which sizes the LDS block; 0: what 64 KB allow (a tree that needs more ends XPG_ERR_UNSUPPORTED in out_status).
 * out_status[b] = XPG_IP_* (or XPG_ERR_UNSUPPORTED), out_v[b], out_sol[b][cols]: a tree that does not end XPG_IP_SUCC has
 * out_v[b] = 0 and its out_sol row is left as the caller passed it in.  A tree whose relaxation is infeasible or unbounded
 * counts no node.  The call itself returns XPG_ERR_UNSUPPORTED, and writes nothing, where the LDS block of a tree exceeds
 * 64 KB even with 4 bound rows; nb = 0 returns 0 and touches nothing.  out_stats (may be NULL): nodes, dual pivots and root
 * pivots summed over the batch, the deepest path.  Tests: tests/test_gpu_warm_mip.py (HiGHS),
 * tests/test_gpu_warm_mip_exact.py (exact references, every launch geometry). */
int xpg_mip_warm_batch_f64(xpg_ctx * ctx, int nb, int is_max, const double * tgtf, const double * leq, int leq_rows, int cols,
                           int is_bin, int32_t * out_status, double * out_v, double * out_sol, long long * out_stats);
/* Host-only view for tests (no device needed): what xpg_mip_warm_batch_f64 launches nb trees of leq_rows x cols with, from
 * the function the launch itself calls.  Fills min(n, 9) entries: out[0] LDS bytes of a workgroup, [1] 1 when the call is
 * refused (XPG_ERR_UNSUPPORTED: more than 64 KB even with 4 bound rows), [2] depth_cap (bound rows a path may append),
 * [3] mcap (row capacity), [4] wcap (row stride), [5] doubles per snapshot, [6] doubles of workspace per tree, [7] trees per
 * launch, [8] launches. */
int xpg_test_warm_batch_geometry(int leq_rows, int cols, int is_bin, int nb, long long * out, int n);
/* Lineq::has_solution(leq, eq, vc, rhs_idx, is_int_sol, is_unique_sol),
 * src/com/linsys.cpp:830-906.  Returns 1 / 0, or XPG_ERR_*. */
int xpg_has_solution_rat32(xpg_ctx * ctx, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq,
                           int eq_rows, const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx,
                           int is_int_sol, int is_unique_sol);
/* Lineq::has_solution for nb systems of one shape in one call: leq [nb][leq_rows][cols], eq [nb][eq_rows][cols], vc
 * [cols-1][cols] shared by the batch.  XPG_ERR_SHAPE as xpg_has_solution_rat32 (rhs_idx == cols - 1, vc_rows == rhs_idx);
 * nb = 0 returns 0; without any row every verdict is 0, without an inequality XPG_ERR_REF_UNDEFINED (the reference sizes its
 * objective from leq).  out_has[b]: 1 / 0, or the negative status a solve of system b returned (-7 where lpsol.h:1232 reads
 * past an equality's row); such a status ends that system at once.  out_status [nb][2] (may be NULL): the XPG_SIX_* /
 * XPG_IP_* status of the maxm solve and of the minm solve, [1] = XPG_HS_NOT_RUN where maxm decided (and both on the
 * per-system route, which reports verdicts only).  The rule is the reference's: status 0 -> 1, status 1 without
 * is_unique_sol -> 1, else minm under the same rule, else 0.
 * is_int_sol = 0: max_iter bounds each SIX solve (0xFFFFFFFF: the reference's default, what the single call uses).
 *   - vc a sign pattern and the largest normal form within 64 KB of LDS in BOTH directions: one launch, a workgroup per
 *     system -- the objective (SIX::reviseTargetFunc on all ones) from the cells as given, SIX::normalize ONCE, maxm, then
 *     minm on the same normal form where maxm left the question open;
 *   - a sign pattern past that with both directions within the limits of xpg_six_batch_vc_hbm_*: the same on a slot in
 *     device memory (one launch, sized for the larger direction);
 *   - anything else: xpg_has_solution_rat32 per system (max_iter is not used there).
 *   The statuses are bit for bit those of xpg_six_maxm_rat32 / xpg_six_minm_rat32 on the objective has_solution builds.
 * is_int_sol = 1 (host arrays only; max_iter ignored, MIP fixes 10000 per node): xpg_mip_batch_vc_hbm_rat32 with
 *   is_max = 1 on all systems, then with is_max = 0 on the open ones; the answers of xpg_has_solution_rat32(..., 1, u).
 * The _dev form: every pointer a device pointer, is_int_sol must be 0, enqueue only -- results after xpg_sync.  The host
 * never sees vc: sized for every variable free; a vc that is no sign pattern ends every system XPG_ERR_UNSUPPORTED, a shape
 * beyond both kernels returns XPG_ERR_UNSUPPORTED before any launch.  Slots live in the areas the handle keeps for
 * xpg_six_batch_vc_* / xpg_six_batch_vc_hbm_*; xpg_trim returns them.
 * Tests: tests/test_has_solution_batch_host.py, tests/test_gpu_has_solution_batch.py. */
enum { XPG_HS_NOT_RUN = 0x7FFFFFFF };
int xpg_has_solution_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                                 const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_int_sol, int is_unique_sol,
                                 unsigned max_iter, int32_t * out_has, int32_t * out_status);
int xpg_has_solution_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                                     const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_int_sol, int is_unique_sol,
                                     unsigned max_iter, int32_t * out_has, int32_t * out_status);
/* Evidence, no reference counterpart: what the calling thread's last xpg_has_solution_batch_* call did.  out[0] systems on
 * the LDS-resident kernel, [1] on the device-memory kernel, [2] solved per system, [3] systems whose second solve ran (-1
 * after a _dev call: only the device knows), [4] the grid of the launch (0 without one).  Fills min(n, 5) entries. */
int xpg_has_solution_batch_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the route rule of xpg_has_solution_batch_* (is_int_sol = 0) for nb rational
 * systems of a shape under vc [vc_rows][cols] on a device of num_cus compute units -- the function the launch itself asks;
 * vc = NULL: the _dev form's view.  Fills min(n, 9) entries: out[0] route (0 LDS-resident kernel, 1 device-memory kernel,
 * 2 neither); [1] free variables (-1: the _dev view); [2] rows of the largest tableau of either direction; [3] LDS bytes
 * per workgroup (route 0: the larger direction's whole LP, else the larger side arrays); [4] bytes of one slot; [5] ld;
 * [6] threads; [7] grid (0 on route 2); [8] scratch bytes of the launch. */
int xpg_test_has_solution_batch_plan(const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int nb, int num_cus,
                                     long long * out, int n);
/* Lineq::has_solution for nb systems of MIXED shapes under one vc in one call -- what a SCoP hands over: DepPolyMgr::build
 * emits systems whose row counts follow the statements' depths.  System b has leq_rows[b] x cols inequalities at CELL offset
 * leq_offsets[b] of leq and eq_rows[b] x cols equalities at eq_offsets[b] of eq (the offset convention of the other ragged
 * entry points; arrays of nb entries); cols, rhs_idx and vc -- the sign pattern of the variables -- are the call's.  eq /
 * eq_offsets may be NULL when every eq_rows[b] is 0.  XPG_ERR_SHAPE, before anything touches a device: the rule of
 * xpg_has_solution_batch_rat32, a NULL shape or offset array, a negative entry.  nb = 0 returns 0.
 * Per system the verdict and the out_status pair are bit for bit those of xpg_has_solution_batch_rat32 called with that
 * system alone (XPG_HS_NOT_RUN, -7, the rule for a system without inequalities).
 * is_int_sol = 0: a system takes, inside this call, the route a uniform call of its shape takes --
 *   - the systems whose own shape the LDS-resident kernel takes: ONE launch of its form over an index list;
 *   - the systems whose own shape the device-memory kernel takes: ONE launch of that kernel's form;
 *   - a general vc, a shape past both kernels: xpg_has_solution_rat32 per system; without inequalities: no solve at all.
 *   A launch is sized by the largest of what the route rule gives its systems, size by size (LDS bytes, threads, slot, tableau
 *   rows, ld), never by the envelope shape (largest leq_rows, largest eq_rows), which can lie past a route all its systems are
 *   on.  The concatenated arrays go up as they lie, one copy each; both launches are enqueued before the call's single
 *   synchronisation.  Slots live in the areas of xpg_six_batch_vc_* / xpg_six_batch_vc_hbm_*; xpg_trim returns them.
 * is_int_sol = 1: the shape classes on the host, each as xpg_has_solution_batch_rat32 with is_int_sol = 1 answers it.
 * There is no _dev form: the route rule needs the shapes on the host.
 * Tests: tests/test_has_solution_ragged_host.py, tests/test_gpu_has_solution_ragged.py. */
int xpg_has_solution_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets,
                                        const xpg_rat32 * eq, const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc,
                                        int vc_rows, int cols, int rhs_idx, int is_int_sol, int is_unique_sol, unsigned max_iter,
                                        int32_t * out_has, int32_t * out_status /* [nb][2], may be NULL */);
/* Evidence, no reference counterpart: what the calling thread's last xpg_has_solution_batch_ragged_rat32 call did.  out[0]
 * systems on the LDS-resident kernel, [1] on the device-memory kernel, [2] answered per system, [3] systems whose second
 * solve ran, [4] the grid of the LDS launch, [5] of the device-memory launch (0 without one), [6] systems answered without a
 * solve.  Fills min(n, 7) entries. */
int xpg_has_solution_batch_ragged_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the plan of a ragged call (is_int_sol = 0) under vc [vc_rows][cols] on a
 * device of num_cus compute units -- the function the launches themselves ask.  out_route[b] (may be NULL): 0 LDS-resident
 * kernel, 1 device-memory kernel, 2 per system, 3 without inequalities.  Fills min(n, 12) entries: the LDS launch -- out[0]
 * systems, [1] LDS bytes, [2] threads, [3] slot bytes, [4] grid; the device-memory launch -- [5] systems, [6] LDS bytes,
 * [7] slot bytes, [8] Rmax, [9] ld, [10] threads, [11] grid.  Each size is the largest of what
 * xpg_test_has_solution_batch_plan reports for a system of that launch; a launch without systems reports zeros. */
int xpg_test_has_solution_batch_ragged_plan(const void * vc, int vc_rows, int cols, int nb, const int32_t * leq_rows, const int32_t * eq_rows,
                                            int num_cus, int32_t * out_route /* [nb] */, long long * out, int n);
/* Lineq::has_solution(..., is_int_sol = true, is_unique_sol) -- the form DepPoly::is_empty asks (src/eng/poly.cpp:571) -- for nb
 * systems of one shape in one call that synchronises ONCE: leq [nb][leq_rows][cols], eq [nb][eq_rows][cols] and the free
 * variables of vc [cols-1][cols] go up once, the feasibility objective is built on the device, both MIP walks and the verdict
 * run there, and only the verdicts and the status pairs come down.  Host arrays, Rational only (the reference's has_solution
 * is).  The shape rules are xpg_has_solution_batch_rat32's (XPG_ERR_SHAPE before anything touches a device; nb = 0 returns 0;
 * without any row every verdict is 0, without an inequality XPG_ERR_REF_UNDEFINED).  out_has[b]: 1 / 0, or the negative status
 * a walk of system b returned; out_status [nb][2] (may be NULL): the XPG_IP_* status of the maxm walk and of the minm walk,
 * [1] = XPG_HS_NOT_RUN where maxm decided.  The caller's arrays are written at the very end only.
 * Per system out_has and the out_status pair are bit for bit what xpg_has_solution_batch_rat32(..., is_int_sol = 1,
 * is_unique_sol, ...) returns on the same arrays.  The route is the shape's alone (XPG_MIP_DEVICE is not read):
 *   - vc a sign pattern and the node LPs of the deepest path within 64 KB of LDS in both directions: the tree-walk kernel of
 *     xpg_mip_batch_vc_* twice -- maxm on all systems, minm under the marks a small kernel sets from maxm's verdicts --
 *     with no host step between the passes;
 *   - a sign pattern past that with both directions within the limits of xpg_mip_batch_vc_hbm_*: ONE launch, a workgroup per
 *     system from the objective to the verdict, node tableaux in device memory, everything sized for the larger direction;
 *   - anything else (a general vc, a shape past either direction's limits): xpg_has_solution_batch_rat32 with is_int_sol = 1.
 * There is no _dev form: the walk sizes its workspace by the number of free variables, which a host that never sees vc cannot
 * know.  Tableau slots live in the area of xpg_six_batch_hbm_* / xpg_mip_batch_vc_hbm_*; xpg_trim returns them.
 * Tests: tests/test_has_solution_int_host.py, tests/test_gpu_has_solution_int.py. */
int xpg_has_solution_int_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                                     const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_unique_sol, int32_t * out_has,
                                     int32_t * out_status /* [nb][2], may be NULL */);
/* The same for systems of MIXED shapes under one vc: the arguments of xpg_has_solution_batch_ragged_rat32 without is_int_sol
 * and max_iter.  The shape classes are formed on the host, in order of first sight, and each is answered by
 * xpg_has_solution_int_batch_rat32; the answers come back in the order given.  Fusing the walks of different shapes into one
 * launch stays open. */
int xpg_has_solution_int_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets,
                                            const xpg_rat32 * eq, const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc,
                                            int vc_rows, int cols, int rhs_idx, int is_unique_sol, int32_t * out_has,
                                            int32_t * out_status /* [nb][2], may be NULL */);
/* Evidence, no reference counterpart: what the calling thread's last xpg_has_solution_int_batch_* call did.  out[0] systems
 * on the LDS-resident walk, [1] on the device-memory kernel, [2] answered by xpg_has_solution_batch_rat32, [3] systems whose
 * second walk ran, [4] the grid of the maxm pass (of the one launch on the device-memory route; 0 without a launch), [5] the
 * grid of the minm pass of the LDS-resident walk (else 0).  After the ragged call: the counts summed over its classes, the
 * largest grids.  Fills min(n, 6) entries. */
int xpg_has_solution_int_batch_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the route rule of xpg_has_solution_int_batch_* for nb systems of a shape under
 * vc [vc_rows][cols] on a device of num_cus compute units -- the function the launches themselves ask.  Fills min(n, 17)
 * entries; where there are two, maxm's then minm's: out[0] route (0 LDS-resident walk, 1 device-memory kernel, 2 neither);
 * [1] free variables; [2] rows of the largest node LP; [3] [4] LDS bytes per workgroup (route 1: the larger side arrays,
 * twice); [5] [6] threads; [7] [8] grid (route 1: the one launch's, twice; route 2: 0); [9] [10] helper workgroups behind the
 * walkers (route 0); [11] bytes of one tableau slot (route 1: the larger direction's); [12] [13] ld; [14] workspace words of
 * a workgroup (route 1: the objective included); [15] the word the objective starts at (route 1); [16] scratch bytes (route
 * 0: the workspaces of the larger grid, helpers included; route 1: grid x (slot + workspace)). */
int xpg_test_has_solution_int_plan(const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int nb, int num_cus,
                                   long long * out, int n);

/* Batches: nb independent problems of one shape, x >= 0, inequalities only
 * (tgtf[nb][cols], leq[nb][leq_rows][cols]).  Every tree is walked on the device by one
 * workgroup (node rebuild, normalisation, LDS solve, the recursion of lpsol.h:2427-2612 as a
 * stack machine); problems whose node LPs do not fit 64 KB of LDS advance in lock step from the
 * host instead, the node LPs of a round sharing one launch.
 * out_nodes (may be NULL) receives the total number of node LPs solved. */
int xpg_mip_batch_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf,
                        const xpg_rat32 * leq, int leq_rows, int cols, int32_t * out_status,
                        xpg_rat32 * out_v, xpg_rat32 * out_sol, long long * out_nodes);
int xpg_mip_batch_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf,
                      const double * leq, int leq_rows, int cols, int32_t * out_status,
                      double * out_v, double * out_sol, long long * out_nodes);
/* The same for nb MIPs with eq_rows EQUALITIES each at the root, eq[nb][eq_rows][cols] (x >= 0; the shape
 * PolyTran::FeaSchedule hands to MIP::maxm / minm, src/eng/poly.cpp:5118-5130); leq may be NULL with
 * leq_rows = 0.  Every node runs SIX::convertEq2Ineq (src/com/lpsol.h:1197-1278) over the root's and the
 * branches' equalities, as the reference's recursion does. */
int xpg_mip_batch_eq_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf,
                           const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows, int cols,
                           int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol, long long * out_nodes);
int xpg_mip_batch_eq_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf,
                         const double * leq, int leq_rows, const double * eq, int eq_rows, int cols,
                         int32_t * out_status, double * out_v, double * out_sol, long long * out_nodes);
/* The same under the caller's variable constraints vc [cols-1][cols], shared by the batch -- the vc the single-problem
 * entry points take: eq [nb][eq_rows][cols] and leq [nb][leq_rows][cols], either of which may be NULL / 0 (not both);
 * rational_indicator (cols bytes, may be NULL) as for MIP::maxm.  A vc that is a sign pattern (see above) and node LPs
 * within 64 KB of LDS: one launch of the device tree walk, free variables split in front of every node LP.  Any other
 * vc, or larger node LPs: the host controller, so the call is defined wherever MIP::maxm / minm is.  Same results. */
int xpg_mip_batch_vc_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf,
                           const xpg_rat32 * vc, const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows,
                           int cols, const uint8_t * rational_indicator, int32_t * out_status, xpg_rat32 * out_v,
                           xpg_rat32 * out_sol, long long * out_nodes);
int xpg_mip_batch_vc_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf,
                         const double * vc, const double * eq, int eq_rows, const double * leq, int leq_rows,
                         int cols, const uint8_t * rational_indicator, int32_t * out_status, double * out_v,
                         double * out_sol, long long * out_nodes);
/* Evidence, no reference counterpart: which route the trees of the calling thread's last MIP, has_solution or
 * dep_is_empty call took (single-context entry points; answers are identical on both routes).  Reset when such a call
 * starts and summed over its walks: out[0] trees walked on the device, out[1] trees walked by the host controller,
 * out[2] free variables split per tree on the device route (0 on the host route).  Fills min(n, 3) entries. */
int xpg_mip_last_route(long long * out, int n);
/* xpg_mip_batch_vc_* for node LPs of ANY size: the same arguments, the same results (status, optimum, solution and node
 * count bit for bit), one more route.
 *   - a sign-pattern vc and node LPs within 64 KB of LDS: the launch xpg_mip_batch_vc_* makes;
 *   - a sign-pattern vc past that: still one launch and no host controller -- a workgroup of 256 threads walks one tree
 *     after the other as above, the tableau [R][ld] of every node LP in a slot in device memory that belongs to the
 *     workgroup (as xpg_six_batch_hbm_*: ld = the widest width V + R + 2 rounded up to an even number of cells, everything
 *     else of the solver in LDS; slots start on 256-byte lines).  Taken when eq_rows + cols + 1 <= 256, the solver's side
 *     arrays for the largest node LP fit 160 KB of LDS beside the kernel's own (about R + V <= 960) and one slot fits
 *     256 MB; grid x (slot + workspace) <= 256 MB, the grid is cut to stay under it; the handle keeps the slots, xpg_trim
 *     returns them;
 *   - anything else (a general vc, a shape beyond those limits): the host controller, as xpg_mip_batch_vc_*.
 * xpg_mip_last_route counts the trees of the first two routes as walked on the device. */
int xpg_mip_batch_vc_hbm_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf,
                               const xpg_rat32 * vc, const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows,
                               int cols, const uint8_t * rational_indicator, int32_t * out_status, xpg_rat32 * out_v,
                               xpg_rat32 * out_sol, long long * out_nodes);
int xpg_mip_batch_vc_hbm_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf,
                             const double * vc, const double * eq, int eq_rows, const double * leq, int leq_rows,
                             int cols, const uint8_t * rational_indicator, int32_t * out_status, double * out_v,
                             double * out_sol, long long * out_nodes);
/* Evidence, no reference counterpart: the route of the calling thread's last xpg_mip_batch_vc_hbm_* call.  out[0] trees
 * on the LDS-resident walk, out[1] trees on the device-memory walk, out[2] trees on the host controller, out[3] free
 * variables split per tree on the device, out[4] the grid of the launch (0 without one).  Fills min(n, 5) entries. */
int xpg_mip_hbm_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the route rule of xpg_mip_batch_vc_hbm_* for nb trees of a shape of kind
 * (0 fp64, 1 rational) on a device of num_cus compute units -- the function the launch itself asks.  pattern: whether vc
 * is a sign pattern, extra: its free variables (ignored without a pattern).  Fills min(n, 11) entries: out[0] route (0
 * LDS-resident walk, 1 device-memory walk, 2 host controller); [1] free variables; [2], [3] rows and variables the
 * largest node LP is solved with (R, V: under minm the dual's); [4] LDS bytes per workgroup (route 0: the whole node LP,
 * else the solver's side arrays); [5] bytes of one tableau slot (0 on route 0); [6] ld; [7] 8-byte words of one
 * workgroup's workspace; [8] threads per workgroup; [9] grid (0 on route 2); [10] scratch bytes of the launch, grid x
 * (slot + workspace).  XPG_ERR_SHAPE unless 0 <= extra <= cols - 1, nb > 0, num_cus > 0. */
int xpg_test_mip_hbm_plan(int kind, int pattern, int leq_rows, int eq_rows, int cols, int is_bin, int is_max, int extra,
                          int nb, int num_cus, long long * out, int n);
/* Host-only views for tests (no device needed).  vc_pattern: 1 when vc [vc_rows][cols] of kind (0 fp64, 1 rational) is a
 * sign pattern, with out_free[j] = 1 for every free variable j < cols - 1; 0 when it is general; XPG_ERR_SHAPE unless
 * vc_rows == cols - 1.  mip_fits: 1 / 0, whether the device tree walk takes a problem of that shape with `extra` free
 * variables (the LDS budget of its largest node LP, maximising and minimising).  mip_front_route: 1 / 0, whether the one
 * route rule of xpg_mip_maxm / minm_*, xpg_mip_batch_*, xpg_mip_batch_eq_* and xpg_mip_batch_vc_* sends a call of that
 * shape to the device tree walk or to the host controller -- fit: the fit test the entry point asks with (1: mip_fits, all
 * of them but xpg_mip_batch_*; 0: the LDS of the direction is_max alone, xpg_mip_batch_*), pattern / extra: vc_pattern's
 * verdict and free variables (1 / 0 for x >= 0), allowed: 0 stands for XPG_MIP_DEVICE=0; XPG_ERR_SHAPE for a fit or kind
 * that is neither 0 nor 1, cols < 2, a negative count or no row at all. */
int xpg_test_vc_pattern(int kind, const void * vc, int vc_rows, int cols, uint8_t * out_free);
int xpg_test_mip_fits(int kind, int leq_rows, int eq_rows, int cols, int is_bin, int extra);
int xpg_test_mip_front_route(int fit, int kind, int pattern, int extra, int leq_rows, int eq_rows, int cols, int is_bin,
                             int is_max, int allowed);
/* Host-only view for tests (no device needed): the launch geometry of the batched LP kernel (xpg_six_batch_*) for nb LPs
 * that are solved as R rows x V variables (maxm: R = m, V = cols - 1; minm solves the dual: the two swap) on a device of
 * num_cus compute units.  Fills min(n, 10) entries: out[0] LDS bytes of one LP, [1] 1 when the call is refused
 * (XPG_ERR_UNSUPPORTED), [2] cells, [3] threads per workgroup, [4] LPs per compute unit by LDS, [5] 1 for the five-per-CU
 * kernel instance, [6] workgroups (before continuation workgroups), [7] seats, [8] 1 when the shape can run in time
 * slices, [9] 1 when nb is large enough for them. */
int xpg_test_batch_geometry(int kind, int R, int V, int nb, int num_cus, long long * out, int n);
/* DepPoly::is_empty(keepit, vc = NULL), src/eng/poly.cpp:530-573, for nb dependence polyhedra
 * mats[nb][rows][cols] without constant symbols (constant in the last column):
 * Lineq::reduce pre-filter, then Lineq::has_solution(is_int_sol, is_unique_sol) = MIP::maxm
 * and, failing that, MIP::minm.  out_empty[b] = 1 / 0, or XPG_ERR_REF_UNDEFINED. */
int xpg_dep_is_empty_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                                 int32_t * out_empty, long long * out_nodes);

/* The same with the two arguments of the reference spelled out: the constant is column rhs_idx and the columns
 * after it are constant symbols, which Lineq::move2var (src/com/linsys.cpp:1177-1200) first turns into variables
 * (i + j <= 1 + M + N  ->  i + j - M - N <= 1, poly.cpp:536-548); vc [rhs_idx][rhs_idx + 1] are the caller's
 * variable constraints (NULL: -x_i <= 0, poly.cpp:559-567).  With symbols the reference hands has_solution a
 * matrix with several constant columns, which SIX::verify only ASSERTs (lpsol.h:1526-1552): systems that
 * Lineq::reduce does not decide then get XPG_ERR_REF_UNDEFINED in out_empty. */
int xpg_dep_is_empty_batch_ex_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                                    int rhs_idx, const xpg_rat32 * vc, int32_t * out_empty,
                                    long long * out_nodes);
/* The same with a choice of what happens to a parametrised polyhedron (rhs_idx < cols - 1) that Lineq::reduce does not decide.
 *   XPG_DEP_PARITY           what the reference does: undefined (XPG_ERR_REF_UNDEFINED in out_empty).  Built with
 *                            -fsanitize=address the reference heap-overflows there: MIP::verify -> Matrix::is_colequ, from
 *                            src/com/linsys.cpp:864 -- vc is sized for rhs_idx variables, the system has rhs_idx + symbols.
 *   XPG_DEP_SYMBOLS_AS_VARS  OPT-IN, NOT PARITY: the evident intent of src/eng/poly.cpp:530-573 -- after move2var the symbols
 *                            are variables of unknown sign, so has_solution(int, unique) is asked about the widened system:
 *                            rhs_idx = cols - 1, vc widened by all-zero (= free) rows and columns for the symbols.  Checked
 *                            against the CPU restatement's move2var + reduce + has_solution on that widened system.
 * (The one other answer of this library that is not the reference's: a list of polyhedra one of whose members fails calcBound
 * -- xpg_lineq_hull_batch_ragged_rat32's out_member, below: the group has no rows, where the reference's release build goes on
 * with stale bounds.  That, too, answers a violated precondition, not a result.) */
enum { XPG_DEP_PARITY = 0, XPG_DEP_SYMBOLS_AS_VARS = 1 };
int xpg_dep_is_empty_batch_mode_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                      const xpg_rat32 * vc, int mode, int32_t * out_empty, long long * out_nodes);
/* Multi-device forms of the two batches above (sharding and devices[] as xpg_six_batch_*_multi;
 * out_nodes receives the sum over the shards). */
int xpg_mip_batch_rat32_multi(int ndev, const int * devices, int nb, int is_max, int is_bin,
                              const xpg_rat32 * tgtf, const xpg_rat32 * leq, int leq_rows, int cols,
                              int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol,
                              long long * out_nodes);
int xpg_dep_is_empty_batch_rat32_multi(int ndev, const int * devices, int nb, const xpg_rat32 * mats,
                                       int rows, int cols, int32_t * out_empty, long long * out_nodes);

/* ---- ragged batches: problems of different shapes in one call -------------------------------------------------
 * What one SCoP hands the dependence analysis: DepPolyMgr::build emits polyhedra whose shape follows the
 * statements' depths and the parameter count (src/eng/poly.cpp:1120-1224, :1009-1053) and DepGraph::rebuild tests
 * each (poly.cpp:268-314, :530-573).  Padding to one shape is not parity-neutral, so shapes are per problem:
 * rows[b], cols[b], and the CELL offset of problem b in the concatenated array (offsets[b]; tgtf / sol / v arrays of
 * the LP form have their own offsets, cols[b] cells each).  The library sorts the problems into shape classes and
 * runs the classes concurrently, each on its own stream of the handle's device; results come back in problem order.
 * Semantics per problem are those of the uniform entry points above. */
int xpg_six_batch_f64_ragged(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * leq,
                             const int32_t * rows, const int32_t * cols, const long long * leq_offsets,
                             const long long * tgtf_offsets, unsigned max_iter, int32_t * out_status,
                             double * out_v, double * out_sol);
int xpg_six_batch_rat32_ragged(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * leq,
                               const int32_t * rows, const int32_t * cols, const long long * leq_offsets,
                               const long long * tgtf_offsets, unsigned max_iter, int32_t * out_status,
                               xpg_rat32 * out_v, xpg_rat32 * out_sol);
/* DepPoly::is_empty (poly.cpp:530-573) on nb polyhedra of mixed shapes, constant in the last column of each. */
int xpg_dep_is_empty_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows,
                                        const int32_t * cols, const long long * offsets, int32_t * out_empty,
                                        long long * out_nodes);
/* Lineq::reduce in place (system b keeps its rows[b] x cols[b] cells at offsets[b], the survivors packed at their
 * front); rhs_idx[b] is its constant column (NULL: the last column of each). */
int xpg_lineq_reduce_batch_ragged_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, const int32_t * rows,
                                        const int32_t * cols, const long long * offsets, const int32_t * rhs_idx,
                                        int is_intersect, int32_t * out_rows, int32_t * out_ok);
/* Lineq::fme eliminating variable u[b] of system b.  Packed result: out_rows[b] rows of cols[b] cells starting at
 * cell out_cell_offsets[b] of outs (out_cell_offsets[nb] = all cells).  outs NULL: a sizing call (returns 0);
 * outs_cap_cells too small: XPG_ERR_SHAPE with out_rows / out_cell_offsets filled. */
int xpg_lineq_fme_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows,
                                     const int32_t * cols, const long long * offsets, const int32_t * rhs_idx,
                                     const int32_t * u, int darkshadow, xpg_rat32 * outs, long long outs_cap_cells,
                                     long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok);

/* ---- rational row elimination, batches of small systems (one wavefront each) -------------
 * mats is [nb][rows][cols] of xpg_rat32 on the host; rhs_idx is the constant column,
 * columns after it are constant symbols (src/com/linsys.h:64-70).
 *   reduce      : Lineq::reduce(m, rhs_idx, is_intersect), src/com/linsys.cpp:359-626, in
 *                 place; out_rows[b] = surviving rows (packed at the front of system b),
 *                 out_ok[b] = its bool (consistent).
 *   remove_iden : Lineq::removeIdenRow, src/com/linsys.cpp:1209-1268, in place.
 *   fme         : Lineq::fme(u, res, darkshadow), src/com/linsys.cpp:656-774; outs is
 *                 [nb][cap_rows][cols]; out_rows[b] < 0 means the result needs -out_rows[b]
 *                 rows (> cap_rows) and was not written.
 *   rank/det/inv: Matrix<Rational>::rank / det / inv, src/com/matt.h:2614-2726, :1621-1736,
 *                 :1743-1845 (Gauss-Jordan with the reference's pivot preference). */
int xpg_lineq_reduce_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols,
                                 int rhs_idx, int is_intersect, int32_t * out_rows, int32_t * out_ok);
int xpg_lineq_remove_iden_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols,
                                      int32_t * out_rows);
/* Lineq::move2var, src/com/linsys.cpp:1177-1200, in place on every system: columns first_sym..last_sym (constant
 * symbols, behind the constant column rhs_idx) are multiplied by -1 and moved in front of column rhs_idx.  A
 * reshaping of the host arrays (no kernel); the multiplication is the reference's Rational '*'. */
int xpg_lineq_move2var_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                   int first_sym, int last_sym);
int xpg_lineq_fme_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                              int rhs_idx, int u, int darkshadow, xpg_rat32 * outs, int cap_rows,
                              int32_t * out_rows, int32_t * out_ok);
/* Lineq::fme (src/com/linsys.cpp:656-774) with a PACKED result -- the form a host-resident caller wants: the
 * worst case of a result is rows^2/4 + rows rows, the typical one a third of it, and the slots of the entry point
 * above come back whole.  Here row_offsets[nb + 1] (in rows) and only the live rows of every system, back to back
 * ([row_offsets[nb]][cols]), travel; both directions go through pinned memory of the handle.
 *   outs      (may be NULL) receives the rows; outs_cap_rows is its capacity in rows.  Too small: XPG_ERR_SHAPE with
 *             row_offsets filled, so the caller can size the buffer and call again.
 *   out_view  (may be NULL) receives a pointer to the same rows in the handle's pinned buffer, valid until the next
 *             packed call on this handle (or xpg_destroy): the zero-copy form the C++ adapter uses.
 *   cap_rows  rows of the device slot per system; <= 0: the worst case.  A result that needs more: XPG_ERR_UNSUPPORTED.
 * out_ok[b] as above.  One handle is used by one host thread at a time. */
int xpg_lineq_fme_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                                     int rhs_idx, int u, int darkshadow, int cap_rows, xpg_rat32 * outs,
                                     long long outs_cap_rows, const xpg_rat32 ** out_view, long long * row_offsets,
                                     int32_t * out_ok);
/* Lineq::reduce (src/com/linsys.cpp:359-626) with a PACKED result, the form a host-resident caller of many systems wants
 * (round 6): mats is read only; row_offsets[nb + 1] (in rows) and the surviving rows of every system, back to back, come
 * back -- the device writes them straight into pinned memory of the handle, so the call synchronises once.  outs /
 * outs_cap_rows / out_view as for the packed fme above; out_rows (may be NULL) receives the per-system counts
 * (= row_offsets[b + 1] - row_offsets[b]); out_ok[b] is Lineq::reduce's bool.  The in-place entry point
 * xpg_lineq_reduce_batch_rat32 is this call plus a copy of every system's survivors to the front of its slot. */
int xpg_lineq_reduce_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                        int is_intersect, xpg_rat32 * outs, long long outs_cap_rows,
                                        const xpg_rat32 ** out_view, long long * row_offsets, int32_t * out_rows,
                                        int32_t * out_ok);
/* Gives the device blocks and pinned staging a handle keeps between host-array calls back to the runtime (they are
 * kept to spare one-system callers four hipMalloc / hipFree pairs per call; at most 1 GiB / 16 blocks), and the
 * scratch slots of xpg_six_batch_vc_*, xpg_six_batch_hbm_*, xpg_six_batch_vc_hbm_* and xpg_mip_batch_vc_hbm_* (which
 * shares xpg_six_batch_hbm_*'s), of xpg_lineq_project_batch_* (xpg_lineq_levels_batch_* shares them) and of
 * xpg_lineq_bounds_batch_*. */
int xpg_trim(xpg_ctx * ctx);
/* Lineq::calcBound, src/com/linsys.cpp:1047-1078, for nb systems: for each variable j every
 * other variable is eliminated (innermost first) by chained fme launches that stay on the
 * device.  bounds is [nb][rhs_idx][cap_rows][cols], out_rows is [nb][rhs_idx];
 * out_ok[b] = 1, 0 (an elimination found the system inconsistent) or -rows_needed. */
int xpg_lineq_calc_bound_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                                     int rhs_idx, int cap_rows, xpg_rat32 * bounds, int32_t * out_rows,
                                     int32_t * out_ok);
/* The same with a PACKED result (round 5): the nb * rhs_idx bound systems back to back instead of worst-case slots --
 * row_offsets[b * rhs_idx + j] is the first row of variable j's bounds of system b, row_offsets[nb * rhs_idx] the total; the
 * slots stay in HBM and are compacted there, only live rows cross the link.  outs (may be NULL) has room for outs_cap_rows
 * rows (too small: XPG_ERR_SHAPE with row_offsets filled); out_view (may be NULL) receives a pointer into the handle's
 * pinned buffer, valid until the handle's next call; cap_rows <= 0: 4 * rows + 16.  out_ok[b] = 1, 0 (inconsistent: its
 * chains count as empty) or -rows_needed (then nothing is packed and every offset is 0: call again with that cap_rows). */
int xpg_lineq_calc_bound_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                            int cap_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                            long long * row_offsets, int32_t * out_ok);
/* The same three on DEVICE arrays (xpg_malloc / any HIP allocation of the handle's device), enqueue only: the
 * results are there after xpg_sync.  For chains of eliminations that stay in HBM, and for measuring the kernels
 * without PCIe.  d_outs is not cleared: rows of a slot past d_out_rows[b] keep what they held. */
int xpg_lineq_reduce_batch_rat32_dev(xpg_ctx * ctx, int nb, xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                     int is_intersect, int32_t * d_out_rows, int32_t * d_out_ok);
int xpg_lineq_fme_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                  int u, int darkshadow, xpg_rat32 * d_outs, int cap_rows, int32_t * d_out_rows,
                                  int32_t * d_out_ok);
/* A PROJECTION: the variables elim[0 .. n_elim) eliminated one after the other, each Lineq::fme's result the input of the
 * next (DepPoly::eliminateAuxVar, src/eng/poly.cpp:643-651; the scanning bounds, src/eng/poly.cpp:4807-4813), for nb systems of
 * one shape in ONE launch: every step of a system runs before its wavefront takes the next system, intermediates live in
 * LDS or in two device slots per resident wavefront, and only the final rows are stored per system.  The list is the
 * batch's (host memory, at most 64 entries: more is XPG_ERR_UNSUPPORTED); an index may repeat, the repeated step copies
 * as the reference's does.  darkshadow goes to every step.
 *   cap_rows      rows an intermediate or a final result may have before it is reduced; <= 0: fme's worst case for `rows`
 *   cap_out_rows  rows of a system's final slot; <= 0 (or above cap_rows): cap_rows
 *   out_ok[b]     1: out_steps[b] = n_elim and system b's rows are packed (none where an intermediate came out empty: fme
 *                 of an empty system is true and empty);  0: step out_steps[b] found the system inconsistent;  -need: step
 *                 out_steps[b] needs `need` > cap_rows rows, or (out_steps[b] == n_elim) the final result has `need` >
 *                 cap_out_rows rows.  A system with out_ok[b] <= 0 contributes no rows; the others are packed all the same.
 * outs, outs_cap_rows, out_view and row_offsets as xpg_lineq_fme_batch_packed_rat32 (neither outs nor out_view: a sizing
 * call).  XPG_ERR_SHAPE: n_elim <= 0, an index outside [0, rhs_idx), rhs_idx outside [1, cols); XPG_ERR_UNSUPPORTED: the LDS
 * layout of cap_rows exceeds 160 KB, or cap_rows > 32767. */
int xpg_lineq_project_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                         const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                         xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                         long long * row_offsets, int32_t * out_ok, int32_t * out_steps);
/* The same on DEVICE arrays, enqueue only (elim stays a host array: it travels as a kernel argument): d_outs
 * [nb][cap_out_rows][cols] receives each result's live rows and is not cleared behind them, d_out_rows / d_out_ok /
 * d_out_steps [nb].  The intermediates' slots belong to the handle (grow-only; xpg_trim returns them).  The row stride of
 * d_outs is the caller's: nothing is defaulted or clamped here -- cap_rows < rows or cap_out_rows > cap_rows is XPG_ERR_SHAPE;
 * cap_out_rows <= 0 alone stands for cap_rows (slots of cap_rows rows). */
int xpg_lineq_project_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                      const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                      xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_steps);
/* Evidence, no reference counterpart: what the calling thread's last xpg_lineq_project_batch_* call did.  out[0] launches of
 * the chain kernel (1; 0 where nothing was launched), [1] its grid, [2] systems per workgroup, [3] LDS bytes per system,
 * [4] rows of the LDS result area (a step at or under it is built in LDS), [5] bytes of intermediate slots the launch was
 * given: grid x [2] x 2 x cap_rows x cols x 8, whatever nb is.  Fills min(n, 6) entries. */
int xpg_lineq_project_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the same six figures from the shape alone -- the function the launch itself
 * asks -- then [6] the cap_rows and [7] the cap_out_rows it settles on.  Fills min(n, 8) entries; XPG_ERR_SHAPE /
 * XPG_ERR_UNSUPPORTED as the call. */
int xpg_test_lineq_project_plan(int nb, int rows, int cols, int cap_rows, int cap_out_rows, long long * out, int n);
/* Host-only view for tests: what both projection calls answer to an elimination list before they look at the handle or at
 * anything else -- 0, XPG_ERR_SHAPE (n_elim <= 0, no list, an index outside [0, rhs_idx), rhs_idx outside [1, cols)) or
 * XPG_ERR_UNSUPPORTED (more than 64 entries).  The function the calls themselves ask. */
int xpg_test_lineq_project_check(int cols, int rhs_idx, const int32_t * elim, int n_elim);
/* A projection that KEEPS EVERY LEVEL: loop-bound generation (LoopTran::transformIterSpace, src/eng/ldtran.cpp:178-196 and
 * :241-257) eliminates rhs_idx-1 .. 1 and records the system after each step, which bounds a loop of its own.  For nb systems
 * of one shape the variables elim[0 .. n_elim) are eliminated one after the other in ONE launch, as the projection does, and
 * the rows after EACH step are stored and packed: level k of system b is the system with elim[0 .. k] eliminated.  The list
 * follows the projection's rules (xpg_test_lineq_project_check); darkshadow goes to every step.
 *   cap_rows      rows an intermediate may have before it is reduced; <= 0: fme's worst case for `rows`
 *   cap_out_rows  rows of a level's slot; <= 0: min(cap_rows, 4 * rows + 16) -- the slots follow nb * n_elim, not the grid, so
 *                 the default is not the worst case; above cap_rows: cap_rows
 *   row_offsets   [nb * n_elim + 1], entry b * n_elim + k the first row of level k of system b (the layout
 *                 xpg_lineq_bounds_batch_packed_rat32 uses for [nb][rhs_idx])
 *   out_ok[b]     1: out_steps[b] = n_elim and every level is packed (after an empty intermediate every later level has 0
 *                 rows: fme of an empty system is true and empty);  0: step out_steps[b] found the system inconsistent;
 *                 -need, with out_steps[b] = k:  need > cap_rows: step k's unreduced result needs `need` rows;
 *                 cap_out_rows < need <= cap_rows: level k's reduced result has `need` rows and does not fit its slot.  The
 *                 two cannot be confused: a reduced result never has more rows than its step built, which were at most
 *                 cap_rows.  A system with out_ok[b] <= 0 contributes no rows at ANY level, those before its failing step
 *                 included; the others are packed all the same.
 * outs, outs_cap_rows and out_view as xpg_lineq_project_batch_packed_rat32 (neither outs nor out_view: a sizing call).
 * XPG_ERR_SHAPE / XPG_ERR_UNSUPPORTED as the projection; nb * n_elim above INT_MAX is XPG_ERR_UNSUPPORTED.  nb == 0: returns
 * 0, row_offsets[0] = 0. */
int xpg_lineq_levels_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                        const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                        xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                        long long * row_offsets, int32_t * out_ok, int32_t * out_steps);
/* The same on DEVICE arrays, enqueue only (elim stays a host array): d_outs [nb][n_elim][cap_out_rows][cols] receives each
 * level's live rows and is not cleared behind them, d_out_rows [nb][n_elim] their counts (all 0 for a system with d_out_ok <=
 * 0), d_out_ok / d_out_steps [nb].  The intermediates' slots are the projection's (grow-only; xpg_trim returns them).  Both
 * capacities are the caller's, nothing is defaulted or clamped: cap_rows < rows, cap_out_rows <= 0 or cap_out_rows > cap_rows
 * is XPG_ERR_SHAPE.  This differs on purpose from xpg_lineq_project_batch_rat32_dev, where cap_out_rows <= 0 stands for
 * cap_rows: here cap_out_rows is the row stride of nb x n_elim slots of d_outs, and no default of it is a safe guess. */
int xpg_lineq_levels_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                     const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                     xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_steps);
/* Evidence, no reference counterpart: what the calling thread's last xpg_lineq_levels_batch_* call did.  out[0 .. 6) as
 * xpg_lineq_project_last_route (launches, grid, systems per workgroup, LDS bytes per system, rows of the LDS result area,
 * bytes of intermediate slots: independent of nb), [6] bytes of the level slots, nb x n_elim x cap_out_rows x cols x 8.  Fills
 * min(n, 7) entries. */
int xpg_lineq_levels_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the same seven figures from the shape alone -- the function the launch itself
 * asks -- then [7] the cap_rows and [8] the cap_out_rows it settles on.  Fills min(n, 9) entries; XPG_ERR_SHAPE (n_elim <= 0
 * too) / XPG_ERR_UNSUPPORTED (n_elim > 64 too) as the call. */
int xpg_test_lineq_levels_plan(int nb, int rows, int cols, int n_elim, int cap_rows, int cap_out_rows, long long * out, int n);
/* Limits of TRANSFORMED loop nests in ONE launch: LoopTran::transformIterSpace (src/eng/ldtran.cpp:131-300) starts from a nest
 * A * i <= C and a transformation T -- det(T) and T^-1 (:148, :160), (A * T^-1 | C) (:162-175), then the fme loop rhs_idx-1 .. 1
 * whose every level is a loop bound (:178-196).  For nb transformations tmats [nb][n][n], n = rhs_idx, each against its own
 * nest nests [nb][rows][cols] or (shared_nest != 0) against ONE rows x cols nest -- the search over transformations: the nest
 * goes up once.
 *   mode 0        T is the transformation.  out_det[b] = det(T) always (Matrix<Rational>::det, src/com/matt.h:1621-1736).
 *                 det == 0: out_kind[b] = 1 (singular; the reference ASSERTs);  |det| != 1: out_kind[b] = 2 (nonsingular, not
 *                 unimodular: the reference's second branch, :203-291).  Both end the system with no rows, out_ok[b] = 1 and
 *                 out_steps[b] = 0.  Else out_kind[b] = 0 and the multiplier M = T^-1 (Matrix<Rational>::inv, matt.h:1743-1845).
 *   mode 1        T is the right multiplier M itself -- the Ui of the second branch (A * Ui, :233-235) or a T^-1 the caller
 *                 holds: no determinant, no inverse, out_det untouched (may be NULL), out_kind[b] = 0.
 *   out_mult      [nb][n][n]: M, the reference's invt / idx_map (zeros for a system of kind 1 or 2)
 *   level 0       A' = (A * M | C): operator* (matt.h:60-79: tmp = 0, tmp = tmp + a(i,k) * m(k,j), k ascending), the constant
 *                 columns copied bit for bit -- aux_limits' tail and trA.  Level k >= 1 is A' with rhs_idx-1 .. rhs_idx-k
 *                 eliminated: a system has n levels; n == 1 has level 0 only.
 *   row_offsets   [nb * n + 1], entry b * n + k the first row of level k of system b
 *   cap_rows, cap_out_rows   as xpg_lineq_levels_batch_packed_rat32; a level's slot holds the nest, so an explicit cap_out_rows
 *                 under rows is XPG_ERR_SHAPE (the default min(cap_rows, 4 * rows + 16) never is)
 *   out_ok, out_steps [nb]   the levels call's, steps counted in eliminations (1 with n - 1; 0 or -need with the step
 *                 concerned).  A system with out_ok[b] <= 0 contributes no rows at any level, level 0 included.
 * outs, outs_cap_rows, out_view and the sizing call as xpg_lineq_levels_batch_packed_rat32; one upload (two copies above 4 MB),
 * one launch.  XPG_ERR_SHAPE: rhs_idx outside [1, cols), mode outside {0, 1}, nb < 0, nests or tmats NULL with nb > 0;
 * XPG_ERR_UNSUPPORTED as the levels call, rhs_idx - 1 > 64 included.  nb == 0: returns 0, row_offsets[0] = 0. */
int xpg_lineq_transform_levels_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * nests, int shared_nest, const xpg_rat32 * tmats,
                                                  int rows, int cols, int rhs_idx, int mode, int cap_rows, int cap_out_rows,
                                                  xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                                  long long * row_offsets, int32_t * out_ok, int32_t * out_steps, int32_t * out_kind,
                                                  xpg_rat32 * out_det, xpg_rat32 * out_mult);
/* The same on DEVICE arrays, enqueue only: d_outs [nb][n][cap_out_rows][cols] receives each level's live rows and is not
 * cleared behind them, d_out_rows [nb][n] their counts, d_out_ok / d_out_steps / d_out_kind [nb], d_out_det [nb] (mode 0),
 * d_out_mult [nb][n][n] (left alone for a system of kind 1 or 2).  The intermediates' slots are the projection's.  Both
 * capacities are the caller's, as xpg_lineq_levels_batch_rat32_dev states them: cap_rows < rows, cap_out_rows > cap_rows or
 * cap_out_rows < rows is XPG_ERR_SHAPE. */
int xpg_lineq_transform_levels_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_nests, int shared_nest, const xpg_rat32 * d_tmats,
                                               int rows, int cols, int rhs_idx, int mode, int cap_rows, int cap_out_rows,
                                               xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_steps,
                                               int32_t * d_out_kind, xpg_rat32 * d_out_det, xpg_rat32 * d_out_mult);
/* Evidence, no reference counterpart: what the calling thread's last xpg_lineq_transform_levels_batch_* call did.  The seven
 * figures of xpg_lineq_levels_last_route, [6] the bytes of the level slots nb x n x cap_out_rows x cols x 8.  Fills min(n, 7). */
int xpg_lineq_transform_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the same seven figures from the shape alone -- the function the launch itself
 * asks -- then [7] cap_rows, [8] cap_out_rows and [9] where the inverse's scratch (n x 2n augmented matrix, T's copy, row
 * factors, live flags) starts in a system's LDS block: 0 where it lies in the walk's two idle areas, else the byte behind the
 * walk's scratch where it was added.  Fills min(n, 10) entries; XPG_ERR_SHAPE / XPG_ERR_UNSUPPORTED as the call. */
int xpg_test_lineq_transform_plan(int nb, int rows, int cols, int rhs_idx, int cap_rows, int cap_out_rows, long long * out, int n);
/* The projection and the levels for systems of MIXED shapes and lists in ONE launch: the statements of a SCoP sit at
 * different depths, so rows, cols, rhs_idx and the list rhs_idx-1 .. 1 differ from statement to statement.  mats holds the
 * systems, system b (rows[b] x cols[b]) at cell offsets[b]; rhs_idx[b] its constant column (NULL: the last column of each);
 * its list is elim[elim_offsets[b] .. elim_offsets[b + 1]) (elim_offsets[0] = 0), under the projection's rules.  Every step of
 * every system runs in one launch, whose LDS layout and capacities are those of the ENVELOPE -- the widest system's columns,
 * the capacities of the system with the most rows -- while each system keeps its own row stride, so its results are, bit for
 * bit, those of the uniform calls with the same capacities.
 *   cap_rows      rows an intermediate may have before it is reduced; <= 0: fme's worst case for the LARGEST rows[b]
 *   cap_out_rows  rows of an output slot; <= 0: cap_rows (projection), min(cap_rows, 4 * max rows + 16) (levels)
 *   projection    out_cell_offsets [nb + 1], out_rows [nb]: result b (out_rows[b] rows, cols[b] wide) starts at CELL
 *                 out_cell_offsets[b] (the convention of xpg_lineq_fme_batch_ragged_rat32)
 *   levels        out_cell_offsets [elim_offsets[nb] + 1], out_rows [elim_offsets[nb]]: level k of system b is entry
 *                 elim_offsets[b] + k
 *   out_ok, out_steps [nb]: as xpg_lineq_project_batch_packed_rat32 / xpg_lineq_levels_batch_packed_rat32, `need` judged
 *                 against the call's cap_rows / cap_out_rows.  A system with out_ok[b] <= 0 contributes no cells.
 * outs (may be NULL) has room for outs_cap_cells cells, out_view (may be NULL) receives a pointer into the handle's pinned
 * buffer, valid until the handle's next packed call; neither: a sizing call.  XPG_ERR_SHAPE where outs is too small (offsets,
 * counts and verdicts are filled).  Decided before anything is launched: XPG_ERR_SHAPE -- an empty list, an index outside
 * [0, rhs_idx[b]), rhs_idx[b] outside [1, cols[b]), rows[b] <= 0; XPG_ERR_UNSUPPORTED -- a list above 64 entries, the
 * envelope's LDS layout over 160 KB, cap_rows > 32767.  nb == 0: returns 0, out_cell_offsets[0] = 0.  The intermediates'
 * slots are the projection's (xpg_trim returns them). */
int xpg_lineq_project_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                         const long long * offsets, const int32_t * rhs_idx, const int32_t * elim,
                                         const int32_t * elim_offsets, int darkshadow, int cap_rows, int cap_out_rows, xpg_rat32 * outs,
                                         long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets,
                                         int32_t * out_rows, int32_t * out_ok, int32_t * out_steps);
int xpg_lineq_levels_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                        const long long * offsets, const int32_t * rhs_idx, const int32_t * elim,
                                        const int32_t * elim_offsets, int darkshadow, int cap_rows, int cap_out_rows, xpg_rat32 * outs,
                                        long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets,
                                        int32_t * out_rows, int32_t * out_ok, int32_t * out_steps);
/* Evidence, no reference counterpart: what the calling thread's last ragged projection / levels call did.  out[0] launches of
 * the chain kernel (1; 0 where nothing ran), [1] its grid, [2] systems per workgroup, [3] LDS bytes per system, [4] rows of
 * the LDS result area, [5] bytes of intermediate slots (grid x [2] x 2 x cap_rows x widest cols x 8), [6] bytes of output
 * slots (cap_out_rows x cols[b] x 8 per result).  Fills min(n, 7) entries. */
int xpg_lineq_ragged_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the same seven figures from the shapes and lists alone -- the function the
 * launch itself asks, with its error codes -- then [7] the cap_rows, [8] the cap_out_rows, [9] the columns and [10] the rows
 * of the envelope.  levels != 0: the levels call's plan.  Fills min(n, 11) entries. */
int xpg_test_lineq_ragged_plan(int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx, const int32_t * elim,
                               const int32_t * elim_offsets, int levels, int cap_rows, int cap_out_rows, long long * out, int n);
/* Lineq::calcBound, src/com/linsys.cpp:1047-1078, for nb systems of one shape in ONE launch: the bounds of every variable j
 * alone (the other rhs_idx - 1 variables eliminated, inner to outer).  The rhs_idx chains of a system share their beginnings
 * -- each starts by eliminating rhs_idx-1 .. j+1 -- so a wavefront walks those prefixes once and runs only the tail j-1 .. 0
 * per variable: (rhs_idx - 1)(rhs_idx + 2) / 2 elimination steps per system instead of rhs_idx (rhs_idx - 1), intermediates
 * in LDS or in three device slots per resident wavefront.  The results are those of the chains run one by one, bit for bit.
 *   cap_rows      rows an intermediate or a result may have before it is reduced; <= 0: 4 * rows + 16
 *   cap_out_rows  rows of a result's slot; <= 0 (or above cap_rows): cap_rows
 *   row_offsets   [nb * rhs_idx + 1], entry b * rhs_idx + j the first row of variable j's bounds of system b (the layout of
 *                 xpg_lineq_calc_bound_batch_packed_rat32)
 *   out_ok[b]     1: every chain ran, out_chain[b] = -1, out_steps[b] = 0 (a chain with an empty intermediate ends empty).
 *                 Else the verdict of the LOWEST failing chain out_chain[b] -- the one the reference, which runs variable 0
 *                 first and returns at once, meets -- at step out_steps[b] of that chain's list:  0: the step found the system
 *                 inconsistent;  -need: the step needs `need` > cap_rows rows, or (out_steps[b] == rhs_idx - 1) the chain's
 *                 result has `need` > cap_out_rows rows.  A system with out_ok[b] <= 0 contributes no rows; the others are
 *                 packed all the same (unlike xpg_lineq_calc_bound_batch_packed_rat32, which packs nothing).
 * outs, outs_cap_rows and out_view as xpg_lineq_project_batch_packed_rat32 (neither outs nor out_view: a sizing call).
 * XPG_ERR_SHAPE: rhs_idx outside [1, cols), rows <= 0, cols <= 1, a missing output; XPG_ERR_UNSUPPORTED: the LDS layout of
 * cap_rows exceeds 160 KB, or cap_rows > 32767.  nb == 0: returns 0, row_offsets[0] = 0. */
int xpg_lineq_bounds_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, int cap_rows,
                                        int cap_out_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                        long long * row_offsets, int32_t * out_ok, int32_t * out_chain, int32_t * out_steps);
/* The same on DEVICE arrays, enqueue only: d_outs [nb][rhs_idx][cap_out_rows][cols] receives each result's live rows and is not
 * cleared behind them, d_out_rows [nb][rhs_idx] their counts (all 0 for a system with d_out_ok <= 0), d_out_ok / d_out_chain
 * / d_out_steps [nb].  The intermediates' slots belong to the handle (grow-only; xpg_trim returns them).  The row stride of
 * d_outs is the caller's: cap_rows < rows or cap_out_rows > cap_rows is XPG_ERR_SHAPE; cap_out_rows <= 0 alone stands for
 * cap_rows. */
int xpg_lineq_bounds_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx, int cap_rows,
                                     int cap_out_rows, xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok,
                                     int32_t * d_out_chain, int32_t * d_out_steps);
/* Evidence, no reference counterpart: what the calling thread's last xpg_lineq_bounds_batch_* call did.  out[0] launches (1; 0
 * where nothing was launched), [1] grid, [2] systems per workgroup, [3] LDS bytes per system, [4] rows of the LDS result
 * area, [5] bytes of slots the launch was given: grid x [2] x 3 x cap_rows x cols x 8, whatever nb is, [6] elimination steps
 * per system, (rhs_idx - 1)(rhs_idx + 2) / 2.  Fills min(n, 7) entries. */
int xpg_lineq_bounds_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the same seven figures from the shape alone -- the function the launch itself
 * asks -- then [7] the cap_rows and [8] the cap_out_rows it settles on.  Fills min(n, 9) entries; XPG_ERR_SHAPE /
 * XPG_ERR_UNSUPPORTED as the call. */
int xpg_test_lineq_bounds_plan(int nb, int rows, int cols, int rhs_idx, int cap_rows, int cap_out_rows, long long * out, int n);
/* The fused calcBound for systems of MIXED shapes in ONE launch: the statements of a SCoP sit at different depths, so rows,
 * cols and rhs_idx differ from statement to statement.  mats holds the systems, system b (rows[b] x cols[b]) at cell
 * offsets[b]; rhs_idx[b] its constant column (NULL: the last column of each).  Every chain of every system runs in one launch
 * (one upload, one synchronisation), whose LDS layout and capacities are those of the ENVELOPE -- the widest system's columns,
 * the most rows -- while each system keeps its own row stride, so its results and verdicts are, bit for bit, those of
 * xpg_lineq_bounds_batch_packed_rat32 called on its shape class with the same capacities.
 *   cap_rows      rows an intermediate or a result may have before it is reduced; <= 0: 4 * LARGEST rows[b] + 16
 *   cap_out_rows  rows of a result's slot; <= 0 (or above cap_rows): cap_rows
 *   R             the sum of rhs_idx[b]; the bounds of variable j of system b are entry first[b] + j, first[b] the sum of the
 *                 rhs_idx before b
 *   out_cell_offsets [R + 1], out_rows [R]: entry r (out_rows[r] rows, its system's cols wide) starts at CELL
 *                 out_cell_offsets[r] (the convention of xpg_lineq_levels_batch_ragged_rat32)
 *   out_ok, out_chain, out_steps [nb]: as xpg_lineq_bounds_batch_packed_rat32, `need` judged against the call's cap_rows /
 *                 cap_out_rows.  A system with out_ok[b] <= 0 contributes no cells; the others are packed all the same.
 * outs (may be NULL) has room for outs_cap_cells cells, out_view (may be NULL) receives a pointer into the handle's pinned
 * buffer, valid until the handle's next packed call; neither: a sizing call.  XPG_ERR_SHAPE where outs is too small (offsets,
 * counts and verdicts are filled).  Decided before anything is launched: XPG_ERR_SHAPE -- nb < 0, rhs_idx[b] outside
 * [1, cols[b]), rows[b] <= 0, cols[b] <= 1, a missing array; XPG_ERR_UNSUPPORTED -- the envelope's LDS layout over 160 KB,
 * cap_rows > 32767.  nb == 0: returns 0, out_cell_offsets[0] = 0.  The intermediates' slots are the fused calcBound's
 * (xpg_trim returns them).  There is no _dev form, as for the ragged projection. */
int xpg_lineq_bounds_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                        const long long * offsets, const int32_t * rhs_idx, int cap_rows, int cap_out_rows,
                                        xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view,
                                        long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok, int32_t * out_chain,
                                        int32_t * out_steps);
/* Evidence, no reference counterpart: what the calling thread's last xpg_lineq_bounds_batch_ragged_rat32 call did.  out[0]
 * launches (1; 0 where nothing was launched), [1] grid, [2] systems per workgroup, [3] LDS bytes per workgroup, [4] rows of the
 * LDS result area, [5] bytes of intermediate slots (grid x 3 x cap_rows x widest cols x 8), [6] bytes of output slots
 * (rhs_idx[b] x cap_out_rows x cols[b] x 8 per system), [7] elimination steps of the batch, the sum of
 * (rhs_idx[b] - 1)(rhs_idx[b] + 2) / 2.  Fills min(n, 8) entries. */
int xpg_lineq_bounds_ragged_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the same eight figures from the shapes alone -- the function the launch itself
 * asks, with its error codes -- then [8] the cap_rows, [9] the cap_out_rows, [10] the columns and [11] the rows of the
 * envelope.  Fills min(n, 12) entries. */
int xpg_test_lineq_bounds_ragged_plan(int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx, int cap_rows,
                                      int cap_out_rows, long long * out, int n);
/* Lineq::ConvexHullUnionAndIntersect (src/com/linsys.cpp:283-336) for MANY lists of polyhedra in one call.  The members are laid
 * out exactly as xpg_lineq_bounds_batch_ragged_rat32 takes its systems; group_offsets [n_groups + 1] partitions them: group g is
 * the list of members group_offsets[g] .. group_offsets[g + 1] - 1, in list order.  Members of one group must share cols and
 * rhs_idx (the reference's "homotype" assertion); their row counts may differ, groups may differ in everything.  Per group:
 * calcBound on every member (ONE launch of the ragged calcBound kernel over all members), every variable's bounds -- members in
 * list order, inside a member the variables 0 .. rhs_idx-1, empty bounds skipped -- appended to a matrix that begins with one
 * zero row (the reference's res.reinit(1, cols)), and Lineq::reduce(res, rhs_idx, is_intersect) over the lot: a second launch on
 * the same stream, one wavefront per group, no host synchronisation between the two.  One upload, one synchronisation.
 * is_intersect == 0: the widest bounds (the union's bounding hull); else the tightest.  Result rows come in gather order.
 *   cap_rows, cap_out_rows   the members' calcBound capacities, as xpg_lineq_bounds_batch_ragged_rat32
 *   cap_hull_rows            rows a group may gather, lead row included; <= 0: the largest 1 + 2 * rhs_idx * members of any
 *                            group, at most 32767; > 32767: XPG_ERR_UNSUPPORTED (reduce indexes rows as 16-bit)
 *   out_cell_offsets [n_groups + 1], out_rows [n_groups]: group g's out_rows[g] rows, its cols wide, start at CELL
 *                            out_cell_offsets[g]
 *   out_ok, out_member, out_chain, out_steps [n_groups]:
 *     out_ok 1, out_member -1     every member's calcBound succeeded and reduce returned true: the rows are reduce's
 *     out_ok 0, out_member -1     reduce returned false.  is_intersect: 0 rows (the reference's res.clean()); else the rows as
 *                                 reduce leaves them, after removeIdenRow, uncompacted -- what xpg_lineq_reduce_batch_rat32
 *                                 returns for an inconsistent system
 *     out_member m >= 0           member m of the group (the LOWEST such) did not succeed: out_ok (0 or -need), out_chain and
 *                                 out_steps are that member's calcBound verdict, the group has 0 rows, reduce is not run.
 *                                 STATED DEVIATION, NOT PARITY: the reference's release build compiles the ASSERT on calcBound
 *                                 out and goes on with the bounds left over from the previous member.  This answers a violated
 *                                 precondition, not a result.
 *     out_ok -need, out_member -1 the group gathers need > cap_hull_rows rows: 0 rows; the other groups are answered all the same
 *     a group without members     0 rows, out_ok 1
 * outs / outs_cap_cells / out_view / a sizing call (neither) / XPG_ERR_SHAPE with offsets, counts and verdicts filled: as
 * xpg_lineq_bounds_batch_ragged_rat32.  Decided before anything is launched: XPG_ERR_SHAPE -- members of a group that differ in
 * cols or rhs_idx, group_offsets not starting at 0, not monotone or not ending at n_members, and what the ragged calcBound
 * refuses; XPG_ERR_UNSUPPORTED -- cap_hull_rows > 32767, the group kernel's LDS (32 KB of rows and the scratch of cap_hull_rows)
 * over 160 KB, and what the ragged calcBound refuses.  n_groups == 0 (and n_members == 0): 0, out_cell_offsets[0] = 0.
 * A group's matrix is gathered in LDS where its gathered capacity min(cap_hull_rows, 1 + members * rhs_idx * cap_out_rows) rows
 * of its own cols fit the LDS rows of the call, else in a device slot of its workgroup.  There is no _dev form. */
int xpg_lineq_hull_batch_ragged_rat32(xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats,
                                      const int32_t * rows, const int32_t * cols, const long long * offsets, const int32_t * rhs_idx,
                                      int is_intersect, int cap_rows, int cap_out_rows, int cap_hull_rows, xpg_rat32 * outs,
                                      long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                                      int32_t * out_ok, int32_t * out_member, int32_t * out_chain, int32_t * out_steps);
/* The projected union of PolyTran::step_4 (src/eng/poly.cpp:4802-4823) for many groups: every member is projected by its own
 * elimination list (elim / elim_offsets / darkshadow per member, as xpg_lineq_project_batch_ragged_rat32: one launch of the
 * ragged chain kernel), the results of a group's members are concatenated in list order -- no lead row -- and ONE
 * Lineq::reduce(ub, rhs_idx, is_intersect) runs per group (step_4 passes 0).  Everything else as
 * xpg_lineq_hull_batch_ragged_rat32: a member's verdict is the chain's (out_ok, out_steps; out_chain is -1), cap_hull_rows <= 0 is
 * the largest 2 * rhs_idx * members of any group, a group's gathered capacity is min(cap_hull_rows, members * cap_out_rows). */
int xpg_lineq_project_union_batch_ragged_rat32(xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats,
                                               const int32_t * rows, const int32_t * cols, const long long * offsets, const int32_t * rhs_idx,
                                               const int32_t * elim, const int32_t * elim_offsets, int darkshadow, int is_intersect,
                                               int cap_rows, int cap_out_rows, int cap_hull_rows, xpg_rat32 * outs, long long outs_cap_cells,
                                               const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok,
                                               int32_t * out_member, int32_t * out_chain, int32_t * out_steps);
/* Evidence, no reference counterpart: what the calling thread's last hull or projected-union call did (one record serves both).
 * out[0] launches of the producer (1; 0 where nothing was launched), [1] launches of the group kernel (1), [2] its grid, [3] its
 * LDS bytes per workgroup, [4] groups whose home is LDS, [5] groups whose home is a device slot (groups without members are in
 * neither), [6] bytes of the producer's intermediate slots, [7] bytes of the workgroups' device slots (0 where no group needs
 * one), [8] bytes of the output slots -- the producer's, and one more slot per group with a lead row; a group's result goes to
 * the front of its own members' slots, nothing grows with n_groups * cap_hull_rows -- [9] rows gathered over all groups (lead
 * rows included).  Fills min(n, 10) entries. */
int xpg_lineq_hull_last_route(long long * out, int n);
int xpg_lineq_project_union_last_route(long long * out, int n);
/* Host-only view for tests (no device needed): the plan of a hull call (elim_offsets NULL) or of a projected union from the
 * shapes alone -- the function the launch itself asks, with its error codes.  out[0 .. 8] as the route, then [9] cap_rows, [10]
 * cap_out_rows, [11] cap_hull_rows as settled, [12] rows of the LDS matrix area at [13] the envelope's columns.  homes [n_groups]
 * (may be NULL): 0 LDS, 1 device slot, -1 no members; gcaps [n_groups] (may be NULL): each group's gathered capacity.  Fills
 * min(n, 14) entries. */
int xpg_test_lineq_hull_plan(int n_groups, const int32_t * group_offsets, int n_members, const int32_t * rows, const int32_t * cols,
                             const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, int cap_rows, int cap_out_rows,
                             int cap_hull_rows, long long * out, int n, int32_t * homes, int32_t * gcaps);
int xpg_rat_rank_batch_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int32_t * d_out_rank);
int xpg_rat_rank_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                       int32_t * out_rank);
int xpg_rat_det_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int n, xpg_rat32 * out_det);
int xpg_rat_inv_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int n, xpg_rat32 * out_inv,
                      int32_t * out_ok);
/* Matrix<Rational>::rank(&basis, is_unitarize), src/com/matt.h:2614-2726 (caller
 * src/eng/ldtran.cpp:440-449).  basis is [nb][rows][cols]; basis_rows[b] = rows, except
 * without unitarising and rank < rows, where the reference returns the rank original rows in
 * pivot order (matt.h:2710-2719).  Rows past basis_rows[b] are zero. */
int xpg_rat_rank_basis_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                             int is_unitarize, int32_t * out_rank, xpg_rat32 * basis,
                             int32_t * basis_rows);
/* Matrix<Rational>::null, src/com/matt.h:2546-2584: ns is [nb][cols][cols], column convention. */
int xpg_rat_null_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                       xpg_rat32 * ns);
/* INTMat::hnf, src/com/xmat.cpp:912-992 (with gen_elim_mat :853-868, exgcd comf.cpp:295-321;
 * caller src/eng/ldtran.cpp:208): h = mat * u, h [nb][rows][cols] lower triangular, u
 * [nb][cols][cols] unimodular.  INT arithmetic is two's-complement 32 bit.  status[b] = 0, or
 * XPG_ERR_REF_UNDEFINED where the reference divides by zero (zero diagonal below row 0) or
 * multiplies by its rows x cols identity read out of bounds (cols > rows, negative diagonal);
 * h and u of such a matrix are left zero. */
int xpg_int_hnf_batch(xpg_ctx * ctx, int nb, const int32_t * mats, int rows, int cols, int32_t * h,
                      int32_t * u, int32_t * status);
/* INTMat::gcd, src/com/xmat.cpp:996-1030: every row divided by the gcd of its nonzero
 * magnitudes, in place. */
int xpg_int_gcd_batch(xpg_ctx * ctx, int nb, int32_t * mats, int rows, int cols);

#ifdef __cplusplus
}
#endif
#endif /* XPOLY_AMD_H */
