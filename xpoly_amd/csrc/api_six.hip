// C ABI of libxpoly_amd.so (include/xpoly_amd.h): SIX::maxm / minm, the LDS-resident LP batches (k_batch,
// k_six_batch_vc), their multi-device and ragged forms. One of the library's eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "six_host.hip.h"
#include "batch_kernels.hip.h"
#include "six_batch_vc.hip.h"
#include "ragged_host.hip.h"
#include "part_instances.hip.h"

using namespace xpg;

namespace xpg {
XPG_BATCH_DEV(template, F64) XPG_BATCH_DEV(template, R32)
XPG_SIX_VC_INSTANCES(template, F64) XPG_SIX_VC_INSTANCES(template, R32)
}

extern "C" {
#ifdef XPG_LIFE
// diagnostic builds (-DXPG_LIFE) only: the per-LP pivot time marks of k_batch (4096 LPs x 32 marks), cleared on read
int xpg_life_debug(xpg_ctx * ctx, unsigned long long * out)
{
    XPG_BIND(ctx);
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_life), sizeof(unsigned long long) * 4096 * 32) != hipSuccess) return XPG_ERR_HIP;
    std::vector<unsigned long long> z(4096 * 32, 0ull);
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_life), z.data(), sizeof(unsigned long long) * 4096 * 32) != hipSuccess) return XPG_ERR_HIP;
    return 0;
}
#endif
#ifdef XPG_STAMPS
// diagnostic builds only: reads and clears sm_solve_lp's tick sums (phase one, plain build, main solve, pivots, counts)
int xpg_lp_solve_debug(xpg_ctx * ctx, unsigned long long * out8)
{
    XPG_BIND(ctx);
    unsigned long long z[8] = {0};
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_lp_ticks), sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_lp_ticks), z, sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    return 0;
}
// diagnostic builds only: reads and clears sm_fast_loop's counters
int xpg_fastloop_debug(xpg_ctx * ctx, unsigned long long * out16)
{
    XPG_BIND(ctx);
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_fl), sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_fl), z, sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    return 0;
}
#endif
// ---- SIX::maxm / minm ---------------------------------------------------------------------
// where the calling thread's last xpg_six_* call spent its time (six_host.hip.h SixProfile)
int xpg_six_last_profile(double * out_ms, int n)
{
    if (!out_ms || n < 0) return XPG_ERR_SHAPE;
    const SixProfile & p = six_profile();
    const double f[9] = { p.total_ms, p.reshape_ms, p.create_ms, p.dual_ms, p.solve_ms, p.read_ms, p.destroy_ms, (double)p.route, (double)p.pivots };
    return copy_fields(out_ms, n, f);
}
int xpg_test_normalize(xpg_ctx * ctx, int kind, const void * tgtf, const void * vc, int vc_rows, const void * eq, int eq_rows,
                       const void * leq, int leq_rows, int cols, void * out_dev_cells, void * out_host_cells, long long cap_cells,
                       int32_t * out_info)
{
    XPG_BIND(ctx);
    if (!ctx || !out_dev_cells || !out_host_cells || !out_info || (kind != 0 && kind != 1)) return XPG_ERR_SHAPE;
    if (kind == 0)
        return test_normalize<F64>(ctx, (const F64 *)tgtf, (const F64 *)vc, vc_rows, (const F64 *)eq, eq_rows, (const F64 *)leq, leq_rows, cols,
                                   (F64 *)out_dev_cells, (F64 *)out_host_cells, cap_cells, out_info);
    return test_normalize<R32>(ctx, (const R32 *)tgtf, (const R32 *)vc, vc_rows, (const R32 *)eq, eq_rows, (const R32 *)leq, leq_rows, cols,
                               (R32 *)out_dev_cells, (R32 *)out_host_cells, cap_cells, out_info);
}
int xpg_six_maxm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows,
                     const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                     unsigned max_iter, double * out_v, double * out_sol)
{
    XPG_BIND(ctx);
    return six_solve<F64>(ctx, 0, true, (const F64 *)tgtf, (const F64 *)vc, vc_rows, (const F64 *)eq,
                          eq_rows, (const F64 *)leq, leq_rows, cols, max_iter, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_minm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows,
                     const double * eq, int eq_rows, const double * leq, int leq_rows, int cols,
                     unsigned max_iter, double * out_v, double * out_sol)
{
    XPG_BIND(ctx);
    return six_solve<F64>(ctx, 0, false, (const F64 *)tgtf, (const F64 *)vc, vc_rows, (const F64 *)eq,
                          eq_rows, (const F64 *)leq, leq_rows, cols, max_iter, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_maxm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc, int vc_rows,
                       const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows,
                       int cols, unsigned max_iter, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return six_solve<R32>(ctx, 1, true, (const R32 *)tgtf, (const R32 *)vc, vc_rows, (const R32 *)eq,
                          eq_rows, (const R32 *)leq, leq_rows, cols, max_iter, (R32 *)out_v, (R32 *)out_sol);
}
int xpg_six_minm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc, int vc_rows,
                       const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows,
                       int cols, unsigned max_iter, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return six_solve<R32>(ctx, 1, false, (const R32 *)tgtf, (const R32 *)vc, vc_rows, (const R32 *)eq,
                          eq_rows, (const R32 *)leq, leq_rows, cols, max_iter, (R32 *)out_v, (R32 *)out_sol);
}

// ---- batches ------------------------------------------------------------------------------
int xpg_six_batch_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * leq,
                          int m, int cols, unsigned max_iter, int32_t * out_status, double * out_v,
                          double * out_sol, uint32_t * out_pivots)
{
    XPG_BIND(ctx);
    return batch_dev<F64>(ctx, is_max, nb, (const F64 *)tgtf, (const F64 *)leq, m, cols, max_iter,
                          out_status, (F64 *)out_v, (F64 *)out_sol, out_pivots);
}
int xpg_six_batch_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf,
                            const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                            int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol,
                            uint32_t * out_pivots)
{
    XPG_BIND(ctx);
    return batch_dev<R32>(ctx, is_max, nb, (const R32 *)tgtf, (const R32 *)leq, m, cols, max_iter,
                          out_status, (R32 *)out_v, (R32 *)out_sol, out_pivots);
}
int xpg_six_batch_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * leq,
                      int m, int cols, unsigned max_iter, int32_t * out_status, double * out_v,
                      double * out_sol)
{
    XPG_BIND(ctx);
    return batch_host<F64>(ctx, is_max, nb, (const F64 *)tgtf, (const F64 *)leq, m, cols, max_iter,
                           out_status, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_batch_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf,
                        const xpg_rat32 * leq, int m, int cols, unsigned max_iter,
                        int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return batch_host<R32>(ctx, is_max, nb, (const R32 *)tgtf, (const R32 *)leq, m, cols, max_iter,
                           out_status, (R32 *)out_v, (R32 *)out_sol);
}

// ---- the same for problems with equalities and free variables: SIX::normalize and calcFinalSolution on the device ----
int xpg_six_batch_vc_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc, const double * eq, int eq_rows,
                         const double * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status, double * out_v,
                         double * out_sol)
{
    XPG_BIND(ctx);
    return six_batch_vc_host<F64>(ctx, 0, is_max != 0, nb, (const F64 *)tgtf, (const F64 *)vc, (const F64 *)eq, eq_rows, (const F64 *)leq,
                                  leq_rows, cols, max_iter, out_status, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_batch_vc_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc, const xpg_rat32 * eq,
                           int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status,
                           xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return six_batch_vc_host<R32>(ctx, 1, is_max != 0, nb, (const R32 *)tgtf, (const R32 *)vc, (const R32 *)eq, eq_rows, (const R32 *)leq,
                                  leq_rows, cols, max_iter, out_status, (R32 *)out_v, (R32 *)out_sol);
}
int xpg_six_batch_vc_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc, const double * eq, int eq_rows,
                             const double * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status, double * out_v,
                             double * out_sol)
{
    XPG_BIND(ctx);
    const int rc = six_batch_vc_dev<F64>(ctx, is_max != 0, nb, (const F64 *)tgtf, (const F64 *)vc, (const F64 *)eq, eq_rows, (const F64 *)leq,
                                         leq_rows, cols, max_iter, -1, out_status, (F64 *)out_v, (F64 *)out_sol);
    six_vc_route() = SixVcRoute{rc == 0 ? nb : 0, 0, -1};
    return rc;
}
int xpg_six_batch_vc_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc, const xpg_rat32 * eq,
                               int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status,
                               xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    const int rc = six_batch_vc_dev<R32>(ctx, is_max != 0, nb, (const R32 *)tgtf, (const R32 *)vc, (const R32 *)eq, eq_rows, (const R32 *)leq,
                                         leq_rows, cols, max_iter, -1, out_status, (R32 *)out_v, (R32 *)out_sol);
    six_vc_route() = SixVcRoute{rc == 0 ? nb : 0, 0, -1};
    return rc;
}
// which route the LPs of the calling thread's last xpg_six_batch_vc_* call took (six_batch_vc.hip.h SixVcRoute)
int xpg_six_batch_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const SixVcRoute & r = six_vc_route();
    const long long f[3] = { r.device, r.fallback, r.free_vars };
    return copy_fields(out, n, f);
}
// host-only test view: the route rule of xpg_six_batch_vc_* and the sizes it decides by
int xpg_test_six_batch_vc_plan(int kind, const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int is_max, long long * out, int n)
{
    if (!vc || !out || n < 0 || cols < 2 || vc_rows != cols - 1 || leq_rows < 0 || eq_rows < 0 || (leq_rows == 0 && eq_rows == 0) ||
        (kind != 0 && kind != 1))
        return XPG_ERR_SHAPE;
    const VcView v = kind == 0 ? vc_view<F64>(vc, vc_rows, cols) : vc_view<R32>(vc, vc_rows, cols);
    const SixVcPlan p = kind == 0 ? six_vc_plan<F64>(v.pattern, v.zero_cols, leq_rows, eq_rows, cols, is_max != 0)
                                  : six_vc_plan<R32>(v.pattern, v.zero_cols, leq_rows, eq_rows, cols, is_max != 0);
    const long long f[5] = { p.device, p.nfree, p.rows_max, p.n, (long long)p.lds };
    return copy_fields(out, n, f);
}

// ---- the same batches over several devices: one context + host thread per shard (run_sharded) ----
int xpg_six_batch_f64_multi(int ndev, const int * devices, int is_max, int nb, const double * tgtf, const double * leq,
                            int m, int cols, unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol)
{
    if (!tgtf || !leq || m <= 0 || cols < 2 || !out_status || !out_v || !out_sol) return XPG_ERR_SHAPE;
    return run_sharded(ndev, devices, nb, [=](xpg_ctx * c, int lo, int hi) {
        return xpg_six_batch_f64(c, is_max, hi - lo, tgtf + (size_t)lo * cols, leq + (size_t)lo * m * cols, m, cols, max_iter,
                                 out_status + lo, out_v + lo, out_sol + (size_t)lo * cols);
    });
}
int xpg_six_batch_rat32_multi(int ndev, const int * devices, int is_max, int nb, const xpg_rat32 * tgtf,
                              const xpg_rat32 * leq, int m, int cols, unsigned max_iter, int32_t * out_status,
                              xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    if (!tgtf || !leq || m <= 0 || cols < 2 || !out_status || !out_v || !out_sol) return XPG_ERR_SHAPE;
    return run_sharded(ndev, devices, nb, [=](xpg_ctx * c, int lo, int hi) {
        return xpg_six_batch_rat32(c, is_max, hi - lo, tgtf + (size_t)lo * cols, leq + (size_t)lo * m * cols, m, cols,
                                   max_iter, out_status + lo, out_v + lo, out_sol + (size_t)lo * cols);
    });
}
} // extern "C"
namespace {
template <class S>
int six_batch_ragged(xpg_ctx * ctx, int is_max, int nb, const S * tgtf, const S * leq, const int32_t * rows, const int32_t * cols,
                     const long long * leq_off, const long long * tg_off, unsigned max_iter, int32_t * out_status, S * out_v, S * out_sol)
{
    if (!ctx || nb < 0 || !tgtf || !leq || !rows || !cols || !leq_off || !tg_off || !out_status || !out_v || !out_sol) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    // ONE launch of the LDS-resident kernel with per-LP shapes (k_batch_ragged): the concatenated arrays go up as they
    // are, the LDS request is that of the largest LP. (Classes on concurrent lanes -- run_ragged, what the other ragged
    // entry points do -- remain the fallback for a batch whose largest LP does not fit one CU's LDS.)
    int max_R = 0, max_V = 0;
    long long leq_cells = 0, tg_cells = 0;
    for (int b = 0; b < nb; b++) {
        if (rows[b] <= 0 || cols[b] < 2 || leq_off[b] < 0 || tg_off[b] < 0) return XPG_ERR_SHAPE;
        const int n = cols[b] - 1, R = is_max ? rows[b] : n, V = is_max ? n : rows[b];
        max_R = R > max_R ? R : max_R; max_V = V > max_V ? V : max_V;
        const long long le = leq_off[b] + (long long)rows[b] * cols[b], te = tg_off[b] + cols[b];
        leq_cells = le > leq_cells ? le : leq_cells; tg_cells = te > tg_cells ? te : tg_cells;
    }
    if (small_lds_fits<S>(max_R, max_V)) {
        const size_t bl = (size_t)leq_cells * 8, bt = (size_t)tg_cells * 8;
        DevBuf dl, dt, ds, dv, dst, dr, dc, dlo, dto;
        XPG_TRY(dl.alloc(ctx, bl)); XPG_TRY(dt.alloc(ctx, bt)); XPG_TRY(ds.alloc(ctx, bt)); XPG_TRY(dv.alloc(ctx, (size_t)nb * 8));
        XPG_TRY(dst.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dr.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dc.alloc(ctx, (size_t)nb * 4));
        XPG_TRY(dlo.alloc(ctx, (size_t)nb * 8)); XPG_TRY(dto.alloc(ctx, (size_t)nb * 8));
        XPG_TRY(hipMemcpyAsync(dl.p, leq, bl, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dt.p, tgtf, bt, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(ds.p, out_sol, bt, hipMemcpyHostToDevice, ctx->stream));     // (slots of unsolved LPs keep what they held)
        XPG_TRY(hipMemcpyAsync(dr.p, rows, (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dc.p, cols, (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dlo.p, leq_off, (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dto.p, tg_off, (size_t)nb * 8, hipMemcpyHostToDevice, ctx->stream));
        const int rc = batch_dev_ragged<S>(ctx, is_max, nb, (const S *)dt.p, (const S *)dl.p, (const int *)dr.p, (const int *)dc.p,
                                           (const long long *)dlo.p, (const long long *)dto.p, max_R, max_V, max_iter,
                                           (int32_t *)dst.p, (S *)dv.p, (S *)ds.p);
        if (rc) return rc;
        XPG_TRY(hipMemcpyAsync(out_status, dst.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipMemcpyAsync(out_v, dv.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipMemcpyAsync(out_sol, ds.p, bt, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        return 0;
    }
    return run_ragged(ctx, nb, rows, cols, [&](xpg_ctx * c, const RaggedClass & g) {
        const size_t ng = g.idx.size();
        std::vector<S> bl, bt, bs(ng * (size_t)g.cols), bv(ng); std::vector<int32_t> st(ng);
        ragged_gather(bl, leq, leq_off, g, (size_t)g.rows * g.cols);
        ragged_gather(bt, tgtf, tg_off, g, (size_t)g.cols);
        ragged_gather(bs, (const S *)out_sol, tg_off, g, (size_t)g.cols);     // (slots of unsolved LPs keep what they held)
        const int r = batch_host<S>(c, is_max, (int)ng, bt.data(), bl.data(), g.rows, g.cols, max_iter, st.data(), bv.data(), bs.data());
        if (r) return r;
        for (size_t k = 0; k < ng; k++) {
            const int b = g.idx[k];
            out_status[b] = st[k]; out_v[b] = bv[k];
            memcpy((void *)(out_sol + tg_off[b]), (const void *)(bs.data() + k * (size_t)g.cols), (size_t)g.cols * sizeof(S));
        }
        return 0;
    });
}
} // namespace
extern "C" {
int xpg_six_batch_f64_ragged(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * leq, const int32_t * rows,
                             const int32_t * cols, const long long * leq_offsets, const long long * tgtf_offsets,
                             unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol)
{
    XPG_BIND(ctx);
    return six_batch_ragged<F64>(ctx, is_max, nb, (const F64 *)tgtf, (const F64 *)leq, rows, cols, leq_offsets, tgtf_offsets, max_iter,
                                 out_status, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_batch_rat32_ragged(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * leq, const int32_t * rows,
                               const int32_t * cols, const long long * leq_offsets, const long long * tgtf_offsets,
                               unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return six_batch_ragged<R32>(ctx, is_max, nb, (const R32 *)tgtf, (const R32 *)leq, rows, cols, leq_offsets, tgtf_offsets, max_iter,
                                 out_status, (R32 *)out_v, (R32 *)out_sol);
}
} // extern "C"
