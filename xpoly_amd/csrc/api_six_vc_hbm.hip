// C ABI of libxpoly_amd.so (include/xpoly_amd.h): LP batches with equalities and free variables beyond one CU's LDS
// (k_six_batch_vc_hbm). One of the library's eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "six_batch_vc_hbm.hip.h"
#include "part_instances.hip.h"

using namespace xpg;

namespace xpg { XPG_SIX_VC_INSTANCES(extern template, F64) XPG_SIX_VC_INSTANCES(extern template, R32) }

extern "C" {
// ---- batches with equalities and free variables beyond 64 KB of LDS: normalize, solve and finish by a workgroup per LP on
// ---- a slot in global memory (six_batch_vc_hbm.hip.h) ----
int xpg_six_batch_vc_hbm_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc, const double * eq, int eq_rows,
                             const double * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status, double * out_v,
                             double * out_sol)
{
    XPG_BIND(ctx);
    return six_batch_vc_hbm_host<F64>(ctx, 0, is_max != 0, nb, (const F64 *)tgtf, (const F64 *)vc, (const F64 *)eq, eq_rows, (const F64 *)leq,
                                      leq_rows, cols, max_iter, out_status, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_batch_vc_hbm_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc, const xpg_rat32 * eq,
                               int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status,
                               xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return six_batch_vc_hbm_host<R32>(ctx, 1, is_max != 0, nb, (const R32 *)tgtf, (const R32 *)vc, (const R32 *)eq, eq_rows, (const R32 *)leq,
                                      leq_rows, cols, max_iter, out_status, (R32 *)out_v, (R32 *)out_sol);
}
int xpg_six_batch_vc_hbm_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * vc, const double * eq, int eq_rows,
                                 const double * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status, double * out_v,
                                 double * out_sol, uint32_t * out_pivots)
{
    XPG_BIND(ctx);
    return six_batch_vc_hbm_dev<F64>(ctx, is_max != 0, nb, (const F64 *)tgtf, (const F64 *)vc, (const F64 *)eq, eq_rows, (const F64 *)leq,
                                     leq_rows, cols, max_iter, out_status, (F64 *)out_v, (F64 *)out_sol, out_pivots);
}
int xpg_six_batch_vc_hbm_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * vc, const xpg_rat32 * eq,
                                   int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status,
                                   xpg_rat32 * out_v, xpg_rat32 * out_sol, uint32_t * out_pivots)
{
    XPG_BIND(ctx);
    return six_batch_vc_hbm_dev<R32>(ctx, is_max != 0, nb, (const R32 *)tgtf, (const R32 *)vc, (const R32 *)eq, eq_rows, (const R32 *)leq,
                                     leq_rows, cols, max_iter, out_status, (R32 *)out_v, (R32 *)out_sol, out_pivots);
}
// which route the LPs of the calling thread's last xpg_six_batch_vc_hbm_* call took (six_batch_vc_hbm.hip.h SixVcHbmRoute)
int xpg_six_batch_vc_hbm_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const SixVcHbmRoute & r = six_vc_hbm_route();
    const long long f[5] = { r.lds, r.hbm, r.fallback, r.free_vars, r.grid };
    return copy_fields(out, n, f);
}
// host-only test view: the route rule of xpg_six_batch_vc_hbm_* and the sizes it decides by; vc == NULL: the _dev forms' view
int xpg_test_six_batch_vc_hbm_plan(int kind, const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int is_max, int nb, int num_cus,
                                   long long * out, int n)
{
    if (!out || n < 0 || cols < 2 || (vc && vc_rows != cols - 1) || leq_rows < 0 || eq_rows < 0 || (leq_rows == 0 && eq_rows == 0) || nb <= 0 ||
        num_cus <= 0 || (kind != 0 && kind != 1))
        return XPG_ERR_SHAPE;
    const VcView v = kind == 0 ? vc_view<F64>(vc, vc_rows, cols) : vc_view<R32>(vc, vc_rows, cols);
    const SixVcHbmPlan g = kind == 0 ? six_vc_hbm_plan<F64>(v.pattern, v.nfree, leq_rows, eq_rows, cols, is_max != 0, nb, num_cus)
                                     : six_vc_hbm_plan<R32>(v.pattern, v.nfree, leq_rows, eq_rows, cols, is_max != 0, nb, num_cus);
    const long long f[10] = { g.route, g.nfree, g.Rmax, g.Vmax, (long long)g.lds, (long long)g.slot, g.ld, g.threads, g.grid, (long long)g.scratch };
    return copy_fields(out, n, f);
}
} // extern "C"
