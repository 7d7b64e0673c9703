// C ABI of libxpoly_amd.so (include/xpoly_amd.h): LP batches beyond one CU's LDS (k_batch_hbm). One of the library's
// eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "batch_hbm.hip.h"
#include "part_instances.hip.h"

using namespace xpg;

namespace xpg { XPG_BATCH_DEV(extern template, F64) XPG_BATCH_DEV(extern template, R32) }

extern "C" {
// ---- batches of LPs beyond one CU's LDS: a workgroup per LP on a tableau in global memory (batch_hbm.hip.h) ----
int xpg_six_batch_hbm_f64(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * leq, int m, int cols,
                          unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol)
{
    XPG_BIND(ctx);
    return batch_hbm_host<F64>(ctx, is_max, nb, (const F64 *)tgtf, (const F64 *)leq, m, cols, max_iter, out_status, (F64 *)out_v, (F64 *)out_sol);
}
int xpg_six_batch_hbm_rat32(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * leq, int m, int cols,
                            unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND(ctx);
    return batch_hbm_host<R32>(ctx, is_max, nb, (const R32 *)tgtf, (const R32 *)leq, m, cols, max_iter, out_status, (R32 *)out_v, (R32 *)out_sol);
}
int xpg_six_batch_hbm_f64_dev(xpg_ctx * ctx, int is_max, int nb, const double * tgtf, const double * leq, int m, int cols,
                              unsigned max_iter, int32_t * out_status, double * out_v, double * out_sol, uint32_t * out_pivots)
{
    XPG_BIND(ctx);
    return batch_hbm_dev<F64>(ctx, is_max, nb, (const F64 *)tgtf, (const F64 *)leq, m, cols, max_iter, out_status, (F64 *)out_v, (F64 *)out_sol,
                              out_pivots);
}
int xpg_six_batch_hbm_rat32_dev(xpg_ctx * ctx, int is_max, int nb, const xpg_rat32 * tgtf, const xpg_rat32 * leq, int m, int cols,
                                unsigned max_iter, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol, uint32_t * out_pivots)
{
    XPG_BIND(ctx);
    return batch_hbm_dev<R32>(ctx, is_max, nb, (const R32 *)tgtf, (const R32 *)leq, m, cols, max_iter, out_status, (R32 *)out_v, (R32 *)out_sol,
                              out_pivots);
}
// which route the LPs of the calling thread's last xpg_six_batch_hbm_* call took (batch_hbm.hip.h BatchHbmRoute)
int xpg_six_batch_hbm_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const BatchHbmRoute & r = batch_hbm_route();
    const long long f[3] = { r.lds, r.hbm, r.grid };
    return copy_fields(out, n, f);
}
// host-only test view: what xpg_six_batch_hbm_* would do with nb LPs solved as R rows x V variables on num_cus compute units
int xpg_test_batch_hbm_geometry(int kind, int R, int V, int nb, int num_cus, long long * out, int n)
{
    if (!out || n < 0 || R <= 0 || V <= 0 || nb <= 0 || num_cus <= 0 || (kind != 0 && kind != 1)) return XPG_ERR_SHAPE;
    const HbmGeom g = kind == 0 ? batch_hbm_geometry<F64>(R, V, nb, num_cus) : batch_hbm_geometry<R32>(R, V, nb, num_cus);
    const long long f[7] = { g.route, (long long)g.lds, (long long)g.slot, g.ld, g.threads, g.grid, (long long)g.scratch };
    return copy_fields(out, n, f);
}
} // extern "C"
