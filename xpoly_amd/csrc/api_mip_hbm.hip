// C ABI of libxpoly_amd.so (include/xpoly_amd.h): MIP tree walks whose node LPs are beyond 64 KB of LDS
// (k_mip_tree_hbm). One of the library's eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "six_host.hip.h"
#include "batch_kernels.hip.h"
#include "mip_tree_hbm.hip.h"
#include "part_instances.hip.h"

using namespace xpg;

namespace xpg {
XPG_BATCH_DEV(extern template, F64) XPG_BATCH_DEV(extern template, R32)
XPG_MIP_SHARED(extern, F64) XPG_MIP_SHARED(extern, R32)
}

extern "C" {
// ---- MIP trees whose node LPs are beyond 64 KB of LDS: the whole walk by a workgroup per tree, node tableaux in device
// ---- memory (mip_tree_hbm.hip.h) ----
int xpg_mip_batch_vc_hbm_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                               const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols, const uint8_t * ind,
                               int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch_vc_hbm<R32>(ctx, 1, nb, is_max != 0, is_bin != 0, (const R32 *)tgtf, (const R32 *)vc, (const R32 *)eq, eq_rows,
                                 (const R32 *)leq, leq_rows, cols, ind, out_status, (R32 *)out_v, (R32 *)out_sol, out_nodes);
}
int xpg_mip_batch_vc_hbm_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf, const double * vc,
                             const double * eq, int eq_rows, const double * leq, int leq_rows, int cols, const uint8_t * ind,
                             int32_t * out_status, double * out_v, double * out_sol, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch_vc_hbm<F64>(ctx, 0, nb, is_max != 0, is_bin != 0, (const F64 *)tgtf, (const F64 *)vc, (const F64 *)eq, eq_rows,
                                 (const F64 *)leq, leq_rows, cols, ind, out_status, (F64 *)out_v, (F64 *)out_sol, out_nodes);
}
// which route the trees of the calling thread's last xpg_mip_batch_vc_hbm_* call took (mip_tree_hbm.hip.h MipHbmRoute)
int xpg_mip_hbm_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const MipHbmRoute & r = mip_hbm_route();
    const long long f[5] = { r.lds, r.hbm, r.host, r.free_vars, r.grid };
    return copy_fields(out, n, f);
}
// host-only test view: the route rule of xpg_mip_batch_vc_hbm_* and the sizes it decides by
int xpg_test_mip_hbm_plan(int kind, int pattern, int leq_rows, int eq_rows, int cols, int is_bin, int is_max, int extra, int nb, int num_cus,
                          long long * out, int n)
{
    if (!out || n < 0 || cols < 2 || leq_rows < 0 || eq_rows < 0 || (leq_rows == 0 && eq_rows == 0) || extra < 0 || extra > cols - 1 ||
        nb <= 0 || num_cus <= 0 || (kind != 0 && kind != 1))
        return XPG_ERR_SHAPE;
    const int ex = pattern ? extra : 0;
    const MipHbmPlan g = kind == 0 ? mip_hbm_plan<F64>(pattern != 0, leq_rows, eq_rows, cols, is_bin != 0, is_max != 0, ex, nb, num_cus)
                                   : mip_hbm_plan<R32>(pattern != 0, leq_rows, eq_rows, cols, is_bin != 0, is_max != 0, ex, nb, num_cus);
    const long long f[11] = { g.route, g.extra, g.R, g.V, (long long)g.lds, (long long)g.slot, g.ld, (long long)g.ws_words, g.threads, g.grid,
                              (long long)g.scratch };
    return copy_fields(out, n, f);
}
} // extern "C"
