// C ABI of libxpoly_amd.so (include/xpoly_amd.h): MIP (device tree walk + host controller), has_solution, the
// DepPoly::is_empty front end. One of the library's eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "six_host.hip.h"
#include "batch_kernels.hip.h"
#include "mip_front.hip.h"
#include "ragged_host.hip.h"
#include "part_instances.hip.h"

using namespace xpg;

namespace xpg {
XPG_BATCH_DEV(extern template, F64) XPG_BATCH_DEV(extern template, R32)
XPG_MIP_SHARED(, F64) XPG_MIP_SHARED(, R32)
XPG_MIP_TREE_LAUNCH(, R32)
}

extern "C" {
int xpg_mip_batch_rat32_multi(int ndev, const int * devices, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf,
                              const xpg_rat32 * leq, int leq_rows, int cols, int32_t * out_status, xpg_rat32 * out_v,
                              xpg_rat32 * out_sol, long long * out_nodes)
{
    if (!tgtf || !leq || leq_rows <= 0 || cols < 2 || !out_status || !out_v || !out_sol) return XPG_ERR_SHAPE;
    std::atomic<long long> nodes(0);
    const int rc = run_sharded(ndev, devices, nb, [=, &nodes](xpg_ctx * c, int lo, int hi) {
        long long n = 0;
        const int r = xpg_mip_batch_rat32(c, hi - lo, is_max, is_bin, tgtf + (size_t)lo * cols,
                                          leq + (size_t)lo * leq_rows * cols, leq_rows, cols, out_status + lo, out_v + lo,
                                          out_sol + (size_t)lo * cols, &n);
        nodes += n;
        return r;
    });
    if (out_nodes) *out_nodes = nodes.load();
    return rc;
}
int xpg_dep_is_empty_batch_rat32_multi(int ndev, const int * devices, int nb, const xpg_rat32 * mats, int rows, int cols,
                                       int32_t * out_empty, long long * out_nodes)
{
    if (!mats || rows <= 0 || cols < 2 || !out_empty) return XPG_ERR_SHAPE;
    std::atomic<long long> nodes(0);
    const int rc = run_sharded(ndev, devices, nb, [=, &nodes](xpg_ctx * c, int lo, int hi) {
        long long n = 0;
        const int r = xpg_dep_is_empty_batch_rat32(c, hi - lo, mats + (size_t)lo * rows * cols, rows, cols, out_empty + lo, &n);
        nodes += n;
        return r;
    });
    if (out_nodes) *out_nodes = nodes.load();
    return rc;
}

int xpg_dep_is_empty_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows,
                                        const int32_t * cols, const long long * offsets, int32_t * out_empty,
                                        long long * out_nodes)
{
    XPG_BIND(ctx);
    if (out_nodes) *out_nodes = 0;
    if (!ctx || nb < 0) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;                                          // an empty SCoP: nothing to answer (mats may be null)
    if (!rows || !cols || !offsets || !out_empty) return XPG_ERR_SHAPE;
    // DepPoly::is_empty answers true for a polyhedron without rows before it looks at anything else (poly.cpp:533-535):
    // those are answered here and left out of the shape classes
    std::vector<int32_t> lrows, lcols; std::vector<long long> loff; std::vector<int> lidx;
    for (int b = 0; b < nb; b++) {
        if (rows[b] < 0) return XPG_ERR_SHAPE;
        if (rows[b] == 0) { out_empty[b] = 1; continue; }
        lrows.push_back(rows[b]); lcols.push_back(cols[b]); loff.push_back(offsets[b]); lidx.push_back(b);
    }
    if (lidx.empty()) return 0;
    if (!mats) return XPG_ERR_SHAPE;
    std::atomic<long long> nodes(0);
    const int rc = run_ragged(ctx, (int)lidx.size(), lrows.data(), lcols.data(), [&](xpg_ctx * c, const RaggedClass & g) {
        std::vector<R32> buf; std::vector<int32_t> emp(g.idx.size());
        ragged_gather(buf, (const R32 *)mats, loff.data(), g, (size_t)g.rows * g.cols);
        long n = 0;
        const int r = dep_is_empty_batch(c, (int)g.idx.size(), buf.data(), g.rows, g.cols, g.cols - 1, (const R32 *)0, emp.data(), &n);
        if (r) return r;
        for (size_t k = 0; k < g.idx.size(); k++) out_empty[lidx[(size_t)g.idx[k]]] = emp[k];
        nodes += n;
        return 0;
    });
    if (out_nodes) *out_nodes = nodes.load();
    return rc;
}

#ifdef XPG_STAMPS
// diagnostic builds only: reads and clears the tick sums of k_mip_tree (build, solve, feed)
int xpg_mip_debug(xpg_ctx * ctx, unsigned long long * out4)
{
    XPG_BIND(ctx);
    unsigned long long z[4] = {0};
    if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_mip_ticks), sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_mip_ticks), z, sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    return 0;
}
#endif
// ---- MIP / has_solution -------------------------------------------------------------------------
int xpg_mip_maxm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc, int vc_rows,
                       const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols,
                       int is_bin, const uint8_t * ind, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND_MIP(ctx);
    return mip_solve<R32>(ctx, 1, true, is_bin != 0, (const R32 *)tgtf, (const R32 *)vc, vc_rows, (const R32 *)eq,
                          eq_rows, (const R32 *)leq, leq_rows, cols, ind, (R32 *)out_v, (R32 *)out_sol, 0);
}
int xpg_mip_minm_rat32(xpg_ctx * ctx, const xpg_rat32 * tgtf, const xpg_rat32 * vc, int vc_rows,
                       const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols,
                       int is_bin, const uint8_t * ind, xpg_rat32 * out_v, xpg_rat32 * out_sol)
{
    XPG_BIND_MIP(ctx);
    return mip_solve<R32>(ctx, 1, false, is_bin != 0, (const R32 *)tgtf, (const R32 *)vc, vc_rows, (const R32 *)eq,
                          eq_rows, (const R32 *)leq, leq_rows, cols, ind, (R32 *)out_v, (R32 *)out_sol, 0);
}
int xpg_mip_maxm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows, const double * eq,
                     int eq_rows, const double * leq, int leq_rows, int cols, int is_bin, const uint8_t * ind,
                     double * out_v, double * out_sol)
{
    XPG_BIND_MIP(ctx);
    return mip_solve<F64>(ctx, 0, true, is_bin != 0, (const F64 *)tgtf, (const F64 *)vc, vc_rows, (const F64 *)eq,
                          eq_rows, (const F64 *)leq, leq_rows, cols, ind, (F64 *)out_v, (F64 *)out_sol, 0);
}
int xpg_mip_minm_f64(xpg_ctx * ctx, const double * tgtf, const double * vc, int vc_rows, const double * eq,
                     int eq_rows, const double * leq, int leq_rows, int cols, int is_bin, const uint8_t * ind,
                     double * out_v, double * out_sol)
{
    XPG_BIND_MIP(ctx);
    return mip_solve<F64>(ctx, 0, false, is_bin != 0, (const F64 *)tgtf, (const F64 *)vc, vc_rows, (const F64 *)eq,
                          eq_rows, (const F64 *)leq, leq_rows, cols, ind, (F64 *)out_v, (F64 *)out_sol, 0);
}
int xpg_has_solution_rat32(xpg_ctx * ctx, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                           const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_int_sol,
                           int is_unique_sol)
{
    XPG_BIND_MIP(ctx);
    return has_solution(ctx, (const R32 *)leq, leq_rows, (const R32 *)eq, eq_rows, (const R32 *)vc, vc_rows, cols,
                        rhs_idx, is_int_sol != 0, is_unique_sol != 0);
}

int xpg_mip_batch_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf, const xpg_rat32 * leq,
                        int leq_rows, int cols, int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol,
                        long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch<R32>(ctx, 1, nb, is_max != 0, is_bin != 0, (const R32 *)tgtf, (const R32 *)leq, leq_rows, cols,
                          out_status, (R32 *)out_v, (R32 *)out_sol, out_nodes);
}
int xpg_mip_batch_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf, const double * leq,
                      int leq_rows, int cols, int32_t * out_status, double * out_v, double * out_sol, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch<F64>(ctx, 0, nb, is_max != 0, is_bin != 0, (const F64 *)tgtf, (const F64 *)leq, leq_rows, cols,
                          out_status, (F64 *)out_v, (F64 *)out_sol, out_nodes);
}
int xpg_mip_batch_eq_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf, const xpg_rat32 * leq,
                           int leq_rows, const xpg_rat32 * eq, int eq_rows, int cols, int32_t * out_status, xpg_rat32 * out_v,
                           xpg_rat32 * out_sol, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch_eq<R32>(ctx, 1, nb, is_max != 0, is_bin != 0, (const R32 *)tgtf, (const R32 *)leq, leq_rows, (const R32 *)eq, eq_rows,
                             cols, out_status, (R32 *)out_v, (R32 *)out_sol, out_nodes);
}
int xpg_mip_batch_eq_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf, const double * leq, int leq_rows,
                         const double * eq, int eq_rows, int cols, int32_t * out_status, double * out_v, double * out_sol,
                         long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch_eq<F64>(ctx, 0, nb, is_max != 0, is_bin != 0, (const F64 *)tgtf, (const F64 *)leq, leq_rows, (const F64 *)eq, eq_rows,
                             cols, out_status, (F64 *)out_v, (F64 *)out_sol, out_nodes);
}
int xpg_dep_is_empty_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols,
                                 int32_t * out_empty, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    long n = 0;
    int rc = dep_is_empty_batch(ctx, nb, (const R32 *)mats, rows, cols, cols - 1, (const R32 *)0, out_empty, &n);
    if (out_nodes) *out_nodes = n;
    return rc;
}
int xpg_dep_is_empty_batch_ex_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                    const xpg_rat32 * vc, int32_t * out_empty, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    long n = 0;
    int rc = dep_is_empty_batch(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, (const R32 *)vc, out_empty, &n);
    if (out_nodes) *out_nodes = n;
    return rc;
}
int xpg_dep_is_empty_batch_mode_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                      const xpg_rat32 * vc, int mode, int32_t * out_empty, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    if (mode != XPG_DEP_PARITY && mode != XPG_DEP_SYMBOLS_AS_VARS) return XPG_ERR_SHAPE;
    long n = 0;
    int rc = dep_is_empty_batch(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, (const R32 *)vc, out_empty, &n, mode == XPG_DEP_SYMBOLS_AS_VARS ? 1 : 0);
    if (out_nodes) *out_nodes = n;
    return rc;
}
int xpg_mip_batch_vc_rat32(xpg_ctx * ctx, int nb, int is_max, int is_bin, const xpg_rat32 * tgtf, const xpg_rat32 * vc,
                           const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * leq, int leq_rows, int cols, const uint8_t * ind,
                           int32_t * out_status, xpg_rat32 * out_v, xpg_rat32 * out_sol, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch_vc<R32>(ctx, 1, nb, is_max != 0, is_bin != 0, (const R32 *)tgtf, (const R32 *)vc, (const R32 *)eq, eq_rows,
                             (const R32 *)leq, leq_rows, cols, ind, out_status, (R32 *)out_v, (R32 *)out_sol, out_nodes);
}
int xpg_mip_batch_vc_f64(xpg_ctx * ctx, int nb, int is_max, int is_bin, const double * tgtf, const double * vc,
                         const double * eq, int eq_rows, const double * leq, int leq_rows, int cols, const uint8_t * ind,
                         int32_t * out_status, double * out_v, double * out_sol, long long * out_nodes)
{
    XPG_BIND_MIP(ctx);
    return mip_batch_vc<F64>(ctx, 0, nb, is_max != 0, is_bin != 0, (const F64 *)tgtf, (const F64 *)vc, (const F64 *)eq, eq_rows,
                             (const F64 *)leq, leq_rows, cols, ind, out_status, (F64 *)out_v, (F64 *)out_sol, out_nodes);
}
// which route the trees of the calling thread's last MIP / has_solution / dep_is_empty call took (mip_host.hip.h MipRoute)
int xpg_mip_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const MipRoute & r = mip_route();
    const long long f[3] = { r.device_trees, r.host_trees, r.free_vars };
    return copy_fields(out, n, f);
}
// host-only test views: the vc classifier, the LDS fit test and the route rule of the MIP entry points
int xpg_test_vc_pattern(int kind, const void * vc, int vc_rows, int cols, uint8_t * out_free)
{
    if (!vc || !out_free || cols < 2 || vc_rows != cols - 1 || (kind != 0 && kind != 1)) return XPG_ERR_SHAPE;
    std::vector<int> fv;
    const bool pat = kind == 0 ? vc_sign_pattern((const F64 *)vc, vc_rows, cols, fv) : vc_sign_pattern((const R32 *)vc, vc_rows, cols, fv);
    for (int j = 0; j < cols - 1; j++) out_free[j] = 0;
    if (!pat) return 0;
    for (size_t k = 0; k < fv.size(); k++) out_free[fv[k]] = 1;
    return 1;
}
int xpg_test_mip_fits(int kind, int leq_rows, int eq_rows, int cols, int is_bin, int extra)
{
    if (cols < 2 || leq_rows < 0 || eq_rows < 0 || extra < 0 || (kind != 0 && kind != 1)) return XPG_ERR_SHAPE;
    return (kind == 0 ? mip_device_fits<F64>(leq_rows, cols, is_bin != 0, eq_rows, extra)
                      : mip_device_fits<R32>(leq_rows, cols, is_bin != 0, eq_rows, extra)) ? 1 : 0;
}
// mip_front_route as an entry point with fit test `fit` (mip_host.hip.h MipFit) asks it; allowed stands for XPG_MIP_DEVICE
int xpg_test_mip_front_route(int fit, int kind, int pattern, int extra, int leq_rows, int eq_rows, int cols, int is_bin, int is_max, int allowed)
{
    if ((fit != MIP_FIT_LAUNCH && fit != MIP_FIT_BOTH) || (kind != 0 && kind != 1) || cols < 2 || leq_rows < 0 || eq_rows < 0 ||
        (leq_rows == 0 && eq_rows == 0) || extra < 0)
        return XPG_ERR_SHAPE;
    return (kind == 0 ? mip_front_route<F64>((MipFit)fit, pattern != 0, extra, leq_rows, eq_rows, cols, is_bin != 0, is_max != 0, allowed != 0)
                      : mip_front_route<R32>((MipFit)fit, pattern != 0, extra, leq_rows, eq_rows, cols, is_bin != 0, is_max != 0, allowed != 0)) ? 1 : 0;
}
// what batch_dev would launch nb LPs solved as R rows x V variables with, on a device of num_cus compute units
int xpg_test_batch_geometry(int kind, int R, int V, int nb, int num_cus, long long * out, int n)
{
    if (!out || n < 0 || R <= 0 || V <= 0 || nb <= 0 || num_cus <= 0 || (kind != 0 && kind != 1)) return XPG_ERR_SHAPE;
    const BatchGeom g = kind == 0 ? batch_geometry<F64>(R, V, nb, num_cus) : batch_geometry<R32>(R, V, nb, num_cus);
    const long long f[10] = { (long long)g.lds, g.refused, g.cells, g.threads, g.per_cu, g.five, g.grid, g.seats, g.slice_shape, g.slice_crowded };
    return copy_fields(out, n, f);
}
} // extern "C"
