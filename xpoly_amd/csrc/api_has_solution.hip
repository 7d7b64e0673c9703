// C ABI of libxpoly_amd.so (include/xpoly_amd.h): batched has_solution (k_has_solution_batch, k_has_solution_batch_hbm,
// their forms for mixed shapes k_has_solution_ragged, k_has_solution_ragged_hbm) and its integer form on the device
// (k_hs_int_objective, k_hs_int_update, k_has_solution_int_hbm). One of the library's eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "has_solution_batch.hip.h"
#include "has_solution_int.hip.h"
#include "part_instances.hip.h"

using namespace xpg;

namespace xpg { XPG_MIP_TREE_LAUNCH(extern, R32) }

extern "C" {
// ---- Lineq::has_solution for a batch: maxm, then minm where still open, one launch (has_solution_batch.hip.h) ----
int xpg_has_solution_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                                 const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_int_sol, int is_unique_sol,
                                 unsigned max_iter, int32_t * out_has, int32_t * out_status)
{
    XPG_BIND(ctx);
    const size_t lc = (size_t)(leq_rows > 0 ? leq_rows : 0) * cols, ec = (size_t)(eq_rows > 0 ? eq_rows : 0) * cols;
    if (is_int_sol)       // the two walks are another part's (mip_tree_hbm.hip.h): its C entry point
        return has_solution_batch_int(ctx, nb, (const R32 *)leq, leq_rows, (const R32 *)eq, eq_rows, (const R32 *)vc, vc_rows, cols, rhs_idx,
                                      is_unique_sol != 0, out_has, out_status,
                                      [&](int is_max, int count, const R32 * tg, const R32 * e, const R32 * l, int32_t * st) {
            std::vector<R32> v((size_t)count), sol((size_t)count * cols);
            return xpg_mip_batch_vc_hbm_rat32(ctx, count, is_max, 0, (const xpg_rat32 *)tg, vc, (const xpg_rat32 *)e, eq_rows, (const xpg_rat32 *)l,
                                              leq_rows, cols, (const uint8_t *)0, st, (xpg_rat32 *)v.data(), (xpg_rat32 *)sol.data(), (long long *)0);
        });
    return has_solution_batch_host<R32>(ctx, nb, (const R32 *)leq, leq_rows, (const R32 *)eq, eq_rows, (const R32 *)vc, vc_rows, cols, rhs_idx,
                                        is_unique_sol != 0, max_iter, out_has, out_status, [&](int b) {   // has_solution() is another part's (mip_front.hip.h)
        return xpg_has_solution_rat32(ctx, leq + (size_t)b * lc, leq_rows, eq_rows > 0 ? eq + (size_t)b * ec : (const xpg_rat32 *)0, eq_rows, vc,
                                      vc_rows, cols, rhs_idx, 0, is_unique_sol);
    });
}
int xpg_has_solution_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                                     const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_int_sol, int is_unique_sol,
                                     unsigned max_iter, int32_t * out_has, int32_t * out_status)
{
    XPG_BIND(ctx);
    return has_solution_batch_dev<R32>(ctx, nb, (const R32 *)leq, leq_rows, (const R32 *)eq, eq_rows, (const R32 *)vc, vc_rows, cols, rhs_idx,
                                       is_int_sol != 0, is_unique_sol != 0, max_iter, out_has, out_status);
}
// what the calling thread's last xpg_has_solution_batch_* call did (has_solution_batch.hip.h HsRoute)
int xpg_has_solution_batch_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const HsRoute & r = hs_route();
    const long long f[5] = { r.lds, r.hbm, r.host, r.second, r.grid };
    return copy_fields(out, n, f);
}
// host-only test view: the route rule of xpg_has_solution_batch_* and the sizes it decides by; vc == NULL: the _dev form's view
int xpg_test_has_solution_batch_plan(const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int nb, int num_cus, long long * out, int n)
{
    if (!out || n < 0 || cols < 2 || (vc && vc_rows != cols - 1) || leq_rows <= 0 || eq_rows < 0 || nb <= 0 || num_cus <= 0) return XPG_ERR_SHAPE;
    const VcView v = vc_view<R32>(vc, vc_rows, cols);
    const HsPlan g = hs_plan<R32>(v.pattern, v.nfree, leq_rows, eq_rows, cols, nb, num_cus);
    const long long f[9] = { g.route, g.nfree, g.Rmax, (long long)g.lds, (long long)g.slot, g.ld, g.threads, g.grid, (long long)g.scratch };
    return copy_fields(out, n, f);
}
// ---- the same for systems of mixed shapes under one vc: every system on the route of its own shape, one launch per route ----
int xpg_has_solution_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets,
                                        const xpg_rat32 * eq, const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc,
                                        int vc_rows, int cols, int rhs_idx, int is_int_sol, int is_unique_sol, unsigned max_iter,
                                        int32_t * out_has, int32_t * out_status)
{
    XPG_BIND(ctx);
    if (is_int_sol)
        return has_solution_ragged_int(ctx, nb, (const R32 *)leq, leq_rows, leq_offsets, (const R32 *)eq, eq_rows, eq_offsets, (const R32 *)vc, vc_rows,
                                       cols, rhs_idx, out_has, out_status,
                                       [&](int lr, int er, int count, const R32 * l, const R32 * e, int32_t * has, int32_t * st) {
            return xpg_has_solution_batch_rat32(ctx, count, (const xpg_rat32 *)l, lr, (const xpg_rat32 *)e, er, vc, vc_rows, cols, rhs_idx, 1,
                                                is_unique_sol, max_iter, has, st);
        });
    return has_solution_ragged_host<R32>(ctx, nb, (const R32 *)leq, leq_rows, leq_offsets, (const R32 *)eq, eq_rows, eq_offsets, (const R32 *)vc,
                                         vc_rows, cols, rhs_idx, is_unique_sol != 0, max_iter, out_has, out_status, [&](int b) {
        return xpg_has_solution_rat32(ctx, leq + leq_offsets[b], leq_rows[b], eq_rows[b] > 0 ? eq + eq_offsets[b] : (const xpg_rat32 *)0, eq_rows[b],
                                      vc, vc_rows, cols, rhs_idx, 0, is_unique_sol);
    });
}
// what the calling thread's last xpg_has_solution_batch_ragged_rat32 call did (has_solution_batch.hip.h HsRaggedRoute)
int xpg_has_solution_batch_ragged_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const HsRaggedRoute & r = hs_ragged_route();
    const long long f[7] = { r.lds, r.hbm, r.host, r.second, r.grid_lds, r.grid_hbm, r.no_solve };
    return copy_fields(out, n, f);
}
// host-only test view: the plan of a ragged call (hs_ragged_plan, which the launches ask too)
int xpg_test_has_solution_batch_ragged_plan(const void * vc, int vc_rows, int cols, int nb, const int32_t * leq_rows, const int32_t * eq_rows,
                                            int num_cus, int32_t * out_route, long long * out, int n)
{
    if (!vc || !out || n < 0 || cols < 2 || vc_rows != cols - 1 || nb <= 0 || !leq_rows || !eq_rows || num_cus <= 0) return XPG_ERR_SHAPE;
    for (int b = 0; b < nb; b++) if (leq_rows[b] < 0 || eq_rows[b] < 0) return XPG_ERR_SHAPE;
    const VcView v = vc_view<R32>(vc, vc_rows, cols);
    const HsRaggedPlan p = hs_ragged_plan<R32>(v.pattern, v.nfree, nb, leq_rows, eq_rows, cols, num_cus);
    if (out_route) std::copy(p.route.begin(), p.route.end(), out_route);
    const HsRaggedLaunch & a = p.at[HS_ROUTE_LDS]; const HsRaggedLaunch & h = p.at[HS_ROUTE_HBM];
    const long long f[12] = { a.count, (long long)a.lds, a.threads, (long long)a.slot, a.grid,
                              h.count, (long long)h.lds, (long long)h.slot, h.Rmax, h.ld, h.threads, h.grid };
    return copy_fields(out, n, f);
}
// ---- Lineq::has_solution with is_int_sol = 1 for a batch: the objective, both MIP walks and the verdict on the device, one
// ---- synchronisation (has_solution_int.hip.h) ----
int xpg_has_solution_int_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows,
                                     const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_unique_sol, int32_t * out_has,
                                     int32_t * out_status)
{
    XPG_BIND(ctx);
    return has_solution_int_batch<R32>(ctx, nb, (const R32 *)leq, leq_rows, (const R32 *)eq, eq_rows, (const R32 *)vc, vc_rows, cols, rhs_idx,
                                       is_unique_sol != 0, out_has, out_status, [&](int32_t * has, int32_t * st) {   // the parent's composition
        return xpg_has_solution_batch_rat32(ctx, nb, leq, leq_rows, eq, eq_rows, vc, vc_rows, cols, rhs_idx, 1, is_unique_sol, 0xFFFFFFFFu, has, st);
    });
}
// the same for systems of mixed shapes under one vc: the shape classes on the host, each answered by the uniform call
int xpg_has_solution_int_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets,
                                            const xpg_rat32 * eq, const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc,
                                            int vc_rows, int cols, int rhs_idx, int is_unique_sol, int32_t * out_has, int32_t * out_status)
{
    XPG_BIND(ctx);
    HsIntRoute sum = {0, 0, 0, 0, 0, 0};
    const int rc = has_solution_ragged_int(ctx, nb, (const R32 *)leq, leq_rows, leq_offsets, (const R32 *)eq, eq_rows, eq_offsets, (const R32 *)vc,
                                           vc_rows, cols, rhs_idx, out_has, out_status,
                                           [&](int lr, int er, int count, const R32 * l, const R32 * e, int32_t * has, int32_t * st) {
        const int r = xpg_has_solution_int_batch_rat32(ctx, count, (const xpg_rat32 *)l, lr, (const xpg_rat32 *)e, er, vc, vc_rows, cols, rhs_idx,
                                                       is_unique_sol, has, st);
        const HsIntRoute & one = hs_int_route();
        sum.lds += one.lds; sum.hbm += one.hbm; sum.host += one.host; sum.second += one.second;
        sum.grid = std::max(sum.grid, one.grid); sum.grid2 = std::max(sum.grid2, one.grid2);
        return r;
    });
    hs_int_route() = rc == 0 ? sum : HsIntRoute{0, 0, 0, 0, 0, 0};
    return rc;
}
// what the calling thread's last xpg_has_solution_int_batch_* call did (has_solution_int.hip.h HsIntRoute)
int xpg_has_solution_int_batch_last_route(long long * out, int n)
{
    if (!out || n < 0) return XPG_ERR_SHAPE;
    const HsIntRoute & r = hs_int_route();
    const long long f[6] = { r.lds, r.hbm, r.host, r.second, r.grid, r.grid2 };
    return copy_fields(out, n, f);
}
// host-only test view: the route rule of xpg_has_solution_int_batch_* and the sizes it decides by
int xpg_test_has_solution_int_plan(const void * vc, int vc_rows, int leq_rows, int eq_rows, int cols, int nb, int num_cus, long long * out, int n)
{
    if (!vc || !out || n < 0 || cols < 2 || vc_rows != cols - 1 || leq_rows <= 0 || eq_rows < 0 || nb <= 0 || num_cus <= 0) return XPG_ERR_SHAPE;
    const VcView v = vc_view<R32>(vc, vc_rows, cols);
    const HsIntPlan g = hs_int_plan<R32>(v.pattern, v.nfree, leq_rows, eq_rows, cols, nb, num_cus);
    const long long f[17] = { g.route, g.extra, g.rmax, (long long)g.lds[0], (long long)g.lds[1], g.threads[0], g.threads[1], g.grid[0], g.grid[1],
                              g.nhelp[0], g.nhelp[1], (long long)g.slot, g.ld[0], g.ld[1], (long long)g.ws_words, (long long)g.obj_word,
                              (long long)g.scratch };
    return copy_fields(out, n, f);
}
} // extern "C"
