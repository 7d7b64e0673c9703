// C ABI of libxpoly_amd.so (include/xpoly_amd.h): rational / integer row elimination (Lineq, rank / det / inv / null,
// hnf, gcd). One of the library's eight sources (build.py).
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "lineq_host.hip.h"
#include "ragged_host.hip.h"
#include "lineq_hull_host.hip.h"

using namespace xpg;

extern "C" {
// Lineq::reduce on systems of different shapes, in place (mats: the systems back to back, system b at cell
// offsets[b]); rhs_idx[b] (NULL: the last column of each).
int xpg_lineq_reduce_batch_ragged_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                        const long long * offsets, const int32_t * rhs_idx, int is_intersect,
                                        int32_t * out_rows, int32_t * out_ok)
{
    XPG_BIND(ctx);
    if (!ctx || nb < 0 || !mats || !rows || !cols || !offsets || !out_rows || !out_ok) return XPG_ERR_SHAPE;
    // a class is (rows, cols, rhs): split the shape classes by constant column on the fly through the key of `cols`
    std::vector<int32_t> key((size_t)nb);
    for (int b = 0; b < nb; b++) {
        const int r = rhs_idx ? rhs_idx[b] : cols[b] - 1;
        if (cols[b] < 2 || cols[b] > 32767 || r < 0 || r >= cols[b]) return XPG_ERR_SHAPE;
        key[(size_t)b] = cols[b] | (r << 16);
    }
    return run_ragged(ctx, nb, rows, key.data(), [&](xpg_ctx * c, const RaggedClass & g) {
        const int gc = g.cols & 0xFFFF, rhs = g.cols >> 16;
        const size_t per = (size_t)g.rows * gc, ng = g.idx.size();
        std::vector<R32> buf; std::vector<int32_t> kr(ng), ko(ng);
        ragged_gather(buf, (const R32 *)mats, offsets, g, per);
        const int r = lineq_reduce_batch(c, (int)ng, buf.data(), g.rows, gc, rhs, 1, is_intersect, kr.data(), ko.data());
        if (r) return r;
        for (size_t k = 0; k < ng; k++) {
            const int b = g.idx[k];
            memcpy((void *)((R32 *)mats + offsets[b]), (const void *)(buf.data() + k * per), per * 8);
            out_rows[b] = kr[k]; out_ok[b] = ko[k];
        }
        return 0;
    });
}
// Lineq::fme on systems of different shapes, eliminating variable u[b] of system b. Packed result: system b's
// rows (cols[b] wide) start at cell out_cell_offsets[b] of outs (out_cell_offsets[nb] = cells in all); outs may
// be NULL or too small (outs_cap_cells): XPG_ERR_SHAPE with out_rows / out_cell_offsets filled.
int xpg_lineq_fme_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                     const long long * offsets, const int32_t * rhs_idx, const int32_t * u, int darkshadow,
                                     xpg_rat32 * outs, long long outs_cap_cells, long long * out_cell_offsets,
                                     int32_t * out_rows, int32_t * out_ok)
{
    XPG_BIND(ctx);
    if (!ctx || nb < 0 || !mats || !rows || !cols || !offsets || !u || !out_cell_offsets || !out_rows || !out_ok) return XPG_ERR_SHAPE;
    std::vector<int32_t> key((size_t)nb);
    for (int b = 0; b < nb; b++) {
        const int r = rhs_idx ? rhs_idx[b] : cols[b] - 1;
        if (cols[b] < 2 || cols[b] > 255 || r < 1 || r >= cols[b] || u[b] < 0 || u[b] >= r) return XPG_ERR_SHAPE;
        key[(size_t)b] = cols[b] | (r << 8) | (u[b] << 16);           // a class shares shape, constant column and variable
    }
    std::vector<std::vector<R32> > res((size_t)nb);
    const int rc = run_ragged(ctx, nb, rows, key.data(), [&](xpg_ctx * c, const RaggedClass & g) {
        const int gc = g.cols & 0xFF, rhs = (g.cols >> 8) & 0xFF, uu = g.cols >> 16;
        const size_t per = (size_t)g.rows * gc, ng = g.idx.size();
        std::vector<R32> buf; std::vector<int32_t> ko(ng); std::vector<long long> off(ng + 1);
        ragged_gather(buf, (const R32 *)mats, offsets, g, per);
        const R32 * view = 0;
        const int r = lineq_fme_batch_packed(c, (int)ng, buf.data(), g.rows, gc, rhs, uu, darkshadow, 0, (R32 *)0, 0, &view, off.data(), ko.data(),
                                           true);                 // (copied out below: the caller's packed view stays)
        if (r) return r;
        for (size_t k = 0; k < ng; k++) {
            const int b = g.idx[k];
            out_rows[b] = (int32_t)(off[k + 1] - off[k]); out_ok[b] = ko[k];
            res[(size_t)b].assign(view + off[k] * gc, view + off[k + 1] * gc);
        }
        return 0;
    });
    if (rc) return rc;
    long long tot = 0;
    for (int b = 0; b < nb; b++) { out_cell_offsets[b] = tot; tot += (long long)res[(size_t)b].size(); }
    out_cell_offsets[nb] = tot;
    if (!outs || outs_cap_cells < tot) return outs ? XPG_ERR_SHAPE : 0;
    for (int b = 0; b < nb; b++)
        if (!res[(size_t)b].empty()) memcpy((void *)((R32 *)outs + out_cell_offsets[b]), (const void *)res[(size_t)b].data(), res[(size_t)b].size() * 8);
    return 0;
}

#ifdef XPG_STAMPS
// diagnostic builds only: reads and clears the phase tick sums of k_fme_batch
int xpg_lineq_debug(xpg_ctx * ctx, unsigned long long * out16)
{
    XPG_BIND(ctx);
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_lq_ticks), sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_lq_ticks), z, sizeof(z)) != hipSuccess) return XPG_ERR_HIP;
    return 0;
}
#endif
int xpg_lineq_move2var_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                   int first_sym, int last_sym)
{
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols < 2 || rhs_idx < 0 || first_sym <= rhs_idx || last_sym < first_sym ||
        last_sym >= cols)
        return XPG_ERR_SHAPE;                           // the reference's ASSERT (linsys.cpp:1185-1188)
    std::vector<R32> tmp((size_t)rows * cols);
    for (int b = 0; b < nb; b++) {
        R32 * m = (R32 *)mats + (size_t)b * rows * cols;
        move2var_one(m, tmp.data(), rows, cols, rhs_idx, first_sym, last_sym);
        memcpy(m, tmp.data(), sizeof(R32) * (size_t)rows * cols);
    }
    return 0;
}

// ---- rational row elimination ---------------------------------------------------------------
int xpg_lineq_reduce_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                 int is_intersect, int32_t * out_rows, int32_t * out_ok)
{
    XPG_BIND(ctx); return lineq_reduce_batch(ctx, nb, (R32 *)mats, rows, cols, rhs_idx, 1, is_intersect, out_rows, out_ok); }
int xpg_lineq_reduce_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                        int is_intersect, xpg_rat32 * outs, long long outs_cap_rows,
                                        const xpg_rat32 ** out_view, long long * row_offsets, int32_t * out_rows,
                                        int32_t * out_ok)
{
    XPG_BIND(ctx);
    return lineq_reduce_batch_packed(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, 1, is_intersect, (R32 *)outs, outs_cap_rows,
                                     (const R32 **)out_view, row_offsets, out_rows, out_ok);
}
int xpg_lineq_remove_iden_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols,
                                      int32_t * out_rows)
{
    XPG_BIND(ctx); return lineq_reduce_batch(ctx, nb, (R32 *)mats, rows, cols, 0, 0, 1, out_rows, 0); }
int xpg_lineq_fme_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                              int u, int darkshadow, xpg_rat32 * outs, int cap_rows, int32_t * out_rows,
                              int32_t * out_ok)
{
    XPG_BIND(ctx);
    return lineq_fme_batch(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, u, darkshadow, (R32 *)outs, cap_rows,
                           out_rows, out_ok);
}
int xpg_lineq_calc_bound_batch_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                     int cap_rows, xpg_rat32 * bounds, int32_t * out_rows, int32_t * out_ok)
{
    XPG_BIND(ctx); return lineq_calc_bound_batch(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, cap_rows, (R32 *)bounds, out_rows, out_ok); }
int xpg_lineq_calc_bound_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                            int cap_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                            long long * row_offsets, int32_t * out_ok)
{
    XPG_BIND(ctx);
    if (!row_offsets) return XPG_ERR_SHAPE;
    if (cap_rows <= 0) cap_rows = 4 * rows + 16;
    return lineq_calc_bound_batch(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, cap_rows, (R32 *)outs, (int32_t *)0, out_ok,
                                  row_offsets, outs_cap_rows, (const R32 **)out_view);
}
int xpg_lineq_reduce_batch_rat32_dev(xpg_ctx * ctx, int nb, xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                     int is_intersect, int32_t * d_out_rows, int32_t * d_out_ok)
{
    XPG_BIND(ctx); return lineq_reduce_batch_dev(ctx, nb, (R32 *)d_mats, rows, cols, rhs_idx, 1, is_intersect, d_out_rows, d_out_ok); }
int xpg_lineq_fme_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, int u,
                                     int darkshadow, int cap_rows, xpg_rat32 * outs, long long outs_cap_rows,
                                     const xpg_rat32 ** out_view, long long * row_offsets, int32_t * out_ok)
{
    XPG_BIND(ctx);
    return lineq_fme_batch_packed(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, u, darkshadow, cap_rows, (R32 *)outs,
                                  outs_cap_rows, (const R32 **)out_view, row_offsets, out_ok);
}
int xpg_lineq_fme_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                  int u, int darkshadow, xpg_rat32 * d_outs, int cap_rows, int32_t * d_out_rows,
                                  int32_t * d_out_ok)
{
    XPG_BIND(ctx); return lineq_fme_batch_dev(ctx, nb, (const R32 *)d_mats, rows, cols, rhs_idx, u, darkshadow, (R32 *)d_outs,
                                              cap_rows, d_out_rows, d_out_ok); }
// ---- projection: a list of variables out of every system in one launch (lineq_host.hip.h) ------------------------------------
int xpg_lineq_project_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                         const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                         xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                         long long * row_offsets, int32_t * out_ok, int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_chain_batch_packed(ctx, false, nb, (const R32 *)mats, rows, cols, rhs_idx, elim, n_elim, darkshadow, cap_rows, cap_out_rows,
                                      (R32 *)outs, outs_cap_rows, (const R32 **)out_view, row_offsets, out_ok, out_steps);
}
int xpg_lineq_project_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                      const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                      xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_steps)
{
    XPG_BIND(ctx);
    return lineq_chain_batch_dev(ctx, false, nb, (const R32 *)d_mats, rows, cols, rhs_idx, elim, n_elim, darkshadow, cap_rows, cap_out_rows,
                                   (R32 *)d_outs, d_out_rows, d_out_ok, d_out_steps);
}
// what the calling thread's last xpg_lineq_project_batch_* call did (lineq_host.hip.h: the table beside LineqRoute)
int xpg_lineq_project_last_route(long long * out, int n) { return route_out(ROUTE_PROJECT, out, n); }
// host-only test view: the plan of a projection call from its shape alone (lineq_host.hip.h project_plan), with the
// capacities it settles on behind the route's six figures
int xpg_test_lineq_project_plan(int nb, int rows, int cols, int cap_rows, int cap_out_rows, long long * out, int n)
{
    LineqPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE : plan_out(ROUTE_PROJECT, project_plan(nb, rows, cols, cap_rows, cap_out_rows, p), p, out, n);
}
// host-only test view: what the projection entry points answer to an elimination list before they look at anything else
// (lineq_host.hip.h project_check, the function they ask): 0, XPG_ERR_SHAPE or XPG_ERR_UNSUPPORTED
int xpg_test_lineq_project_check(int cols, int rhs_idx, const int32_t * elim, int n_elim) { return project_check(cols, rhs_idx, elim, n_elim); }
// ---- projection that keeps every level: loop-nest limits in one launch (lineq_host.hip.h) ------------------------------------
int xpg_lineq_levels_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx,
                                        const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                        xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                        long long * row_offsets, int32_t * out_ok, int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_chain_batch_packed(ctx, true, nb, (const R32 *)mats, rows, cols, rhs_idx, elim, n_elim, darkshadow, cap_rows, cap_out_rows,
                                     (R32 *)outs, outs_cap_rows, (const R32 **)out_view, row_offsets, out_ok, out_steps);
}
int xpg_lineq_levels_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx,
                                     const int32_t * elim, int n_elim, int darkshadow, int cap_rows, int cap_out_rows,
                                     xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_steps)
{
    XPG_BIND(ctx);
    return lineq_chain_batch_dev(ctx, true, nb, (const R32 *)d_mats, rows, cols, rhs_idx, elim, n_elim, darkshadow, cap_rows, cap_out_rows,
                                  (R32 *)d_outs, d_out_rows, d_out_ok, d_out_steps);
}
// what the calling thread's last xpg_lineq_levels_batch_* call did (lineq_host.hip.h: the table beside LineqRoute)
int xpg_lineq_levels_last_route(long long * out, int n) { return route_out(ROUTE_LEVELS, out, n); }
// host-only test view: the plan of a levels call from its shape alone (lineq_host.hip.h levels_plan), with the capacities it
// settles on behind the route's seven figures
int xpg_test_lineq_levels_plan(int nb, int rows, int cols, int n_elim, int cap_rows, int cap_out_rows, long long * out, int n)
{
    LineqPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE : plan_out(ROUTE_LEVELS, levels_plan(nb, rows, cols, n_elim, cap_rows, cap_out_rows, p), p, out, n);
}
// ---- limits of transformed loop nests: T^-1, A * T^-1 and every level in one launch (lineq_host.hip.h) ------------------------
int xpg_lineq_transform_levels_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * nests, int shared_nest, const xpg_rat32 * tmats,
                                                  int rows, int cols, int rhs_idx, int mode, int cap_rows, int cap_out_rows,
                                                  xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                                  long long * row_offsets, int32_t * out_ok, int32_t * out_steps, int32_t * out_kind,
                                                  xpg_rat32 * out_det, xpg_rat32 * out_mult)
{
    XPG_BIND(ctx);
    return lineq_transform_batch_packed(ctx, nb, (const R32 *)nests, shared_nest, (const R32 *)tmats, rows, cols, rhs_idx, mode, cap_rows,
                                        cap_out_rows, (R32 *)outs, outs_cap_rows, (const R32 **)out_view, row_offsets, out_ok, out_steps,
                                        out_kind, (R32 *)out_det, (R32 *)out_mult);
}
int xpg_lineq_transform_levels_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_nests, int shared_nest, const xpg_rat32 * d_tmats,
                                               int rows, int cols, int rhs_idx, int mode, int cap_rows, int cap_out_rows,
                                               xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_steps,
                                               int32_t * d_out_kind, xpg_rat32 * d_out_det, xpg_rat32 * d_out_mult)
{
    XPG_BIND(ctx);
    return lineq_transform_batch_dev(ctx, nb, (const R32 *)d_nests, shared_nest, (const R32 *)d_tmats, rows, cols, rhs_idx, mode, cap_rows,
                                     cap_out_rows, (R32 *)d_outs, d_out_rows, d_out_ok, d_out_steps, d_out_kind, (R32 *)d_out_det,
                                     (R32 *)d_out_mult);
}
// what the calling thread's last xpg_lineq_transform_levels_batch_* call did (lineq_host.hip.h: the table beside LineqRoute)
int xpg_lineq_transform_last_route(long long * out, int n) { return route_out(ROUTE_TRANSFORM, out, n); }
// host-only test view: the plan of a transformed-nest call from its shape alone (lineq_host.hip.h transform_plan), with the
// capacities it settles on and where the inverse's scratch lies behind the route's seven figures
int xpg_test_lineq_transform_plan(int nb, int rows, int cols, int rhs_idx, int cap_rows, int cap_out_rows, long long * out, int n)
{
    LineqPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE : plan_out(ROUTE_TRANSFORM, transform_plan(nb, rows, cols, rhs_idx, cap_rows, cap_out_rows, p), p, out, n);
}
// ---- projection / levels of systems of mixed shapes and lists in one launch (lineq_host.hip.h) --------------------------------
int xpg_lineq_project_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                         const long long * offsets, const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets,
                                         int darkshadow, int cap_rows, int cap_out_rows, xpg_rat32 * outs, long long outs_cap_cells,
                                         const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok,
                                         int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_chain_ragged_packed(ctx, nb, (const R32 *)mats, rows, cols, offsets, rhs_idx, elim, elim_offsets, false, darkshadow, cap_rows,
                                     cap_out_rows, (R32 *)outs, outs_cap_cells, (const R32 **)out_view, out_cell_offsets, out_rows, out_ok, out_steps);
}
int xpg_lineq_levels_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                        const long long * offsets, const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets,
                                        int darkshadow, int cap_rows, int cap_out_rows, xpg_rat32 * outs, long long outs_cap_cells,
                                        const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok,
                                        int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_chain_ragged_packed(ctx, nb, (const R32 *)mats, rows, cols, offsets, rhs_idx, elim, elim_offsets, true, darkshadow, cap_rows,
                                     cap_out_rows, (R32 *)outs, outs_cap_cells, (const R32 **)out_view, out_cell_offsets, out_rows, out_ok, out_steps);
}
// what the calling thread's last ragged projection / levels call did (lineq_host.hip.h: the table beside LineqRoute)
int xpg_lineq_ragged_last_route(long long * out, int n) { return route_out(ROUTE_RAGGED, out, n); }
// host-only test view: the plan of a ragged call from its shapes and lists alone (lineq_host.hip.h ragged_chain_plan, the
// function the launch asks -- the error codes are its own), with the envelope it settles on behind the route's seven figures
int xpg_test_lineq_ragged_plan(int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx, const int32_t * elim,
                               const int32_t * elim_offsets, int levels, int cap_rows, int cap_out_rows, long long * out, int n)
{
    LineqPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE
                         : plan_out(ROUTE_RAGGED, ragged_chain_plan(nb, rows, cols, rhs_idx, elim, elim_offsets, levels != 0, cap_rows, cap_out_rows, p), p, out, n);
}
// ---- calcBound fused: the bounds of every variable of every system in one launch (lineq_host.hip.h) ---------------------------
int xpg_lineq_bounds_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, int cap_rows,
                                        int cap_out_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                        long long * row_offsets, int32_t * out_ok, int32_t * out_chain, int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_bounds_batch_packed(ctx, nb, (const R32 *)mats, rows, cols, rhs_idx, cap_rows, cap_out_rows, (R32 *)outs, outs_cap_rows,
                                     (const R32 **)out_view, row_offsets, out_ok, out_chain, out_steps);
}
int xpg_lineq_bounds_batch_rat32_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int rhs_idx, int cap_rows,
                                     int cap_out_rows, xpg_rat32 * d_outs, int32_t * d_out_rows, int32_t * d_out_ok, int32_t * d_out_chain,
                                     int32_t * d_out_steps)
{
    XPG_BIND(ctx);
    return lineq_bounds_batch_dev(ctx, nb, (const R32 *)d_mats, rows, cols, rhs_idx, cap_rows, cap_out_rows, (R32 *)d_outs, d_out_rows,
                                  d_out_ok, d_out_chain, d_out_steps);
}
// what the calling thread's last xpg_lineq_bounds_batch_* call did (lineq_host.hip.h: the table beside LineqRoute)
int xpg_lineq_bounds_last_route(long long * out, int n) { return route_out(ROUTE_BOUNDS, out, n); }
// host-only test view: the plan of a fused calcBound call from its shape alone (lineq_host.hip.h bounds_plan), with the
// capacities it settles on behind the route's seven figures
int xpg_test_lineq_bounds_plan(int nb, int rows, int cols, int rhs_idx, int cap_rows, int cap_out_rows, long long * out, int n)
{
    LineqPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE : plan_out(ROUTE_BOUNDS, bounds_plan(nb, rows, cols, rhs_idx, cap_rows, cap_out_rows, p), p, out, n);
}
// ---- calcBound fused for systems of mixed shapes in one launch (lineq_host.hip.h) ---------------------------------------------
int xpg_lineq_bounds_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                                        const long long * offsets, const int32_t * rhs_idx, int cap_rows, int cap_out_rows, xpg_rat32 * outs,
                                        long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                                        int32_t * out_ok, int32_t * out_chain, int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_bounds_ragged_packed(ctx, nb, (const R32 *)mats, rows, cols, offsets, rhs_idx, cap_rows, cap_out_rows, (R32 *)outs, outs_cap_cells,
                                      (const R32 **)out_view, out_cell_offsets, out_rows, out_ok, out_chain, out_steps);
}
// what the calling thread's last xpg_lineq_bounds_batch_ragged_rat32 call did (lineq_host.hip.h: the table beside LineqRoute)
int xpg_lineq_bounds_ragged_last_route(long long * out, int n) { return route_out(ROUTE_BOUNDS_RAGGED, out, n); }
// host-only test view: the plan of a ragged calcBound call from its shapes alone (lineq_host.hip.h bounds_ragged_plan, the
// function the launch asks -- the error codes are its own), with the envelope it settles on behind the route's eight figures
int xpg_test_lineq_bounds_ragged_plan(int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx, int cap_rows,
                                      int cap_out_rows, long long * out, int n)
{
    LineqPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE : plan_out(ROUTE_BOUNDS_RAGGED, bounds_ragged_plan(nb, rows, cols, rhs_idx, cap_rows, cap_out_rows, p), p, out, n);
}
// ---- hulls of lists of polyhedra: a producer launch, then ONE reduce per group (lineq_hull_host.hip.h) --------------------------
int xpg_lineq_hull_batch_ragged_rat32(xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats,
                                      const int32_t * rows, const int32_t * cols, const long long * offsets, const int32_t * rhs_idx,
                                      int is_intersect, int cap_rows, int cap_out_rows, int cap_hull_rows, xpg_rat32 * outs,
                                      long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                                      int32_t * out_ok, int32_t * out_member, int32_t * out_chain, int32_t * out_steps)
{
    XPG_BIND(ctx);
    return lineq_hull_ragged_packed(ctx, n_groups, group_offsets, n_members, (const R32 *)mats, rows, cols, offsets, rhs_idx, (const int32_t *)0,
                                    (const int32_t *)0, 0, is_intersect, cap_rows, cap_out_rows, cap_hull_rows, (R32 *)outs, outs_cap_cells,
                                    (const R32 **)out_view, out_cell_offsets, out_rows, out_ok, out_member, out_chain, out_steps);
}
int xpg_lineq_project_union_batch_ragged_rat32(xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats,
                                               const int32_t * rows, const int32_t * cols, const long long * offsets, const int32_t * rhs_idx,
                                               const int32_t * elim, const int32_t * elim_offsets, int darkshadow, int is_intersect,
                                               int cap_rows, int cap_out_rows, int cap_hull_rows, xpg_rat32 * outs, long long outs_cap_cells,
                                               const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok,
                                               int32_t * out_member, int32_t * out_chain, int32_t * out_steps)
{
    XPG_BIND(ctx);
    if (out_view) *out_view = 0;
    if (!elim_offsets && (n_groups != 0 || n_members != 0)) { route_clear(ROUTE_HULL); return XPG_ERR_SHAPE; }
    return lineq_hull_ragged_packed(ctx, n_groups, group_offsets, n_members, (const R32 *)mats, rows, cols, offsets, rhs_idx, elim, elim_offsets,
                                    darkshadow, is_intersect, cap_rows, cap_out_rows, cap_hull_rows, (R32 *)outs, outs_cap_cells,
                                    (const R32 **)out_view, out_cell_offsets, out_rows, out_ok, out_member, out_chain, out_steps);
}
// what the calling thread's last hull / projected-union call did (lineq_host.hip.h: the table beside LineqRoute); one record
// serves both
int xpg_lineq_hull_last_route(long long * out, int n) { return route_out(ROUTE_HULL, out, n); }
int xpg_lineq_project_union_last_route(long long * out, int n) { return route_out(ROUTE_HULL, out, n); }
// host-only test view: the plan of a hull call (elim_offsets NULL) or of a projected union from the shapes alone
// (lineq_hull_host.hip.h hull_plan, the function the launch asks -- the error codes are its own): the route's first nine
// figures, then the capacities, the rows of the LDS matrix area and the envelope's columns; homes / gcaps [n_groups] (may be NULL)
int xpg_test_lineq_hull_plan(int n_groups, const int32_t * group_offsets, int n_members, const int32_t * rows, const int32_t * cols,
                             const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, int cap_rows, int cap_out_rows,
                             int cap_hull_rows, long long * out, int n, int32_t * homes, int32_t * gcaps)
{
    HullPlan p;
    return !out || n < 0 ? XPG_ERR_SHAPE
                         : hull_plan_out(hull_plan(n_groups, group_offsets, n_members, rows, cols, rhs_idx, elim, elim_offsets, cap_rows, cap_out_rows,
                                                   cap_hull_rows, p, homes, gcaps), p, out, n);
}
int xpg_rat_rank_batch_dev(xpg_ctx * ctx, int nb, const xpg_rat32 * d_mats, int rows, int cols, int32_t * d_out_rank)
{
    XPG_BIND(ctx); return rat_rank_batch_dev(ctx, nb, (const R32 *)d_mats, rows, cols, d_out_rank); }
int xpg_rat_rank_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int32_t * out_rank)
{
    XPG_BIND(ctx); return out_rank ? gauss_batch(ctx, nb, (const R32 *)mats, rows, cols, 0, out_rank, 0, 0) : XPG_ERR_SHAPE; }
int xpg_rat_det_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int n, xpg_rat32 * out_det)
{
    XPG_BIND(ctx); return out_det ? gauss_batch(ctx, nb, (const R32 *)mats, n, n, 1, 0, (R32 *)out_det, 0) : XPG_ERR_SHAPE; }
int xpg_rat_inv_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int n, xpg_rat32 * out_inv, int32_t * out_ok)
{
    XPG_BIND(ctx); return (out_inv && out_ok) ? gauss_batch(ctx, nb, (const R32 *)mats, n, n, 2, out_ok, 0, (R32 *)out_inv) : XPG_ERR_SHAPE; }
int xpg_rat_rank_basis_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int is_unitarize,
                             int32_t * out_rank, xpg_rat32 * basis, int32_t * basis_rows)
{
    XPG_BIND(ctx);
    if (!out_rank || !basis || !basis_rows) return XPG_ERR_SHAPE;
    const int st = gauss_batch(ctx, nb, (const R32 *)mats, rows, cols, 3, out_rank, 0, (R32 *)basis, is_unitarize ? 1 : 0);
    if (st != 0) return st;
    for (int b = 0; b < nb; b++) basis_rows[b] = (!is_unitarize && out_rank[b] < rows) ? out_rank[b] : rows;
    return 0;
}
int xpg_rat_null_batch(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, xpg_rat32 * ns)
{
    XPG_BIND(ctx); return ns ? gauss_batch(ctx, nb, (const R32 *)mats, rows, cols, 4, 0, 0, (R32 *)ns) : XPG_ERR_SHAPE; }
int xpg_int_hnf_batch(xpg_ctx * ctx, int nb, const int32_t * mats, int rows, int cols, int32_t * h, int32_t * u,
                      int32_t * status)
{
    XPG_BIND(ctx); return int_hnf_batch(ctx, nb, mats, rows, cols, h, u, status); }
int xpg_int_gcd_batch(xpg_ctx * ctx, int nb, int32_t * mats, int rows, int cols)
{
    XPG_BIND(ctx); return int_gcd_batch(ctx, nb, mats, rows, cols); }

} // extern "C"
