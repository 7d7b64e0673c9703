// Lineq::has_solution with is_int_sol = true (src/com/linsys.cpp:830-906; the form DepPoly::is_empty asks, src/eng/poly.cpp:571)
// for a batch of systems of one shape in ONE call that synchronises once (xpg_has_solution_int_batch_*): the leq / eq arrays and
// the free-variable list go up once, the feasibility objective is built on the device, both MIP walks -- maxm, then minm where
// that left the question open -- and the verdict run there, and only `has` and the status pairs come down. ONE route rule
// (hs_int_plan) on the shape alone:
//   LDS   a sign-pattern vc whose node LPs fit the LDS walk in both directions (mip_device_fits): k_mip_tree exactly as it is,
//         twice, in the manner of dep_is_empty_batch (mip_front.hip.h) -- pass 0 on all systems, k_hs_int_update between the
//         passes, pass 1 under the `active` marks it sets; no host step between them
//   HBM   a sign pattern past that with both directions on mip_hbm_plan's HBM route: k_has_solution_int_hbm below, one workgroup
//         per system from the objective to the verdict, slot, LDS and workspace sized for the larger direction
//   HOST  anything else: has_solution_batch_int's composition (has_solution_batch.hip.h) unchanged
// Per system the verdict and the status pair are bit for bit those of xpg_has_solution_batch_rat32(is_int_sol = 1): the walks
// are the same code on the same objective, and has_solution's rules are stated once (six_host.hip.h hs_verdict, hs_store).
#pragma once
#include "has_solution_batch.hip.h"
#include "mip_tree_hbm.hip.h"

namespace xpg {

// What the calling thread's last xpg_has_solution_int_batch_* call did (xpg_has_solution_int_batch_last_route): systems on the
// LDS walk / the device-memory kernel / the host composition, systems whose second walk ran, the grid of pass 0 (or of the one
// device-memory launch) and of pass 1. A ragged call sums the counts over its classes and keeps the largest grids.
struct HsIntRoute { long long lds, hbm, host, second, grid, grid2; };
inline HsIntRoute & hs_int_route() { static thread_local HsIntRoute r = {0, 0, 0, 0, 0, 0}; return r; }

enum { HS_INT_ROUTE_LDS = 0, HS_INT_ROUTE_HBM = 1, HS_INT_ROUTE_HOST = 2 };
// What k_has_solution_int_hbm holds in static LDS: k_mip_tree_hbm's figure, array by array (the solver's reduction scratch,
// mip_build_node's sh_left and sh_nf, the walk's sh_ctl and the node's objective scratch). Held against the code object's
// before the launch (hbm_static_lds_check).
enum { HS_INT_HBM_LDS_STATIC = MIP_HBM_LDS_STATIC };

// THE route rule (the launches and xpg_test_has_solution_int_plan both ask it) for nb systems of one shape under a vc that is a
// sign pattern with `extra` free variables, or is not (pattern = false). The shape alone decides: XPG_MIP_DEVICE is not read
// here, as mip_batch_vc_hbm does not read it. [0]: maxm, [1]: minm.
struct HsIntPlan {
    int route, extra, rmax;
    size_t lds[2];          // LDS route: mip_geom's bytes per pass; HBM route: both hold the larger hbm_side_bytes
    int threads[2], grid[2];    // HBM route: one launch, [1] = [0]
    int nhelp[2];           // LDS route: helper workgroups behind the walkers of a pass (mip_batch_device's rule)
    size_t slot;            // HBM route: bytes of one workgroup's tableau slot, the larger direction's
    int ld[2];              // HBM route: each direction's own hbm_ld(R, V)
    size_t ws_words;        // one workgroup's workspace in 8-byte words: mip_ws_words, and on the HBM route the objective behind it
    size_t obj_word;        // HBM route: where the objective starts in the workspace
    size_t scratch;         // LDS route: workspaces of the larger grid, helpers included; HBM route: grid x (slot + workspace)
};
template <class S> inline HsIntPlan hs_int_plan(bool pattern, int extra, int leq_rows, int eq_rows, int cols, int nb, int num_cus)
{
    const MipHbmPlan a = mip_hbm_plan<S>(pattern, leq_rows, eq_rows, cols, false, true, extra, nb, num_cus);
    const MipHbmPlan b = mip_hbm_plan<S>(pattern, leq_rows, eq_rows, cols, false, false, extra, nb, num_cus);
    HsIntPlan g;
    g.extra = a.extra; g.rmax = a.R;
    g.lds[0] = a.lds; g.lds[1] = b.lds; g.threads[0] = a.threads; g.threads[1] = b.threads; g.grid[0] = a.grid; g.grid[1] = b.grid;
    g.nhelp[0] = g.nhelp[1] = 0;
    g.slot = 0; g.ld[0] = a.ld; g.ld[1] = b.ld; g.ws_words = a.ws_words; g.obj_word = 0; g.scratch = 0;
    if (a.route == MIP_HBM_ROUTE_LDS && b.route == MIP_HBM_ROUTE_LDS) {      // (mip_device_fits asks both directions: never one alone)
        g.route = HS_INT_ROUTE_LDS;
        int most = 0;
        for (int p = 0; p < 2; p++) {
            g.nhelp[p] = eq_rows == 0 && g.grid[p] == nb && nb <= 8 * num_cus ? num_cus : 0;
            if (g.grid[p] + g.nhelp[p] > most) most = g.grid[p] + g.nhelp[p];
        }
        g.scratch = (size_t)most * g.ws_words * 8;
        return g;
    }
    if (a.route != MIP_HBM_ROUTE_HBM || b.route != MIP_HBM_ROUTE_HBM) {
        g.route = HS_INT_ROUTE_HOST; g.grid[0] = g.grid[1] = 0;
        return g;
    }
    g.route = HS_INT_ROUTE_HBM;
    g.lds[0] = g.lds[1] = a.lds > b.lds ? a.lds : b.lds;
    g.slot = a.slot > b.slot ? a.slot : b.slot;
    g.obj_word = a.ws_words;                                     // (mip_ws_words is even: the objective starts on 16 bytes)
    g.ws_words = a.ws_words + (((size_t)cols + 1) & ~(size_t)1);
    g.threads[0] = g.threads[1] = MIP_HBM_THREADS;
    const size_t each = g.slot + g.ws_words * 8;
    g.grid[0] = g.grid[1] = (int)hbm_grid(num_cus, MIP_HBM_THREADS, MIP_HBM_WAVES_PER_CU, g.lds[0] + HS_INT_HBM_LDS_STATIC, each,
                                          BATCH_HBM_SCRATCH_MAX, nb);
    g.scratch = (size_t)g.grid[0] * each;
    return g;
}

// feasibility_objective (six_host.hip.h) per system, a workgroup a system: hs_objective on the leq and eq cells as given.
template <class S> __global__ __launch_bounds__(64)
void k_hs_int_objective(int nb, const S * __restrict__ leq, int leq_rows, const S * __restrict__ eqs, int eq_rows, int cols, S * __restrict__ tgtf)
{
    for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x)
        hs_objective<S>(leq + (size_t)b * leq_rows * cols, leq_rows, eq_rows > 0 ? eqs + (size_t)b * eq_rows * cols : (const S *)0, eq_rows, cols,
                        tgtf + (size_t)b * cols);
}
// After walk `pass` (0: maxm over all systems, 1: minm over the marked ones): hs_verdict on the walk's status, the verdict and
// the status pair as hs_store lays them out, and the marks of the next pass -- a system stays open only where maxm's verdict
// is 0; a negative status is its verdict and closes it.
__global__ void k_hs_int_update(int nb, int pass, const int32_t * __restrict__ walk, int is_unique, int * __restrict__ active,
                                int32_t * __restrict__ out_has, int32_t * __restrict__ out_status)
{
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= nb || (pass > 0 && active[b] != 1)) return;
    const int st = walk[b], has = hs_verdict(st, is_unique != 0);
    out_has[b] = has;
    out_status[2 * (size_t)b + pass] = st;
    if (pass == 0) out_status[2 * (size_t)b + 1] = XPG_HS_NOT_RUN;
    active[b] = pass == 0 && has == 0 ? 1 : 0;
}

// The device-memory form: one workgroup per system, grid-stride over the batch, in the mould of k_mip_tree_hbm with a loop of
// its own over the same steps (MipTask::start, mip_build_node, mip_hbm_solve_node -- registers of its own --, nf_products,
// mip_feed), asked twice. Per system: the objective into tg, behind everything mip_ws_carve hands out, so that no walk writes
// it; maxm on tab[rmax][ld_max] under hbm_carve(rmax, n); where hs_verdict leaves the question open, minm on tab[n][ld_min]
// under hbm_carve(n, rmax) over the SAME slot, workspace and LDS block -- all three sized for the larger direction. The
// barrier at the top of a walk has every thread through with the layout, the workspace fields and the status of the walk (or
// the system) before, so the start that follows may rewrite forks, spec_ctl, ctl, frame 0 and kept_v[0]; every other field is
// written before it is read (mip_build_node rebuilds the node, mip_feed sets a frame when it pushes it). A system that ends
// negative stops there: its status is its verdict, the next system starts from the same barrier.
template <class S> __global__ __launch_bounds__(256, 4)
void k_has_solution_int_hbm(int nb, const S * __restrict__ leq_all, int leq_rows, const S * __restrict__ eq_all, int eq_rows, int cols, int is_unique,
                            int rmax, int depth, unsigned long long * ws_all, size_t ws_words, size_t obj_word, unsigned long long * slots,
                            unsigned long long slot_cells, int ld_max, int ld_min, unsigned lds_bytes, const int * __restrict__ free_var, int extra,
                            int32_t * __restrict__ out_has, int32_t * __restrict__ out_status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int sh_ctl[2];
    __shared__ unsigned long long sh_v;                      // the node's own objective: recomputed by mip_feed
    const int n = cols - 1 + extra;                          // variables of a node LP
    // the launch's sizes against what this shape needs in either direction: a plan that was made for another shape ends every
    // system unanswered instead of writing past a slot, a workspace or the LDS block
    if (rmax <= 0 || extra < 0 || eq_rows + cols + 1 > MIP_EQ_MAX || mip_ws_words(rmax, cols, depth, extra) > obj_word ||
        obj_word + (size_t)cols > ws_words || (int)hbm_ld(rmax, n) > ld_max || (int)hbm_ld(n, rmax) > ld_min ||
        (size_t)rmax * ld_max > (size_t)slot_cells || (size_t)n * ld_min > (size_t)slot_cells ||
        hbm_side_bytes<S>(rmax, n) > (size_t)lds_bytes || hbm_side_bytes<S>(n, rmax) > (size_t)lds_bytes) {
        hs_end_all(nb, XPG_ERR_UNSUPPORTED, XPG_ERR_UNSUPPORTED, out_has, out_status);
        return;
    }
    S * const tab = (S *)(slots + (size_t)blockIdx.x * slot_cells);
    unsigned long long * const ws = ws_all + (size_t)blockIdx.x * ws_words;
    const MipWs<S> w = mip_ws_carve<S>(ws, rmax, cols, depth, extra);
    S * const tg = (S *)(ws + obj_word);
    for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
        const S * root = leq_all + (size_t)b * leq_rows * cols;
        const S * root_eq = eq_rows > 0 ? eq_all + (size_t)b * eq_rows * cols : (const S *)0;
        __syncthreads();                                     // the system before is through with tg
        hs_objective<S>(root, leq_rows, root_eq, eq_rows, cols, tg);
        int has = 0, st2[2] = {XPG_HS_NOT_RUN, XPG_HS_NOT_RUN};
        for (int pass = 0; pass < 2 && has == 0; pass++) {   // maxm, then minm of what that left open
            const int is_max = pass == 0 ? 1 : 0;
            const int R = is_max ? rmax : n, V = is_max ? n : rmax, ld = is_max ? ld_max : ld_min;
            __syncthreads();                                 // the walk before is through with the workspace, the slot and LDS
            // MipTask::start
            for (int j = threadIdx.x; j < cols; j += blockDim.x) w.forks[j] = 0;
            for (int j = threadIdx.x; j < 2 * depth; j += blockDim.x) w.spec_ctl[j] = 0;
            if (threadIdx.x == 0) {
                w.ctl[MC_HAVE_BEST] = 0; w.ctl[MC_TOP] = 0; w.ctl[MC_NODES] = 0; w.ctl[MC_FINAL] = 0; w.ctl[MC_SEQ] = 0;
                w.vals[0] = zero<S>(); w.vals[1] = zero<S>();
                int * f = w.frame;
                f[MF_STAGE] = 0; f[MF_COL] = 0; f[MF_LO] = 0; f[MF_HI] = 1; f[MF_KEPT] = 0;
                w.kept_v[0] = zero<S>();
            }
            __syncthreads();
            for (;;) {
                const int top = w.ctl[MC_TOP];
                __syncthreads();
                if (threadIdx.x == 0) w.ctl[MC_NODES] += 1;
                int st = mip_build_node<S>(w, tg, root, leq_rows, root_eq, eq_rows, cols, false, top, free_var, extra);
                if (st >= 0) {
                    const int rows = st;
                    st = mip_hbm_solve_node<S>((XPG_AS_LDS unsigned char *)lds, (XPG_AS_GLOBAL S *)tab, R, V, ld,
                                               (XPG_AS_GLOBAL const S *)(extra > 0 ? w.N : w.L),
                                               (XPG_AS_GLOBAL const S *)(extra > 0 ? w.wobj : tg), rows, cols + extra, is_max,
                                               (XPG_AS_GLOBAL S *)w.y, (XPG_AS_LDS S *)&sh_v);
                    if (extra > 0 && st == XPG_SIX_SUCC) nf_unsplit<S>(w.y, cols, free_var, extra);
                }
                if (st == XPG_SIX_SUCC) nf_products<S>(w.y, tg, cols, w.y, w.sol);    // (st is the same in every thread)
                if (threadIdx.x == 0) sh_ctl[0] = mip_feed<S>(w, cols, is_max != 0, false, st, (const uint8_t *)0) ? 1 : 0;
                __syncthreads();
                if (sh_ctl[0]) break;
            }
            st2[pass] = w.ctl[MC_FINAL];                     // (behind the loop's last barrier: the same in every thread)
            has = hs_verdict(st2[pass], is_unique != 0);
        }
        if (threadIdx.x == 0) hs_store(b, has, st2[0], st2[1], out_has, out_status);
    }
}

// The launches of a plan on route 0 or 1, enqueue only; every pointer is a device pointer, d_act [nb] ints, d_walk [nb] the
// walks' statuses, d_v [nb] cells and d_nodes [nb] ints what k_mip_tree writes beside them, d_q the speculation queue where a
// pass has helpers, d_ws the plan's workspaces. Sets the route's grids.
template <class S>
int hs_int_launch(xpg_ctx * ctx, HsIntPlan g, int nb, const S * leq, int leq_rows, const S * eqs, int eq_rows, int cols, bool is_unique,
                  const int * d_fv, S * d_tg, void * d_ws, int * d_act, int32_t * d_walk, S * d_v, int * d_nodes, void * d_q, int32_t * d_has,
                  int32_t * d_status)
{
    const int n0 = cols - 1, depth = n0 + 2;
    HsIntRoute & rt = hs_int_route();
    if (g.route == HS_INT_ROUTE_LDS) {
        hipLaunchKernelGGL((k_hs_int_objective<S>), dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(64), 0, ctx->stream, nb, leq, leq_rows, eqs, eq_rows,
                           cols, d_tg);
        XPG_HIP(ctx, hipGetLastError());
        for (int pass = 0; pass < 2; pass++) {
            MipGeom q;
            q.lds = g.lds[pass]; q.threads = g.threads[pass]; q.grid = g.grid[pass];
            if (g.nhelp[pass] > 0) XPG_HIP(ctx, hipMemsetAsync(d_q, 0, spq_bytes(), ctx->stream));
            // pass 1: under the marks pass 0's update set; no ragged rows, no solution wanted, no rational_indicator
            if (const int rc = mip_tree_launch<S>(ctx, q, g.nhelp[pass], nb, d_tg, leq, leq_rows, cols, pass == 0, false, g.rmax, depth, d_ws,
                                                  g.ws_words, d_walk, d_v, (void *)0, d_nodes, (const void *)0, pass == 0 ? (const void *)0 : d_act,
                                                  (const void *)0, eqs, eq_rows, g.nhelp[pass] > 0 ? d_q : (void *)0, d_fv, g.extra))
                return rc;
            hipLaunchKernelGGL(k_hs_int_update, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, ctx->stream, nb, pass, (const int32_t *)d_walk,
                               is_unique ? 1 : 0, d_act, d_has, d_status);
            XPG_HIP(ctx, hipGetLastError());
        }
        rt.grid = g.grid[0]; rt.grid2 = g.grid[1];
        return 0;
    }
    Scratch & slots = ctx->scratch[SCRATCH_BATCH_HBM];
    const size_t slots_bytes = (size_t)g.grid[0] * g.slot;
    if (const int rc = scratch_reserve(ctx, slots, slots_bytes, slots_bytes, "hipMalloc(has_solution_int_batch scratch)")) return rc;
    if (const int rc = hbm_static_lds_check(ctx, (const void *)k_has_solution_int_hbm<S>, HS_INT_HBM_LDS_STATIC,
                                            "k_has_solution_int_hbm: static LDS above HS_INT_HBM_LDS_STATIC"))
        return rc;
    XPG_HIP(ctx, lds_limit((const void *)k_has_solution_int_hbm<S>, ctx->device, g.lds[0]));
    hipLaunchKernelGGL((k_has_solution_int_hbm<S>), dim3((unsigned)g.grid[0]), dim3((unsigned)g.threads[0]), g.lds[0], ctx->stream, nb, leq, leq_rows,
                       eqs, eq_rows, cols, is_unique ? 1 : 0, g.rmax, depth, (unsigned long long *)d_ws, g.ws_words, g.obj_word,
                       (unsigned long long *)slots.buf, (unsigned long long)(g.slot / 8), g.ld[0], g.ld[1], (unsigned)g.lds[0], d_fv, g.extra, d_has,
                       d_status);
    XPG_HIP(ctx, hipGetLastError());
    rt.grid = g.grid[0]; rt.grid2 = 0;
    return 0;
}

// Host arrays; synchronises once; the caller's arrays are written at the very end. host(has, status): the parent's composition
// on the same arrays (route 2: has_solution_batch_int with its walks, functions of other parts of the library).
template <class S, class Host>
int has_solution_int_batch(xpg_ctx * ctx, int nb, const S * leq, int leq_rows, const S * eqs, int eq_rows, const S * vc, int vc_rows, int cols,
                           int rhs, bool is_unique, int32_t * out_has, int32_t * out_status, Host host)
{
    HsIntRoute & rt = hs_int_route();
    rt = HsIntRoute{0, 0, 0, 0, 0, 0};
    if (!hs_args_ok(ctx, nb, leq, leq_rows, eqs, eq_rows, vc, vc_rows, cols, rhs, out_has)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    if (leq_rows == 0) {
        const HsNoLeq e = hs_no_inequality(eq_rows);
        for (int b = 0; b < nb; b++) hs_store(b, e.has, e.status0, XPG_HS_NOT_RUN, out_has, out_status);
        return 0;
    }
    std::vector<int> fv;
    const bool pattern = vc_sign_pattern(vc, vc_rows, cols, fv);
    const int extra = pattern ? (int)fv.size() : 0;
    HsIntPlan g = hs_int_plan<S>(pattern, extra, leq_rows, eq_rows, cols, nb, ctx_cus(ctx));
    std::vector<int32_t> has((size_t)nb, 0), st((size_t)nb * 2, (int32_t)XPG_HS_NOT_RUN);   // staged: a call that fails leaves the caller's arrays untouched
    if (g.route == HS_INT_ROUTE_HOST) {
        if (const int rc = host(has.data(), st.data())) return rc;
        rt.host = nb;
    } else {
        const int grid_cap = XPG_INT_HOOK("XPG_HS_GRID");        // tests: the grid-stride path at small nb
        if (g.route == HS_INT_ROUTE_HBM && grid_cap > 0 && g.grid[0] > grid_cap) {
            g.grid[0] = g.grid[1] = grid_cap; g.scratch = (size_t)grid_cap * (g.slot + g.ws_words * 8);
        }
        const bool lds_route = g.route == HS_INT_ROUTE_LDS;
        const size_t bl = (size_t)nb * leq_rows * cols * 8, be = (size_t)nb * eq_rows * cols * 8;
        const size_t ws_bytes = lds_route ? g.scratch : (size_t)g.grid[0] * g.ws_words * 8;
        DevBuf dl, de, dfv, dtg, dws, dact, dwalk, dv, dn, dq, dhas, dst;
        XPG_TRY(dl.alloc(ctx, bl)); XPG_TRY(dws.alloc(ctx, ws_bytes));
        XPG_TRY(dhas.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dst.alloc(ctx, (size_t)nb * 8));
        XPG_TRY(hipMemcpyAsync(dl.p, leq, bl, hipMemcpyHostToDevice, ctx->stream));
        if (eq_rows > 0) {
            XPG_TRY(de.alloc(ctx, be));
            XPG_TRY(hipMemcpyAsync(de.p, eqs, be, hipMemcpyHostToDevice, ctx->stream));
        }
        if (extra > 0) {
            XPG_TRY(dfv.alloc(ctx, (size_t)extra * 4));
            XPG_TRY(hipMemcpyAsync(dfv.p, fv.data(), (size_t)extra * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        if (lds_route) {
            XPG_TRY(dtg.alloc(ctx, (size_t)nb * cols * 8)); XPG_TRY(dact.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dwalk.alloc(ctx, (size_t)nb * 4));
            XPG_TRY(dv.alloc(ctx, (size_t)nb * 8)); XPG_TRY(dn.alloc(ctx, (size_t)nb * 4));
            if (g.nhelp[0] > 0 || g.nhelp[1] > 0) XPG_TRY(dq.alloc(ctx, spq_bytes()));
        }
        const int rc = hs_int_launch<S>(ctx, g, nb, (const S *)dl.p, leq_rows, (const S *)de.p, eq_rows, cols, is_unique, (const int *)dfv.p, (S *)dtg.p,
                                        dws.p, (int *)dact.p, (int32_t *)dwalk.p, (S *)dv.p, (int *)dn.p, dq.p, (int32_t *)dhas.p, (int32_t *)dst.p);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); rt = HsIntRoute{0, 0, 0, 0, 0, 0}; return rc; }
        XPG_TRY(hipMemcpyAsync(has.data(), dhas.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipMemcpyAsync(st.data(), dst.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        (lds_route ? rt.lds : rt.hbm) = nb;
    }
    for (int b = 0; b < nb; b++) {
        hs_store(b, has[(size_t)b], st[2 * (size_t)b], st[2 * (size_t)b + 1], out_has, out_status);
        rt.second += st[2 * (size_t)b + 1] != XPG_HS_NOT_RUN;
    }
    return 0;
}

} // namespace xpg
