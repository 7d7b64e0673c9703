// MIP trees whose node LPs do NOT fit 64 KB of LDS, walked on the device all the same (xpg_mip_batch_vc_hbm_*): the join of
// k_mip_tree (mip_kernels.hip.h: the whole depth-first walk of one tree in one workgroup, state in a workspace in device
// memory) and k_batch_hbm (batch_hbm.hip.h: the solve on a tableau in global memory). One workgroup of 256 threads owns one
// tree from the caller's arrays to the answer, grid-stride over the batch, and every step is code that exists already:
//   walk     MipWs / mip_ws_carve, MipTask::start's initialisation, mip_build_node (root equalities, 0-1 and integer
//            branching, free variables split by nf_form), nf_products by all threads, mip_feed by thread 0 -- k_mip_tree's
//            loop without its helper workgroups, ragged rows, active marks and time slices.
//   solve    sm_solve_lp<S, true> on the node mip_build_node left in the workspace (raw solution into w.y), nf_unsplit after
//            it with free variables: the tableau tab[R][ld] lies in the WORKGROUP's slot in global memory (maximising R =
//            rmax, V = cols - 1 + extra, minimising the two swap; ld and the 256-byte slot alignment by hbm_ld and
//            hbm_slot_bytes), the side arrays in LDS under hbm_carve, carved for the largest node of the deepest path.
// A workgroup reads and writes its own slot and its own workspace alone: __syncthreads() is the only ordering. A slot is
// rewritten by every node (sm_build writes every live cell before anything reads it) and the workspace fields
// MipTask::start sets by every tree, so a workgroup takes tree after tree. Status, optimum, solution and node count are bit
// for bit those of k_mip_tree where that accepts the shape, and of the host controller (run_mip_tasks) everywhere.
#pragma once
#include "mip_host.hip.h"
#include "batch_hbm.hip.h"

namespace xpg {

// Which route the trees of the calling thread's last xpg_mip_batch_vc_hbm_* call took (xpg_mip_hbm_last_route).
struct MipHbmRoute { long long lds, hbm, host, free_vars, grid; };
inline MipHbmRoute & mip_hbm_route() { static thread_local MipHbmRoute r = {0, 0, 0, 0, 0}; return r; }

enum { MIP_HBM_ROUTE_LDS = 0, MIP_HBM_ROUTE_HBM = 1, MIP_HBM_ROUTE_HOST = 2 };
// What k_mip_tree_hbm holds in LDS besides hbm_carve's arrays (the code object's group_segment_fixed_size): the reduction
// scratch of the solver's inlined helpers (256 bytes), mip_build_node's sh_left[MIP_EQ_MAX] and sh_nf[4] (528), the walk's
// sh_ctl[2] and the node's objective scratch (8 + 8). The launch holds the figure against the code object's
// (hbm_static_lds_check).
enum { MIP_HBM_LDS_STATIC = 256 + 2 * MIP_EQ_MAX + 16 + 16 };
enum { MIP_HBM_THREADS = BATCH_HBM_THREADS, MIP_HBM_WAVES_PER_CU = BATCH_HBM_WAVES_PER_CU };

// THE route rule (the launch and xpg_test_mip_hbm_plan both ask it) for nb trees of one shape under a vc that is a sign
// pattern with `extra` free variables, or is not (pattern = false):
//   LDS    the pattern holds and mip_device_fits: k_mip_tree exactly as xpg_mip_batch_vc_* launches it (mip_batch_device)
//   HBM    the pattern holds past that: k_mip_tree_hbm, if the node's equality list fits (eq_rows + n + 2 <= MIP_EQ_MAX), the
//          side arrays of the largest node fit 160 KB beside the kernel's static LDS and one slot fits the scratch cap
//   HOST   anything else: the host controller under the caller's vc (mip_batch_vc_host)
struct MipHbmPlan {
    int route, extra, R, V;
    size_t lds;             // LDS route: the largest node's small_lds_bytes; else hbm_side_bytes(R, V)
    size_t slot;            // bytes of one workgroup's tableau slot (0 on the LDS route)
    int ld;
    size_t ws_words;        // one workgroup's workspace in 8-byte words (mip_ws_words)
    int threads, grid;
    size_t scratch;         // grid x (slot + workspace)
};
template <class S>
inline MipHbmPlan mip_hbm_plan(bool pattern, int leq_rows, int eq_rows, int cols, bool is_bin, bool is_max, int extra, int nb, int num_cus)
{
    const int n0 = cols - 1, n = n0 + extra, rmax = mip_rmax(leq_rows, eq_rows, n0, is_bin), depth = n0 + 2;
    MipHbmPlan g;
    g.extra = pattern ? extra : 0;
    g.R = is_max ? rmax : n; g.V = is_max ? n : rmax;
    g.ws_words = mip_ws_words(rmax, cols, depth, extra);
    if (pattern && mip_device_fits<S>(leq_rows, cols, is_bin, eq_rows, extra)) {
        const MipGeom q = mip_geom_cus<S>(num_cus, nb, rmax, n, is_max);
        g.route = MIP_HBM_ROUTE_LDS; g.lds = q.lds; g.slot = 0; g.ld = g.V + g.R + 2; g.threads = q.threads; g.grid = q.grid;
        g.scratch = (size_t)q.grid * g.ws_words * 8;
        return g;
    }
    const size_t ld = hbm_ld(g.R, g.V);
    g.lds = rmax > 0 ? hbm_side_bytes<S>(g.R, g.V) : 0;
    g.ld = (int)ld;
    g.slot = hbm_slot_bytes(g.R > 0 ? g.R : 0, ld);
    g.threads = MIP_HBM_THREADS;
    if (!pattern || rmax <= 0 || extra < 0 || extra > n0 || eq_rows + n0 + 2 > MIP_EQ_MAX ||
        g.lds + MIP_HBM_LDS_STATIC > (size_t)160 * 1024 || g.slot > BATCH_HBM_SCRATCH_MAX) {
        g.route = MIP_HBM_ROUTE_HOST; g.grid = 0; g.scratch = 0;
        return g;
    }
    g.route = MIP_HBM_ROUTE_HBM;
    const size_t each = g.slot + g.ws_words * 8;
    g.grid = (int)hbm_grid(num_cus, g.threads, MIP_HBM_WAVES_PER_CU, g.lds + MIP_HBM_LDS_STATIC, each, BATCH_HBM_SCRATCH_MAX, nb);
    g.scratch = (size_t)g.grid * each;
    return g;
}

// The node's LP as a function of its own, as six_vc_hbm_solve is (six_batch_vc_hbm.hip.h): its registers are allocated for
// the pivot loop alone instead of together with the walk around it. The LDS block and the objective scratch come in as
// address-space-3 pointers, the slot and the workspace's arrays as address-space-1 ones, so behind the call boundary the side
// arrays stay ds_* and the tableau global_* accesses; scalars by value, the status by value. (R, V): the largest node's, which
// the LDS block was sized for -- every node carves the same arrays, as k_mip_tree's one sm_carve does.
template <class S> __device__ __noinline__ int mip_hbm_solve_node(XPG_AS_LDS unsigned char * lds, XPG_AS_GLOBAL S * tab, int R, int V, int ld,
                                                                  XPG_AS_GLOBAL const S * node, XPG_AS_GLOBAL const S * obj, int rows, int ncols,
                                                                  int is_max, XPG_AS_GLOBAL S * y, XPG_AS_LDS S * v_scratch)
{
    Small<S> P;
    hbm_carve(P, (unsigned char *)lds, (S *)tab, R, V, ld);
    Source<S> src;
    src.leq = (const S *)node; src.tgtf = (const S *)obj; src.m = rows; src.cols = ncols; src.is_max = is_max;
    return sm_solve_lp<S, true>(P, src, 10000u, /*raw_sol=*/1, (S *)y, (S *)v_scratch);
}

// One workgroup per tree, grid-stride over the batch; arguments as k_mip_tree's (eq_all / eq_rows, allow, free_var / extra
// may be NULL / 0), slots: one tableau of slot_cells 8-byte cells per workgroup, ws_all: one workspace of ws_words per
// workgroup.
template <class S> __global__ __launch_bounds__(256, 4)
void k_mip_tree_hbm(int nb, const S * tgtf_all, const S * leq_all, int leq_rows, int cols, int is_max, int is_bin, int rmax,
                    int depth, unsigned long long * ws_all, size_t ws_words, unsigned long long * slots, unsigned long long slot_cells,
                    int ld, int32_t * out_status, S * out_v, S * out_sol, int * out_nodes, const uint8_t * allow, const S * eq_all,
                    int eq_rows, const int * free_var, int extra)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int sh_ctl[2];
    __shared__ unsigned long long sh_v;                      // the node's own objective: recomputed by mip_feed
    const int n = cols - 1 + extra;                          // variables of a node LP
    const int R = is_max ? rmax : n, V = is_max ? n : rmax;
    S * const tab = (S *)(slots + (size_t)blockIdx.x * slot_cells);
    const MipWs<S> w = mip_ws_carve<S>(ws_all + (size_t)blockIdx.x * ws_words, rmax, cols, depth, extra);
    for (int b = (int)blockIdx.x; b < nb; b += (int)gridDim.x) {
        const S * tgtf = tgtf_all + (size_t)b * cols;
        const S * root = leq_all + (size_t)b * leq_rows * cols;
        const S * root_eq = eq_rows > 0 ? eq_all + (size_t)b * eq_rows * cols : (const S *)0;
        __syncthreads();                                     // the tree before is through with the workspace, the slot and LDS
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
            int st = mip_build_node<S>(w, tgtf, root, leq_rows, root_eq, eq_rows, cols, is_bin != 0, top, free_var, extra);
            if (st >= 0) {
                const int rows = st;
                st = mip_hbm_solve_node<S>((XPG_AS_LDS unsigned char *)lds, (XPG_AS_GLOBAL S *)tab, R, V, ld,
                                           (XPG_AS_GLOBAL const S *)(extra > 0 ? w.N : w.L),
                                           (XPG_AS_GLOBAL const S *)(extra > 0 ? w.wobj : tgtf), rows, cols + extra, is_max,
                                           (XPG_AS_GLOBAL S *)w.y, (XPG_AS_LDS S *)&sh_v);
                if (extra > 0 && st == XPG_SIX_SUCC) nf_unsplit<S>(w.y, cols, free_var, extra);
            }
            // finish_host's products into y and the reduced solution, by all threads; their sum, in the reference's order,
            // stays with thread 0 (mip_feed)
            if (st == XPG_SIX_SUCC) nf_products<S>(w.y, tgtf, cols, w.y, w.sol);    // (st is the same in every thread)
            if (threadIdx.x == 0) sh_ctl[0] = mip_feed<S>(w, cols, is_max != 0, is_bin != 0, st, allow) ? 1 : 0;
            __syncthreads();
            if (sh_ctl[0]) break;
        }
        if (threadIdx.x == 0) {
            out_status[b] = w.ctl[MC_FINAL];
            out_v[b] = w.vals[0];
            out_nodes[b] = w.ctl[MC_NODES];
        }
        if (w.ctl[MC_FINAL] == XPG_IP_SUCC && out_sol)
            for (int j = threadIdx.x; j < cols; j += blockDim.x) out_sol[(size_t)b * cols + j] = w.sol[j];
    }
}

// mip_batch_device's counterpart for a plan on the HBM route: host arrays in and out through the same MipIo, one launch.
template <class S>
int mip_hbm_launch(xpg_ctx * ctx, const MipHbmPlan & g, int nb, bool is_max, bool is_bin, const S * tgtf, const S * leq, int leq_rows, int cols,
                   int32_t * out_status, S * out_v, S * out_sol, long long * out_nodes, const uint8_t * allow_rational, const S * eqs,
                   int eq_rows, const int * free_var, int extra)
{
    const int n0 = cols - 1, rmax = mip_rmax(leq_rows, eq_rows, n0, is_bin), depth = n0 + 2;
    const size_t slots_bytes = (size_t)g.grid * g.slot;
    Scratch & slots = ctx->scratch[SCRATCH_BATCH_HBM];
    if (const int rc = scratch_reserve(ctx, slots, slots_bytes, slots_bytes, "hipMalloc(mip_batch_vc_hbm scratch)")) return rc;
    MipIo io;
    if (const int rc = io.up(ctx, nb, tgtf, leq, leq_rows, eqs, eq_rows, cols, allow_rational, free_var, extra, out_sol,
                             (size_t)g.grid * g.ws_words * 8)) return rc;
    if (const int rc = hbm_static_lds_check(ctx, (const void *)k_mip_tree_hbm<S>, MIP_HBM_LDS_STATIC, "k_mip_tree_hbm: static LDS above MIP_HBM_LDS_STATIC"))
        return rc;
    XPG_TRY(lds_limit((const void *)k_mip_tree_hbm<S>, ctx->device, g.lds));
    hipLaunchKernelGGL((k_mip_tree_hbm<S>), dim3((unsigned)g.grid), dim3((unsigned)g.threads), g.lds, ctx->stream, nb, (const S *)io.dt.p,
                       (const S *)io.dl.p, leq_rows, cols, is_max ? 1 : 0, is_bin ? 1 : 0, rmax, depth, (unsigned long long *)io.dws.p, g.ws_words,
                       (unsigned long long *)slots.buf, (unsigned long long)(g.slot / 8), g.ld, (int32_t *)io.dst.p, (S *)io.dv.p,
                       out_sol ? (S *)io.dsol.p : (S *)0, (int *)io.dn.p, (const uint8_t *)io.dal.p, (const S *)io.de.p, eq_rows,
                       (const int *)io.dfv.p, extra);
    XPG_TRY(hipGetLastError());
    return io.down(ctx, nb, cols, out_status, out_v, out_sol, out_nodes);
}

// mip_batch_vc for node LPs of any size: the arguments and results of mip_batch_vc, the route by mip_hbm_plan. The rule is the
// shape's alone: XPG_MIP_DEVICE=0, which sends mip_batch_vc to the host controller for A/B runs, is NOT read here -- the host
// controller's side of an A/B is mip_batch_vc on the same arrays (tools/lab/probe_mip_hbm.py).
template <class S>
int mip_batch_vc_hbm(xpg_ctx * ctx, int kind, int nb, bool is_max, bool is_bin, const S * tgtf, const S * vc, const S * eqs, int eq_rows,
                     const S * leq, int leq_rows, int cols, const uint8_t * allow_rational, int32_t * out_status, S * out_v, S * out_sol,
                     long long * out_nodes)
{
    MipHbmRoute & rt = mip_hbm_route();
    rt = MipHbmRoute{0, 0, 0, 0, 0};
    if (!ctx || nb < 0 || !tgtf || !vc || eq_rows < 0 || leq_rows < 0 || (eq_rows == 0 && leq_rows == 0) || (eq_rows > 0 && !eqs) ||
        (leq_rows > 0 && !leq) || cols < 2 || !out_status || !out_v)
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    std::vector<int> fv;
    const bool pattern = vc_sign_pattern(vc, cols - 1, cols, fv);
    const int extra = pattern ? (int)fv.size() : 0;
    const MipHbmPlan g = mip_hbm_plan<S>(pattern, leq_rows, eq_rows, cols, is_bin, is_max, extra, nb, ctx_cus(ctx));
    if (g.route == MIP_HBM_ROUTE_LDS) {
        const int rc = mip_batch_device<S>(ctx, nb, is_max, is_bin, tgtf, leq, leq_rows, cols, out_status, out_v, out_sol, out_nodes,
                                           allow_rational, eqs, eq_rows, fv.data(), extra);
        if (rc != XPG_ERR_UNSUPPORTED) {
            if (rc == 0) { rt.lds = nb; rt.free_vars = extra; rt.grid = g.grid; }
            return rc;
        }
    }
    if (g.route == MIP_HBM_ROUTE_HBM) {
        const int rc = mip_hbm_launch<S>(ctx, g, nb, is_max, is_bin, tgtf, leq, leq_rows, cols, out_status, out_v, out_sol, out_nodes,
                                         allow_rational, eqs, eq_rows, fv.data(), extra);
        if (rc) return rc;
        rt.hbm = nb; rt.free_vars = extra; rt.grid = g.grid;
        MipRoute & mr = mip_route();
        mr.device_trees += nb;
        if (extra > mr.free_vars) mr.free_vars = extra;
        return 0;
    }
    const int rc = mip_batch_vc_host<S>(ctx, kind, nb, is_max, is_bin, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, allow_rational, out_status,
                                        out_v, out_sol, out_nodes);
    if (rc == 0) rt.host = nb;
    return rc;
}

} // namespace xpg
