// Batches of LPs WITH equalities and free variables whose normal form does NOT fit 64 KB of LDS (xpg_six_batch_vc_hbm_*):
// the join of k_six_batch_vc (six_batch_vc.hip.h: SIX::normalize and calcFinalSolution around the solve, on the device) and
// k_batch_hbm (batch_hbm.hip.h: the solve on a tableau in global memory). One workgroup owns one LP from the caller's arrays
// to the answer, grid-stride over the batch, and every step is code that exists already:
//   reshape  normalize_dev.hip.h's nf_* on plain pointers -- here L, E, rest and N all lie in the workgroup's slot in global
//            memory, so a substitution is O(rows x cols) L2 accesses instead of LDS ones (nf_fold_step reads the coefficient
//            column of a step while it writes the others and rewrites that column behind a barrier: nothing in it cares where
//            L lives). Where the reference's leading value (lpsol.h:1232) leaves the row the LP ends XPG_ERR_REF_UNDEFINED
//            alone and never meets the pivot loop.
//   solve    sm_solve_lp<S, true> on N, raw solution: hbm_carve for the rows THIS LP has (batches are ragged: an LP keeps
//            leq_rows + 2 nrest rows), the slot's ld kept.
//   finish   nf_unsplit, nf_products, the sum in column order on one thread -- k_six_batch_vc's ending.
// Slot (one per WORKGROUP, on a 256-byte line, every section on a 16-byte one):
//   fv | L [leq_rows x cols] | E [eq_rows x cols] | rest | N [(leq_rows + 2 eq_rows) x (n + 1)] | obj | y | v | tab [Rmax x ld]
// LDS: hbm_carve's side arrays for the largest (R, V) of the batch, and statically the solver's reduction scratch and the four
// ints nf_* take (SIX_VC_HBM_LDS_STATIC: the route rule counts both). A workgroup reads and writes its own slot alone:
// __syncthreads() is the only ordering. Status, optimum and solution are bit for bit those of k_six_batch_vc where that
// accepts the shape, and of the single-problem entry points everywhere.
#pragma once
#include "six_batch_vc.hip.h"
#include "batch_hbm.hip.h"

namespace xpg {

// Which route the LPs of the calling thread's last xpg_six_batch_vc_hbm_* call took (xpg_six_batch_vc_hbm_last_route).
struct SixVcHbmRoute { long long lds, hbm, fallback, free_vars, grid; };
inline SixVcHbmRoute & six_vc_hbm_route() { static thread_local SixVcHbmRoute r = {0, 0, 0, 0, 0}; return r; }

enum { SIX_VC_HBM_ROUTE_LDS = 0, SIX_VC_HBM_ROUTE_HBM = 1, SIX_VC_HBM_ROUTE_OTHER = 2 };
// What k_six_batch_vc_hbm holds in LDS besides hbm_carve's arrays (the code object's group_segment_fixed_size): the
// reduction scratch of the solver's inlined helpers, 256 bytes -- SMALL_LDS_STATIC's share without k_batch's sh_next --
// and hdr[4].
enum { SIX_VC_HBM_LDS_STATIC = 256 + 16 };
enum { SIX_VC_HBM_THREADS = BATCH_HBM_THREADS, SIX_VC_HBM_WAVES_PER_CU = BATCH_HBM_WAVES_PER_CU };

// The slot of one workgroup in 8-byte cells. nfree: the most free variables an LP of the launch can have (the host-array
// form has read vc; the _dev form sizes for every variable free), Rmax x ld: the tableau of the largest normal form.
struct SixVcHbmSlot { size_t fv, L, E, rest, N, obj, y, v, tab, cells; };
__host__ __device__ inline SixVcHbmSlot six_vc_hbm_slot(int leq_rows, int eq_rows, int cols, int nfree, int Rmax, int ld)
{
    const size_t n0 = (size_t)cols - 1, n = n0 + (size_t)nfree, rows_max = (size_t)leq_rows + 2 * (size_t)eq_rows;
    const auto even = [](size_t c) { return (c + 1) & ~(size_t)1; };
    SixVcHbmSlot s;
    size_t o = 0;
    s.fv = o; o += even((n0 + 1) / 2);
    s.L = o; o += even((size_t)leq_rows * cols);
    s.E = o; o += even((size_t)eq_rows * cols);
    s.rest = o; o += even(((size_t)eq_rows + 1) / 2);
    s.N = o; o += even(rows_max * (n + 1));
    s.obj = o; o += even(n + 1);
    s.y = o; o += even(n + 1);
    s.v = o; o += 2;
    s.tab = o; o += (size_t)Rmax * (size_t)ld;
    s.cells = (o + 31) & ~(size_t)31;        // slots start on 256-byte lines
    return s;
}

// THE route rule (the launch and xpg_test_six_batch_vc_hbm_plan both ask it). nfree >= 0: the caller has read vc (the
// host-array form; pattern says whether it is a sign pattern); nfree < 0: vc is known to the device alone and everything is
// sized for every variable free.
//   LDS    six_vc_plan(...).device: k_six_batch_vc exactly as xpg_six_batch_vc_* launches it
//   HBM    a sign pattern past 64 KB: k_six_batch_vc_hbm, if eq_rows <= SIX_VC_MAX_EQ, the side arrays of the largest normal
//          form fit 160 KB beside the kernel's static LDS and one slot fits the scratch cap
//   OTHER  the host-array form solves per problem (six_solve), the _dev form returns XPG_ERR_UNSUPPORTED before any launch
// Its device-memory half, which hs_plan (has_solution_batch.hip.h) decides by too: the grid (hbm_grid under SIX_VC_SCRATCH_MAX;
// the scratch is grid x slot), or 0, refused: not `allowed`, side arrays past 160 KB beside the static LDS, a slot past the cap.
inline int six_vc_hbm_grid(bool allowed, size_t lds, size_t slot, int nb, int num_cus)
{
    if (!allowed || lds + SIX_VC_HBM_LDS_STATIC > (size_t)160 * 1024 || slot > SIX_VC_SCRATCH_MAX) return 0;
    return (int)hbm_grid(num_cus, SIX_VC_HBM_THREADS, SIX_VC_HBM_WAVES_PER_CU, lds + SIX_VC_HBM_LDS_STATIC, slot, SIX_VC_SCRATCH_MAX, nb);
}
struct SixVcHbmPlan {
    int route, nfree, Rmax, Vmax;
    size_t lds;             // LDS route: the largest normal form's small_lds_bytes; else hbm_side_bytes(Rmax, Vmax)
    size_t slot;            // bytes of one workgroup's slot
    int ld, threads, grid;
    size_t scratch;         // grid x slot
};
template <class S>
inline SixVcHbmPlan six_vc_hbm_plan(bool pattern, int nfree, int leq_rows, int eq_rows, int cols, bool is_max, int nb, int num_cus)
{
    const int cap = nfree >= 0 ? nfree : cols - 1;
    const SixVcPlan p = six_vc_plan<S>(pattern, cap, leq_rows, eq_rows, cols, is_max);
    SixVcHbmPlan g;
    g.nfree = nfree >= 0 ? nfree : -1;
    g.Rmax = is_max ? p.rows_max : p.n; g.Vmax = is_max ? p.n : p.rows_max;
    if (p.device) {
        const SixVcGeom q = six_vc_geometry<S>(nfree, nb, leq_rows, eq_rows, cols, is_max);
        g.route = SIX_VC_HBM_ROUTE_LDS; g.lds = p.lds; g.slot = q.slot_cells * 8; g.ld = g.Vmax + g.Rmax + 2;
        g.threads = q.threads; g.grid = (int)q.grid; g.scratch = (size_t)q.grid * g.slot;
        return g;
    }
    const size_t ld = hbm_ld(g.Rmax, g.Vmax);
    g.lds = hbm_side_bytes<S>(g.Rmax, g.Vmax);
    g.ld = (int)ld;
    g.slot = six_vc_hbm_slot(leq_rows, eq_rows, cols, cap, g.Rmax, g.ld).cells * 8;
    g.threads = SIX_VC_HBM_THREADS;
    g.grid = six_vc_hbm_grid(pattern && eq_rows <= SIX_VC_MAX_EQ, g.lds, g.slot, nb, num_cus);
    g.route = g.grid > 0 ? SIX_VC_HBM_ROUTE_HBM : SIX_VC_HBM_ROUTE_OTHER;
    g.scratch = (size_t)g.grid * g.slot;
    return g;
}

// The solve as a function of its own, as k_batch keeps its specialised loop (batch_kernels.hip.h sm_fast_loop_32x97x256): its
// registers are allocated for the pivot loop alone instead of together with the staging and the reshaping around it (inlined,
// the kernel's 128 registers spilled 10 / 23 of them, fp64 / Rational). The LDS block comes in as an address-space-3 pointer,
// and the slot's arrays as address-space-1 ones, so
// behind the call boundary the side arrays stay ds_* and the tableau global_* accesses (through generic pointers both became flat_*);
// scalars by value, results by value.
struct SixVcHbmSolved { int status; unsigned pivots; };
template <class S> __device__ __noinline__ SixVcHbmSolved six_vc_hbm_solve(XPG_AS_LDS unsigned char * lds, XPG_AS_GLOBAL S * tab, int ld, XPG_AS_GLOBAL const S * N,
                                                                          XPG_AS_GLOBAL const S * obj, int rows, int n, int is_max, unsigned max_iter,
                                                                          XPG_AS_GLOBAL S * y, XPG_AS_GLOBAL S * vout)
{
    Small<S> P;
    hbm_carve(P, (unsigned char *)lds, (S *)tab, is_max ? rows : n, is_max ? n : rows, ld);
    Source<S> src;
    src.leq = (const S *)N; src.tgtf = (const S *)obj; src.m = rows; src.cols = n + 1; src.is_max = is_max;
    SixVcHbmSolved r;
    r.status = sm_solve_lp<S, true>(P, src, max_iter, /*raw_sol=*/1, (S *)y, (S *)vout);
    r.pivots = P.pivots;
    return r;
}

// One workgroup per LP, grid-stride over the batch. vc is read on the device as k_six_batch_vc reads it: every workgroup
// derives the free list once; a vc that is no sign pattern, or one with more free variables than the launch was sized for
// (nfree_cap), ends every LP XPG_ERR_UNSUPPORTED. The slot is reused from LP to LP: every cell of L, E, rest, N, obj and
// the tableau that an LP reads, that LP has written.
template <class S> __global__ __launch_bounds__(1024)
void k_six_batch_vc_hbm(int nb, const S * __restrict__ tgtf, const S * __restrict__ vc, const S * __restrict__ eqs, int eq_rows,
                        const S * __restrict__ leq, int leq_rows, int cols, int is_max, unsigned max_iter, int nfree_cap,
                        int Rmax, int ld, unsigned lds_bytes, unsigned long long * slots, unsigned long long slot_cells,
                        int32_t * __restrict__ out_status, S * __restrict__ out_v, S * __restrict__ out_sol,
                        uint32_t * __restrict__ out_pivots)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int hdr[4];                                       // [0]: the free variables, until all have read them; then nf_convert_eq's
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const VcProlog<S> pr = vc_prologue<S>(vc, cols, slots, slot_cells, hdr);
    S * const slot = pr.slot; const int * const fv = pr.fv;
    const int nfree = pr.nfree, n = pr.n;
    const int rows_max = leq_rows + 2 * eq_rows;
    const int Rlp = is_max ? rows_max : n, Vlp = is_max ? n : rows_max;      // the largest normal form under the vc found
    if (pr.general || nfree > nfree_cap || eq_rows > (int)SIX_VC_MAX_EQ || Rlp > Rmax || Vlp + Rlp + 2 > ld ||
        hbm_side_bytes<S>(Rlp, Vlp) > (size_t)lds_bytes) {
        vc_end_all<S>(tid, nt, nb, out_status, out_v, out_pivots);
        return;
    }
    const SixVcHbmSlot sl = six_vc_hbm_slot(leq_rows, eq_rows, cols, nfree_cap, Rmax, ld);
    S * const L = slot + sl.L; S * const E = slot + sl.E; int * const rest = (int *)(slot + sl.rest);
    S * const N = slot + sl.N; S * const obj = slot + sl.obj; S * const y = slot + sl.y; S * const vout = slot + sl.v;
    S * const tab = slot + sl.tab;
    const int lcells = leq_rows * cols, ecells = eq_rows * cols;

    for (int lp = (int)blockIdx.x; lp < nb; lp += (int)gridDim.x) {
        const S * tg = tgtf + (size_t)lp * cols;
        vc_stage<S>(tid, nt, leq, lcells, eqs, ecells, lp, L, E);
        const int nrest = vc_reshape<S>(L, leq_rows, cols, E, eq_rows, rest, hdr, tg, fv, nfree, obj, N);    // on the slot
        if (nrest < 0) {
            if (tid == 0) { out_status[lp] = XPG_ERR_REF_UNDEFINED; out_v[lp] = zero<S>(); if (out_pivots) out_pivots[lp] = 0u; }
            continue;
        }
        const int rows = leq_rows + 2 * nrest;
        // ---- solve: k_batch_hbm's, on the rows this LP has
        const SixVcHbmSolved solved = six_vc_hbm_solve<S>((XPG_AS_LDS unsigned char *)lds, (XPG_AS_GLOBAL S *)tab, ld, (XPG_AS_GLOBAL const S *)N,
                                                          (XPG_AS_GLOBAL const S *)obj, rows, n, is_max, max_iter, (XPG_AS_GLOBAL S *)y,
                                                          (XPG_AS_GLOBAL S *)vout);
        const int status = solved.status;
        if (tid == 0 && out_pivots) out_pivots[lp] = solved.pivots;
        if (status != 0) {
            if (tid == 0) { out_status[lp] = status; out_v[lp] = zero<S>(); }
            continue;
        }
        // ---- finish (calcFinalSolution): the products into obj, which has done its work
        vc_finish<S>(y, tg, cols, fv, nfree, obj, out_sol + (size_t)lp * cols, out_v + lp, out_status + lp);
    }
}

// The launch of k_six_batch_vc_hbm for a plan on the HBM route; every pointer is a device pointer.
template <class S>
int six_vc_hbm_launch(xpg_ctx * ctx, const SixVcHbmPlan & g, int nfree_cap, bool is_max, int nb, const S * tgtf, const S * vc, const S * eqs,
                      int eq_rows, const S * leq, int leq_rows, int cols, unsigned max_iter, int32_t * out_status, S * out_v, S * out_sol,
                      uint32_t * out_pivots)
{
    Scratch & slots = ctx->scratch[SCRATCH_SIX_VC_HBM];
    if (const int rc = scratch_reserve(ctx, slots, g.scratch, g.scratch, "hipMalloc(six_batch_vc_hbm scratch)")) return rc;
    if (const int rc = hbm_static_lds_check(ctx, (const void *)k_six_batch_vc_hbm<S>, SIX_VC_HBM_LDS_STATIC,
                                            "k_six_batch_vc_hbm: static LDS above SIX_VC_HBM_LDS_STATIC"))
        return rc;
    XPG_HIP(ctx, lds_limit((const void *)k_six_batch_vc_hbm<S>, ctx->device, g.lds));
    hipLaunchKernelGGL((k_six_batch_vc_hbm<S>), dim3((unsigned)g.grid), dim3((unsigned)g.threads), g.lds, ctx->stream, nb, tgtf, vc, eqs, eq_rows,
                       leq, leq_rows, cols, is_max ? 1 : 0, max_iter, nfree_cap, g.Rmax, g.ld, (unsigned)g.lds,
                       (unsigned long long *)slots.buf, (unsigned long long)(g.slot / 8), out_status, out_v, out_sol, out_pivots);
    XPG_HIP(ctx, hipGetLastError());
    return 0;
}

// Device arrays in and out, enqueue only (a scratch area that has to grow waits for the stream first). The host never
// sees vc: where the shape fits 64 KB with every variable free, k_six_batch_vc is launched untouched (it does not count
// pivots: out_pivots is set to 0xFFFFFFFF, "not counted"); otherwise every LP takes k_six_batch_vc_hbm.
template <class S>
int six_batch_vc_hbm_dev(xpg_ctx * ctx, bool is_max, int nb, const S * tgtf, const S * vc, const S * eqs, int eq_rows, const S * leq,
                         int leq_rows, int cols, unsigned max_iter, int32_t * out_status, S * out_v, S * out_sol, uint32_t * out_pivots)
{
    SixVcHbmRoute & rt = six_vc_hbm_route();
    rt = SixVcHbmRoute{0, 0, 0, -1, 0};
    if (!six_vc_args_ok(ctx, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, out_status, out_v, out_sol)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const SixVcHbmPlan g = six_vc_hbm_plan<S>(true, -1, leq_rows, eq_rows, cols, is_max, nb, ctx_cus(ctx));
    if (g.route == SIX_VC_HBM_ROUTE_OTHER) return XPG_ERR_UNSUPPORTED;
    if (g.route == SIX_VC_HBM_ROUTE_LDS) {
        const int rc = six_batch_vc_dev<S>(ctx, is_max, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, max_iter, -1, out_status, out_v, out_sol);
        if (rc) return rc;
        if (out_pivots) XPG_HIP(ctx, hipMemsetAsync(out_pivots, 0xFF, (size_t)nb * 4, ctx->stream));
        rt.lds = nb; rt.grid = g.grid;
        return 0;
    }
    const int rc = six_vc_hbm_launch<S>(ctx, g, cols - 1, is_max, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, max_iter, out_status, out_v,
                                        out_sol, out_pivots);
    if (rc) return rc;
    rt.hbm = nb; rt.grid = g.grid;
    return 0;
}

// Host arrays; synchronises once. The LDS route and the per-problem route are six_batch_vc_host's, called as
// xpg_six_batch_vc_* calls it.
template <class S>
int six_batch_vc_hbm_host(xpg_ctx * ctx, int kind, bool is_max, int nb, const S * tgtf, const S * vc, const S * eqs, int eq_rows, const S * leq,
                          int leq_rows, int cols, unsigned max_iter, int32_t * out_status, S * out_v, S * out_sol)
{
    SixVcHbmRoute & rt = six_vc_hbm_route();
    rt = SixVcHbmRoute{0, 0, 0, 0, 0};
    if (!six_vc_args_ok(ctx, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, out_status, out_v, out_sol)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    std::vector<int> fvar;
    const bool pattern = vc_sign_pattern(vc, cols - 1, cols, fvar);
    const int nfree = pattern ? (int)fvar.size() : 0;
    const SixVcHbmPlan g = six_vc_hbm_plan<S>(pattern, nfree, leq_rows, eq_rows, cols, is_max, nb, ctx_cus(ctx));
    if (g.route != SIX_VC_HBM_ROUTE_HBM) {
        const int rc = six_batch_vc_host<S>(ctx, kind, is_max, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, max_iter, out_status, out_v, out_sol);
        const SixVcRoute & r = six_vc_route();
        rt.lds = r.device; rt.fallback = r.fallback; rt.free_vars = r.free_vars; rt.grid = rc == 0 && r.device ? g.grid : 0;
        return rc;
    }
    BatchIo io;
    int rc = io.up(ctx, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols);
    if (rc) return rc;
    rc = six_vc_hbm_launch<S>(ctx, g, nfree, is_max, nb, (const S *)io.dt.p, (const S *)io.dvc.p, (const S *)io.de.p, eq_rows, (const S *)io.dl.p,
                              leq_rows, cols, max_iter, (int32_t *)io.dst.p, (S *)io.dv.p, (S *)io.ds.p, nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    rc = io.down(ctx, nb, cols, out_status, out_v, out_sol);
    if (rc) return rc;
    rt.hbm = nb; rt.free_vars = nfree; rt.grid = g.grid;
    return 0;
}

} // namespace xpg
