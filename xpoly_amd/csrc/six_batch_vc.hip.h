// Batches of small LPs WITH equalities and free variables (xpg_six_batch_vc_*): SIX::maxm / minm as the reference's callers
// use it -- eq and leq per problem, one vc shared by the batch -- for nb problems in ONE launch. What six_solve does on the
// host around a batch launch of one LP moves onto the device: SIX::normalize (src/com/lpsol.h:1290-1394) with
// convertEq2Ineq (:1197-1278) in front of the LDS-resident solve, calcFinalSolution (:1851-1899) behind it. One workgroup
// owns one LP from the caller's arrays to the answer:
//   reshape  SIX::normalize as normalize_dev.hip.h states it for every device route: convertEq2Ineq's choices from this LP's
//            eq alone, each substitution folded into this LP's inequalities as it is chosen (where the reference's leading
//            value, :1232, leaves the row the LP ends XPG_ERR_REF_UNDEFINED and never meets the pivot loop), then the normal
//            form N [rows x (n + 1)] (kept equalities as pairs, twins of the free variables) and the normalised objective
//            into the workgroup's scratch slot
//   solve    sm_solve_lp (batch_kernels.hip.h) on N, raw solution
//   finish   calcFinalSolution: undo the split, the objective on the ORIGINAL tgtf in column order, reduce
// The caller's leq / eq are staged in the LP's LDS block BEFORE sm_carve claims it and reshaped there. They always fit: the
// solver's tableau alone holds (leq_rows + 2 eq_rows) x (n + rows + 2) cells for maxm, and for minm its three rows of
// n + rows + 2 cells, three counters per column and n rows of the tableau outweigh the (leq_rows + eq_rows) x (cols + 2) cells
// staged (the kernel checks, and refuses instead of writing past the block). The number of equalities kept as pairs differs per LP, so
// the normal forms of a batch are ragged in rows: the slot is sized for the largest (leq_rows + 2 eq_rows), the LDS is
// carved per LP for the rows it has -- the arrays a single call (six_solve -> k_batch, nb = 1) carves, so both give the same
// bits. Slots belong to the WORKGROUP, not the LP (a workgroup walks its LPs one after the other): the scratch of a launch
// is grid x slot whatever nb is, the grid is cut so that it stays under SIX_VC_SCRATCH_MAX, and nothing is chunked.
#pragma once
#include "six_host.hip.h"

namespace xpg {

// Which route the LPs of the calling thread's last xpg_six_batch_vc_* call took (xpg_six_batch_last_route).
struct SixVcRoute { long long device, fallback, free_vars; };
inline SixVcRoute & six_vc_route() { static thread_local SixVcRoute r = {0, 0, 0}; return r; }

enum { SIX_VC_LDS_MAX = 64 * 1024, SIX_VC_MAX_EQ = 4096 };
#define SIX_VC_SCRATCH_MAX ((size_t)256 << 20)

// THE route rule (the launch and xpg_test_six_batch_vc_plan both ask it): the batch is reshaped and solved on the device
// when vc is a sign pattern (vc_sign_pattern) and the largest normal form a problem of the batch can have --
// leq_rows + 2 eq_rows inequalities (no equality substituted), cols - 1 + nfree variables -- fits 64 KB of LDS in the
// direction asked: NormalForm::fits_lds's bound, so a problem the device route takes is one six_solve solves LDS-resident.
struct SixVcPlan { int device, nfree, rows_max, n; size_t lds; };
template <class S> __host__ __device__ inline SixVcPlan six_vc_plan(bool pattern, int nfree, int leq_rows, int eq_rows, int cols, bool is_max)
{
    SixVcPlan p;
    p.nfree = nfree; p.rows_max = leq_rows + 2 * eq_rows; p.n = cols - 1 + nfree;
    p.lds = small_lds_bytes<S>(is_max ? p.rows_max : p.n, is_max ? p.n : p.rows_max);
    p.device = pattern && p.lds <= (size_t)SIX_VC_LDS_MAX && eq_rows <= SIX_VC_MAX_EQ ? 1 : 0;
    return p;
}

// The scratch slot of one workgroup in HBM, in 8-byte cells: fv (the free variables, ascending) | N | obj | y | v.
// And what the reshaping holds in LDS while it runs (work_cells): L (the inequalities, folded in place) | E | rest (int).
struct SixVcSlot { size_t fv, N, obj, y, v, cells; size_t L, E, rest, work_cells; };
__host__ __device__ inline SixVcSlot six_vc_slot(int leq_rows, int eq_rows, int cols, int nfree)
{
    const size_t n0 = (size_t)cols - 1, n = n0 + (size_t)nfree, rows_max = (size_t)leq_rows + 2 * (size_t)eq_rows;
    SixVcSlot s;
    size_t o = 0;
    s.fv = o; o += (n0 + 1) / 2;
    s.N = o; o += rows_max * (n + 1);
    s.obj = o; o += n + 1;
    s.y = o; o += n + 1;
    s.v = o; o += 1;
    size_t w = 0;
    s.L = w; w += (size_t)leq_rows * cols;
    s.E = w; w += (size_t)eq_rows * cols;
    s.rest = w; w += ((size_t)eq_rows + 1) / 2;
    s.work_cells = w;
    s.cells = (o + 31) & ~(size_t)31;        // slots start on 256-byte lines
    return s;
}

// What every xpg_six_batch_vc_* and xpg_six_batch_vc_hbm_* entry point asks of its arguments.
inline bool six_vc_args_ok(const xpg_ctx * ctx, int nb, const void * tgtf, const void * vc, const void * eqs, int eq_rows,
                           const void * leq, int leq_rows, int cols, const void * out_status, const void * out_v, const void * out_sol)
{
    return ctx && nb >= 0 && tgtf && vc && cols >= 2 && eq_rows >= 0 && leq_rows >= 0 && !(eq_rows == 0 && leq_rows == 0) &&
           !(eq_rows > 0 && !eqs) && !(leq_rows > 0 && !leq) && out_status && out_v && out_sol;
}

// vc on the device (k_six_batch_vc, k_six_batch_vc_hbm), by all threads: is it a sign pattern, and which variables are free
// (lpsol.h:1321-1339: a column of vc without a nonzero). Returns whether vc is general, i.e. no sign pattern; behind its
// barrier fv holds the free variables, ascending, and hdr[0] their number.
template <class S> __device__ __forceinline__ bool vc_scan(const S * __restrict__ vc, int n0, int cols, int * fv, int * hdr)
{
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x, lane = tid & 63;
    const S m1 = minus_one<S>();
    bool bad = false;
    for (int t = tid; t < n0 * cols; t += nt) {
        const int i = t / cols, j = t - i * cols;
        const S c = vc[t];
        if (j == i) bad |= !eq(c, zero<S>()) && !eq(c, m1);
        else bad |= !eq(c, zero<S>());
    }
    if (tid < 64) {
        int cnt = 0;
        for (int base = 0; base < n0; base += 64) {
            const int j = base + lane;
            const bool fr = j < n0 && eq(vc[(size_t)j * cols + j], zero<S>());
            const unsigned long long mask = __ballot(fr);
            if (fr) fv[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = j;
            cnt += __popcll(mask);
        }
        if (tid == 0) hdr[0] = cnt;
    }
    return __syncthreads_or(bad ? 1 : 0) != 0;                   // (a barrier: hdr[0] and fv are the workgroup's now)
}

// calcFinalSolution behind a solve that ended 0, by all threads: the split undone in y, the products with the ORIGINAL tgtf
// into prod, the reduced solution into out_sol; their sum in column order, v and status 0 by thread 0.
template <class S> __device__ __forceinline__ void vc_finish(S * y, const S * tg, int cols, const int * fv, int nfree, S * prod, S * out_sol,
                                                             S * out_v, int32_t * out_status)
{
    nf_unsplit<S>(y, cols, fv, nfree);
    nf_products<S>(y, tg, cols, prod, out_sol);
    if (threadIdx.x == 0) {
        S v = zero<S>();
        for (int j = 0; j < cols; j++) v = add(v, prod[j]);
        reduce(v);
        *out_v = v;
        *out_status = 0;
    }
}

// The LP loop's steps that k_six_batch_vc, k_six_batch_vc_hbm and the two has_solution kernels (has_solution_batch.hip.h) share,
// on plain pointers like the nf_* they drive: whether L, E and rest lie in the LDS block or in the slot is the caller's business.
// Prologue: the workgroup's slot, fv at its cell 0 (whatever the shape is, in SixVcSlot and SixVcHbmSlot), vc_scan and what it
// found. The device-memory kernels call it; k_six_batch_vc and k_has_solution_batch, with sm_solve_lp inlined, keep its five
// lines: through the function their register allocation moved (profiles/vc_kernels_shared_isa.txt).
template <class S> struct VcProlog { S * slot; int * fv; bool general; int nfree, n; };
template <class S> __device__ __forceinline__ VcProlog<S> vc_prologue(const S * vc, int cols, unsigned long long * slots, unsigned long long slot_cells,
                                                                      int * hdr)
{
    const int n0 = cols - 1;
    VcProlog<S> p;
    p.slot = (S *)(slots + (size_t)blockIdx.x * slot_cells);
    p.fv = (int *)p.slot;
    p.general = vc_scan<S>(vc, n0, cols, p.fv, hdr);
    p.nfree = hdr[0]; p.n = n0 + p.nfree;
    return p;
}
// Every LP of the launch ends XPG_ERR_UNSUPPORTED (a general vc, a shape the launch was not sized for). tid, nt: threadIdx.x and
// blockDim.x as the kernel read them at its top, here and in vc_stage.
template <class S> __device__ __forceinline__ void vc_end_all(int tid, int nt, int nb, int32_t * out_status, S * out_v, uint32_t * out_pivots)
{
    for (int lp = (int)blockIdx.x * nt + tid; lp < nb; lp += (int)gridDim.x * nt) {
        out_status[lp] = XPG_ERR_UNSUPPORTED; out_v[lp] = zero<S>();
        if (out_pivots) out_pivots[lp] = 0u;
    }
}
// Stage: problem lp's cells as they lie, whole rows by consecutive lanes, between two barriers.
template <class S> __device__ __forceinline__ void vc_stage(int tid, int nt, const S * leq, int lcells, const S * eqs, int ecells, int lp, S * L, S * E)
{
    __syncthreads();                                             // the LP before is through with the LDS block, the slot and hdr
    const S * gl = leq + (size_t)lp * lcells; const S * ge = eqs + (size_t)lp * ecells;
    for (int t = tid; t < lcells; t += nt) L[t] = gl[t];
    for (int t = tid; t < ecells; t += nt) E[t] = ge[t];
    __syncthreads();
}
// Reshape (normalize_dev.hip.h): L folded in place, then the normalised objective and N. Returns nf_convert_eq's answer: the
// equalities kept as pairs (the normal form has leq_rows + 2 of them rows), or < 0: that LP alone ends XPG_ERR_REF_UNDEFINED and
// never meets the pivot loop. Behind nf_form's barrier L / E are read: where they lie in the LDS block, that is the solver's.
template <class S> __device__ __forceinline__ int vc_reshape(S * L, int leq_rows, int cols, const S * E, int eq_rows, int * rest, int * hdr, const S * tg,
                                                             const int * fv, int nfree, S * obj, S * N)
{
    const EqRows<S> eq = {E, cols};
    const int nrest = nf_convert_eq<S>(L, leq_rows, cols, eq, eq_rows, rest, hdr);
    if (nrest < 0) return nrest;
    nf_objective<S>(tg, cols, fv, nfree, obj);
    nf_form<S>(L, leq_rows, cols, eq, rest, nrest, fv, nfree, N);
    return nrest;
}

// One workgroup per LP, grid-stride over the batch. vc is read on the device (the _dev entry points hold it there): every
// workgroup derives the free list once; a vc that is no sign pattern, or a normal form beyond the launch's LDS, ends
// every LP XPG_ERR_UNSUPPORTED (the host-array entry point has sent such a batch to six_solve instead and never launches).
template <class S> __global__ __launch_bounds__(256, 4)
void k_six_batch_vc(int nb, const S * __restrict__ tgtf, const S * __restrict__ vc, const S * __restrict__ eqs, int eq_rows,
                    const S * __restrict__ leq, int leq_rows, int cols, int is_max, unsigned max_iter, unsigned lds_bytes,
                    unsigned long long * __restrict__ slots, unsigned long long slot_cells,
                    int32_t * __restrict__ out_status, S * __restrict__ out_v, S * __restrict__ out_sol)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int hdr[4];                                       // [0]: the free variables, until all have read them; then nf_convert_eq's
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int n0 = cols - 1;                                     // (vc_prologue's lines: through it this kernel's spills move)
    S * const slot = (S *)(slots + (size_t)blockIdx.x * slot_cells);
    int * const fv = (int *)slot;
    const bool general = vc_scan<S>(vc, n0, cols, fv, hdr);
    const int nfree = hdr[0], n = n0 + nfree;
    const SixVcPlan plan = six_vc_plan<S>(!general, nfree, leq_rows, eq_rows, cols, is_max != 0);
    const SixVcSlot sl = six_vc_slot(leq_rows, eq_rows, cols, nfree);
    if (!plan.device || plan.lds > (size_t)lds_bytes || sl.work_cells * 8 > (size_t)lds_bytes) {
        vc_end_all<S>(tid, nt, nb, out_status, out_v, nullptr);
        return;
    }
    S * const N = slot + sl.N; S * const obj = slot + sl.obj; S * const y = slot + sl.y; S * const vout = slot + sl.v;
    S * const work = (S *)lds;
    S * const L = work + sl.L; S * const E = work + sl.E; int * const rest = (int *)(work + sl.rest);
    const int lcells = leq_rows * cols, ecells = eq_rows * cols;

    for (int lp = (int)blockIdx.x; lp < nb; lp += (int)gridDim.x) {
        const S * tg = tgtf + (size_t)lp * cols;
        vc_stage<S>(tid, nt, leq, lcells, eqs, ecells, lp, L, E);
        const int nrest = vc_reshape<S>(L, leq_rows, cols, E, eq_rows, rest, hdr, tg, fv, nfree, obj, N);
        if (nrest < 0) {
            if (tid == 0) { out_status[lp] = XPG_ERR_REF_UNDEFINED; out_v[lp] = zero<S>(); }
            continue;
        }
        const int rows = leq_rows + 2 * nrest;
        // ---- solve: the arrays and the code of a single call's launch (k_batch with nb = 1 on this normal form)
        Small<S> P;
        sm_carve(P, lds, is_max ? rows : n, is_max ? n : rows);
        Source<S> src;
        src.leq = N; src.tgtf = obj; src.m = rows; src.cols = n + 1; src.is_max = is_max;
        const int status = sm_solve_lp<S>(P, src, max_iter, /*raw_sol=*/1, y, vout);
        if (status != 0) {
            if (tid == 0) { out_status[lp] = status; out_v[lp] = zero<S>(); }
            continue;
        }
        // ---- finish (calcFinalSolution): the products into obj, which has done its work
        vc_finish<S>(y, tg, cols, fv, nfree, obj, out_sol + (size_t)lp * cols, out_v + lp, out_status + lp);
    }
}

// The scratch cut of the LDS-resident launches: grid x slot stays under SIX_VC_SCRATCH_MAX, with one workgroup at the least.
inline long long six_vc_scratch_cut(long long grid, size_t slot_bytes)
{
    const long long by_scratch = (long long)(SIX_VC_SCRATCH_MAX / slot_bytes);
    return grid > by_scratch ? (by_scratch > 0 ? by_scratch : 1) : grid;
}
// The grid of an LDS-resident launch whose workgroups hold `lds` bytes each and one slot of slot_bytes: what 160 KB hold, 16
// at the most, on 256 x 64 places; no more than nb; under the scratch cut. (six_vc_geometry for one shape, and the ragged
// has_solution launch for the largest of its systems, has_solution_batch.hip.h.)
inline long long six_vc_grid(size_t lds, long long nb, size_t slot_bytes)
{
    const int per_cu = (int)((160 * 1024) / lds) > 0 ? (int)((160 * 1024) / lds) : 1;
    long long grid = 256ll * (per_cu > 16 ? 16 : per_cu) * 64;
    if (grid > nb) grid = nb;
    return six_vc_scratch_cut(grid, slot_bytes);
}
// The launch of k_six_batch_vc for a shape the device route takes (six_batch_vc_dev asks it, and the route rule of
// xpg_six_batch_vc_hbm_* reports it): nfree as six_batch_vc_dev takes it.
struct SixVcGeom { size_t lds; int threads; long long grid; size_t slot_cells; };
template <class S> inline SixVcGeom six_vc_geometry(int nfree, int nb, int leq_rows, int eq_rows, int cols, bool is_max)
{
    const int nfree_cap = nfree >= 0 ? nfree : cols - 1;
    const SixVcPlan least = six_vc_plan<S>(true, nfree >= 0 ? nfree : 0, leq_rows, eq_rows, cols, is_max);
    const SixVcPlan most = six_vc_plan<S>(true, nfree_cap, leq_rows, eq_rows, cols, is_max);
    SixVcGeom q;
    q.lds = most.lds < (size_t)SIX_VC_LDS_MAX ? most.lds : (size_t)SIX_VC_LDS_MAX;
    q.slot_cells = six_vc_slot(leq_rows, eq_rows, cols, nfree_cap).cells;
    const int R = is_max ? least.rows_max : least.n, V = is_max ? least.n : least.rows_max;
    const int cells = R * (V + R + 2);
    q.threads = cells >= 2048 ? 256 : (cells >= 1024 ? 128 : 64);             // batch_geometry's rule
    q.grid = six_vc_grid(q.lds, nb, q.slot_cells * 8);
    return q;
}

// Enqueue only; every pointer is a device pointer. nfree >= 0: the caller has read vc (the host-array form); -1: vc is known
// to the device alone -- LDS and slots are sized for the worst vc can hold (every variable free), the kernel sizes each LP
// by what it finds.
template <class S>
int six_batch_vc_dev(xpg_ctx * ctx, bool is_max, int nb, const S * tgtf, const S * vc, const S * eqs, int eq_rows, const S * leq,
                     int leq_rows, int cols, unsigned max_iter, int nfree, int32_t * out_status, S * out_v, S * out_sol)
{
    if (!six_vc_args_ok(ctx, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, out_status, out_v, out_sol)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const SixVcPlan least = six_vc_plan<S>(true, nfree >= 0 ? nfree : 0, leq_rows, eq_rows, cols, is_max);
    if (!least.device) return XPG_ERR_UNSUPPORTED;               // (no vc makes this shape fit)
    const SixVcGeom q = six_vc_geometry<S>(nfree, nb, leq_rows, eq_rows, cols, is_max);
    const size_t lds = q.lds;
    const int threads = q.threads;
    long long grid = q.grid;
    const int grid_cap = XPG_INT_HOOK("XPG_SIX_VC_GRID");        // tests: the grid-stride path at small nb
    if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
    const size_t need = (size_t)grid * q.slot_cells * 8;
    Scratch & slots = ctx->scratch[SCRATCH_SIX_VC];              // grown with head room, so a batch a little larger does not grow it again
    if (const int rc = scratch_reserve(ctx, slots, need, need + need / 2 < SIX_VC_SCRATCH_MAX ? need + need / 2 : need, "hipMalloc(six_batch_vc scratch)"))
        return rc;
    XPG_HIP(ctx, lds_limit((const void *)k_six_batch_vc<S>, ctx->device, lds));
    hipLaunchKernelGGL((k_six_batch_vc<S>), dim3((unsigned)grid), dim3(threads), lds, ctx->stream, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows,
                       cols, is_max ? 1 : 0, max_iter, (unsigned)lds, (unsigned long long *)slots.buf, (unsigned long long)q.slot_cells,
                       out_status, out_v, out_sol);
    XPG_HIP(ctx, hipGetLastError());
    return 0;
}

// Host arrays; synchronises once. The route rule decides: the device for the whole batch, or six_solve per problem (a
// general vc, a normal form beyond 64 KB), so the call is defined wherever SIX::maxm / minm is. Same results either way.
template <class S>
int six_batch_vc_host(xpg_ctx * ctx, int kind, bool is_max, int nb, const S * tgtf, const S * vc, const S * eqs, int eq_rows, const S * leq,
                      int leq_rows, int cols, unsigned max_iter, int32_t * out_status, S * out_v, S * out_sol)
{
    if (!six_vc_args_ok(ctx, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, out_status, out_v, out_sol)) return XPG_ERR_SHAPE;
    SixVcRoute & rt = six_vc_route();
    rt = SixVcRoute{0, 0, 0};
    if (nb == 0) return 0;
    std::vector<int> fvar;
    const bool pattern = vc_sign_pattern(vc, cols - 1, cols, fvar);
    const SixVcPlan plan = six_vc_plan<S>(pattern, (int)fvar.size(), leq_rows, eq_rows, cols, is_max);
    if (!plan.device) {
        for (int b = 0; b < nb; b++) {
            out_v[b] = zero<S>();
            const int st = six_solve<S>(ctx, kind, is_max, tgtf + (size_t)b * cols, vc, cols - 1, eq_rows > 0 ? eqs + (size_t)b * eq_rows * cols : (const S *)0,
                                        eq_rows, leq_rows > 0 ? leq + (size_t)b * leq_rows * cols : (const S *)0, leq_rows, cols, max_iter,
                                        out_v + b, out_sol + (size_t)b * cols);
            if (st < 0 && st != XPG_ERR_REF_UNDEFINED) return st;
            out_status[b] = st;
            if (st != 0) out_v[b] = zero<S>();
            rt.fallback++;
        }
        return 0;
    }
    BatchIo io;
    int rc = io.up(ctx, nb, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols);
    if (rc) return rc;
    rc = six_batch_vc_dev<S>(ctx, is_max, nb, (const S *)io.dt.p, (const S *)io.dvc.p, (const S *)io.de.p, eq_rows, (const S *)io.dl.p, leq_rows, cols,
                             max_iter, plan.nfree, (int32_t *)io.dst.p, (S *)io.dv.p, (S *)io.ds.p);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    rc = io.down(ctx, nb, cols, out_status, out_v, out_sol);
    if (rc) return rc;
    rt.device = nb; rt.free_vars = plan.nfree;
    return 0;
}

} // namespace xpg
