// Lineq::has_solution (src/com/linsys.cpp:830-906) for a batch of systems of one shape in ONE launch (xpg_has_solution_batch_*):
// maxm on SIX::reviseTargetFunc's all-ones objective, then minm where that left the question open. One workgroup owns one
// system from the caller's arrays to the verdict, grid-stride over the batch, through the steps the four kernels of this family
// share (six_batch_vc.hip.h: vc_prologue, vc_stage, vc_reshape) and has_solution's rules as six_host.hip.h states them once
// (hs_verdict, hs_no_inequality, hs_store):
//   stage      vc_stage: leq and eq between two barriers
//   objective  hs_objective below: feasibility_objective (six_host.hip.h) on the cells as staged, BEFORE any fold, into tg
//   normalise  ONCE, vc_reshape: nf_convert_eq, nf_objective, nf_form (normalize_dev.hip.h) into the slot's N and obj
//   maxm       the carve of a single call for (rows, n), sm_solve_lp with is_max = 1, raw solution
//   minm       if hs_verdict leaves it open: the carve for the dual's shape over the same LDS, sm_solve_lp with is_max = 0 on the
//              SAME N and obj -- sm_solve_lp reads its source and never writes it
// There is no calcFinalSolution (vc_finish never changes a status), so the statuses are those of two single
// xpg_six_{maxm,minm}_rat32 calls and the verdict is has_solution()'s (mip_front.hip.h). Two kernels: k_has_solution_batch, the
// LDS-resident form of k_six_batch_vc, and k_has_solution_batch_hbm, the device-memory form of k_six_batch_vc_hbm; their two-pass
// loops stay two (one body taking the solve as a callable moved the spills of both). ONE route rule (hs_plan) sends the whole
// batch to one of them, sized for the larger direction, or to the host.
// Slots are those of the two kernels this one joins with tg [cols] behind them: six_vc_slot | tg, six_vc_hbm_slot | tg, in
// the handle's SCRATCH_SIX_VC / SCRATCH_SIX_VC_HBM areas. is_int_sol = 1 is composed on the host from xpg_mip_batch_vc_hbm_rat32.
#pragma once
#include "six_batch_vc_hbm.hip.h"

namespace xpg {

// What the calling thread's last xpg_has_solution_batch_* call did (xpg_has_solution_batch_last_route): systems on route 0 / 1 /
// 2, systems whose second solve ran (-1 after a _dev call: only the device knows), the grid of the launch.
struct HsRoute { long long lds, hbm, host, second, grid; };
inline HsRoute & hs_route() { static thread_local HsRoute r = {0, 0, 0, 0, 0}; return r; }

enum { HS_ROUTE_LDS = 0, HS_ROUTE_HBM = 1, HS_ROUTE_OTHER = 2 };

// THE route rule (the launch and xpg_test_has_solution_batch_plan both ask it), from the plans of the two directions
// (six_vc_hbm_plan, which asks six_vc_plan): nfree as six_vc_hbm_plan takes it.
//   LDS    both directions keep k_six_batch_vc's launch: k_has_solution_batch, LDS and threads of the larger direction
//   HBM    a sign pattern past that with neither direction refused: k_has_solution_batch_hbm, side arrays, tableau rows and
//          slot of the larger of each, under the limits six_vc_hbm_plan holds one direction to
//   OTHER  the host-array form calls has_solution() per system, the _dev form returns XPG_ERR_UNSUPPORTED before any launch
struct HsPlan {
    int route, nfree, Rmax;
    size_t lds;             // LDS route: the larger small_lds_bytes; else the larger hbm_side_bytes
    size_t slot;            // bytes of one workgroup's slot, tg included
    int ld, threads, grid;
    size_t scratch;         // grid x slot
    size_t tg_cell;         // where tg starts in the slot, in 8-byte cells
};
template <class S> inline HsPlan hs_plan(bool pattern, int nfree, int leq_rows, int eq_rows, int cols, int nb, int num_cus)
{
    const SixVcHbmPlan a = six_vc_hbm_plan<S>(pattern, nfree, leq_rows, eq_rows, cols, true, nb, num_cus);
    const SixVcHbmPlan b = six_vc_hbm_plan<S>(pattern, nfree, leq_rows, eq_rows, cols, false, nb, num_cus);
    const size_t tgc = ((size_t)cols + 31) & ~(size_t)31;        // slots keep starting on 256-byte lines
    HsPlan g;
    g.nfree = a.nfree; g.Rmax = a.Rmax > b.Rmax ? a.Rmax : b.Rmax;
    if (a.route == SIX_VC_HBM_ROUTE_LDS && b.route == SIX_VC_HBM_ROUTE_LDS) {
        g.route = HS_ROUTE_LDS; g.lds = a.lds > b.lds ? a.lds : b.lds; g.ld = a.ld;
        g.threads = a.threads > b.threads ? a.threads : b.threads;
        g.tg_cell = a.slot / 8; g.slot = a.slot + tgc * 8;
        const long long grid = six_vc_scratch_cut(a.grid < b.grid ? a.grid : b.grid, g.slot);
        g.grid = (int)grid; g.scratch = (size_t)grid * g.slot;
        return g;
    }
    const int cap = nfree >= 0 ? nfree : cols - 1;
    const size_t sa = hbm_side_bytes<S>(a.Rmax, a.Vmax), sb = hbm_side_bytes<S>(b.Rmax, b.Vmax);
    g.lds = sa > sb ? sa : sb;
    g.ld = (int)hbm_ld(a.Rmax, a.Vmax);                          // (R + V is the same in both directions)
    g.tg_cell = six_vc_hbm_slot(leq_rows, eq_rows, cols, cap, g.Rmax, g.ld).cells;
    g.slot = (g.tg_cell + tgc) * 8;
    g.threads = SIX_VC_HBM_THREADS;
    g.grid = six_vc_hbm_grid(a.route != SIX_VC_HBM_ROUTE_OTHER && b.route != SIX_VC_HBM_ROUTE_OTHER, g.lds, g.slot, nb, num_cus);
    g.route = g.grid > 0 ? HS_ROUTE_HBM : HS_ROUTE_OTHER;
    g.scratch = (size_t)g.grid * g.slot;
    return g;
}

// feasibility_objective (six_host.hip.h) by all threads, a thread a column: tg[j] = 1 where some staged inequality or equality
// has a nonzero in column j < cols - 1, else 0. Behind its barrier tg is the workgroup's.
template <class S> __device__ __forceinline__ void hs_objective(const S * L, int leq_rows, const S * E, int eq_rows, int cols, S * tg)
{
    for (int j = (int)threadIdx.x; j < cols; j += (int)blockDim.x) {
        bool nz = false;
        if (j < cols - 1) {
            for (int i = 0; i < leq_rows && !nz; i++) nz = ne(L[(size_t)i * cols + j], zero<S>());
            for (int i = 0; i < eq_rows && !nz; i++) nz = ne(E[(size_t)i * cols + j], zero<S>());
        }
        tg[j] = nz ? one<S>() : zero<S>();
    }
    __syncthreads();
}
// Every system of the launch ends `has` without a solve (a general vc, a shape the launch was not sized for; leq_rows = 0).
__device__ __forceinline__ void hs_end_all(int nb, int has, int s0, int32_t * out_has, int32_t * out_status)
{
    for (int b = (int)(blockIdx.x * blockDim.x + threadIdx.x); b < nb; b += (int)(gridDim.x * blockDim.x))
        hs_store(b, has, s0, XPG_HS_NOT_RUN, out_has, out_status);
}
__global__ void k_hs_fill(int nb, int has, int s0, int32_t * out_has, int32_t * out_status) { hs_end_all(nb, has, s0, out_has, out_status); }

// The LDS-resident form: k_six_batch_vc with the objective built on the device and the solve asked twice.
template <class S> __global__ __launch_bounds__(256, 4)
void k_has_solution_batch(int nb, const S * __restrict__ vc, const S * __restrict__ eqs, int eq_rows, const S * __restrict__ leq, int leq_rows,
                          int cols, int is_unique, unsigned max_iter, unsigned lds_bytes, unsigned long long * __restrict__ slots,
                          unsigned long long slot_cells, unsigned long long tg_cell, int32_t * __restrict__ out_has,
                          int32_t * __restrict__ out_status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int hdr[4];                                       // [0]: the free variables, until all have read them; then nf_convert_eq's
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int n0 = cols - 1;                                     // (vc_prologue's lines: through it this kernel's spills move)
    S * const slot = (S *)(slots + (size_t)blockIdx.x * slot_cells);
    int * const fv = (int *)slot;
    const bool general = vc_scan<S>(vc, n0, cols, fv, hdr);
    const int nfree = hdr[0], n = n0 + nfree;
    const SixVcPlan up = six_vc_plan<S>(!general, nfree, leq_rows, eq_rows, cols, true);
    const SixVcPlan down = six_vc_plan<S>(!general, nfree, leq_rows, eq_rows, cols, false);
    const SixVcSlot sl = six_vc_slot(leq_rows, eq_rows, cols, nfree);
    if (!up.device || !down.device || up.lds > (size_t)lds_bytes || down.lds > (size_t)lds_bytes || sl.work_cells * 8 > (size_t)lds_bytes ||
        sl.cells > (size_t)tg_cell || tg_cell + (size_t)cols > (size_t)slot_cells) {
        hs_end_all(nb, XPG_ERR_UNSUPPORTED, XPG_ERR_UNSUPPORTED, out_has, out_status);
        return;
    }
    S * const N = slot + sl.N; S * const obj = slot + sl.obj; S * const y = slot + sl.y; S * const vout = slot + sl.v;
    S * const tg = slot + tg_cell;
    S * const work = (S *)lds;
    S * const L = work + sl.L; S * const E = work + sl.E; int * const rest = (int *)(work + sl.rest);
    const int lcells = leq_rows * cols, ecells = eq_rows * cols;

    for (int lp = (int)blockIdx.x; lp < nb; lp += (int)gridDim.x) {
        vc_stage<S>(tid, nt, leq, lcells, eqs, ecells, lp, L, E);
        hs_objective<S>(L, leq_rows, E, eq_rows, cols, tg);
        const int nrest = vc_reshape<S>(L, leq_rows, cols, E, eq_rows, rest, hdr, tg, fv, nfree, obj, N);
        int has = 0, st[2] = {XPG_HS_NOT_RUN, XPG_HS_NOT_RUN};
        if (nrest < 0) {                                         // this system alone; it never meets the pivot loop
            has = st[0] = XPG_ERR_REF_UNDEFINED;
        } else {
            const int rows = leq_rows + 2 * nrest;
            for (int pass = 0; pass < 2 && has == 0; pass++) {   // maxm, then minm of what that left open
                const int is_max = pass == 0 ? 1 : 0;
                __syncthreads();                                 // pass 1 is through with the LDS block
                Small<S> P;
                sm_carve(P, lds, is_max ? rows : n, is_max ? n : rows);
                Source<S> src;
                src.leq = N; src.tgtf = obj; src.m = rows; src.cols = n + 1; src.is_max = is_max;
                st[pass] = sm_solve_lp<S>(P, src, max_iter, /*raw_sol=*/1, y, vout);
                has = hs_verdict(st[pass], is_unique != 0);
            }
        }
        if (tid == 0) hs_store(lp, has, st[0], st[1], out_has, out_status);
    }
}

// The device-memory form: k_six_batch_vc_hbm's slot, reshaping and solve (six_vc_hbm_solve, registers of its own), asked twice.
template <class S> __global__ __launch_bounds__(1024)
void k_has_solution_batch_hbm(int nb, const S * __restrict__ vc, const S * __restrict__ eqs, int eq_rows, const S * __restrict__ leq,
                              int leq_rows, int cols, int is_unique, unsigned max_iter, int nfree_cap, int Rmax, int ld, unsigned lds_bytes,
                              unsigned long long * slots, unsigned long long slot_cells, int32_t * __restrict__ out_has,
                              int32_t * __restrict__ out_status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int hdr[4];                                       // [0]: the free variables, until all have read them; then nf_convert_eq's
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const VcProlog<S> pr = vc_prologue<S>(vc, cols, slots, slot_cells, hdr);
    S * const slot = pr.slot; const int * const fv = pr.fv;
    const int nfree = pr.nfree, n = pr.n;
    const int rows_max = leq_rows + 2 * eq_rows;
    const SixVcHbmSlot sl = six_vc_hbm_slot(leq_rows, eq_rows, cols, nfree_cap, Rmax, ld);
    if (pr.general || nfree > nfree_cap || eq_rows > (int)SIX_VC_MAX_EQ || rows_max > Rmax || n > Rmax || n + rows_max + 2 > ld ||
        hbm_side_bytes<S>(rows_max, n) > (size_t)lds_bytes || hbm_side_bytes<S>(n, rows_max) > (size_t)lds_bytes ||
        sl.cells + (size_t)cols > (size_t)slot_cells) {
        hs_end_all(nb, XPG_ERR_UNSUPPORTED, XPG_ERR_UNSUPPORTED, out_has, out_status);
        return;
    }
    S * const L = slot + sl.L; S * const E = slot + sl.E; int * const rest = (int *)(slot + sl.rest);
    S * const N = slot + sl.N; S * const obj = slot + sl.obj; S * const y = slot + sl.y; S * const vout = slot + sl.v;
    S * const tab = slot + sl.tab; S * const tg = slot + sl.cells;
    const int lcells = leq_rows * cols, ecells = eq_rows * cols;

    for (int lp = (int)blockIdx.x; lp < nb; lp += (int)gridDim.x) {
        vc_stage<S>(tid, nt, leq, lcells, eqs, ecells, lp, L, E);
        hs_objective<S>(L, leq_rows, E, eq_rows, cols, tg);
        const int nrest = vc_reshape<S>(L, leq_rows, cols, E, eq_rows, rest, hdr, tg, fv, nfree, obj, N);
        int has = 0, st[2] = {XPG_HS_NOT_RUN, XPG_HS_NOT_RUN};
        if (nrest < 0) {
            has = st[0] = XPG_ERR_REF_UNDEFINED;
        } else {
            const int rows = leq_rows + 2 * nrest;
            for (int pass = 0; pass < 2 && has == 0; pass++) {   // maxm, then minm of what that left open
                __syncthreads();                                 // pass 1 is through with the LDS block and the tableau
                st[pass] = six_vc_hbm_solve<S>((XPG_AS_LDS unsigned char *)lds, (XPG_AS_GLOBAL S *)tab, ld, (XPG_AS_GLOBAL const S *)N,
                                               (XPG_AS_GLOBAL const S *)obj, rows, n, pass == 0 ? 1 : 0, max_iter, (XPG_AS_GLOBAL S *)y,
                                               (XPG_AS_GLOBAL S *)vout).status;
                has = hs_verdict(st[pass], is_unique != 0);
            }
        }
        if (tid == 0) hs_store(lp, has, st[0], st[1], out_has, out_status);
    }
}

// ---- systems of MIXED shapes under one vc (xpg_has_solution_batch_ragged_rat32) -----------------------------------------------
// System b has leq_rows[b] x cols inequalities at cell leq_off[b] of leq and eq_rows[b] x cols equalities at cell eq_off[b] of
// eqs; cols and vc are the call's. A launch walks an index list: workgroup blockIdx.x answers systems idx[blockIdx.x],
// idx[blockIdx.x + gridDim.x], ... -- the host sorts the list so that the longest solves start first, which changes no answer.
struct HsRagged { const int32_t * idx, * leq_rows, * eq_rows; const long long * leq_off, * eq_off; };
// The tableau of ONE shape on the device-memory route as hs_plan sizes it (Rmax and ld of that shape's own plan): a system of
// a ragged launch keeps them, so its slot, its solve and its bits are those of a uniform call of its shape.
struct HsHbmTab { int Rmax, ld; };
__host__ __device__ inline HsHbmTab hs_hbm_tab(int leq_rows, int eq_rows, int cols, int nfree_cap)
{
    const int rows_max = leq_rows + 2 * eq_rows, n = cols - 1 + nfree_cap;
    return HsHbmTab{rows_max > n ? rows_max : n, (int)hbm_ld(rows_max, n)};
}
// Every system of the list ends `has` without a solve (a general vc, a slot without room for tg).
__device__ __forceinline__ void hs_end_list(int nidx, const int32_t * idx, int has, int32_t * out_has, int32_t * out_status)
{
    for (int k = (int)(blockIdx.x * blockDim.x + threadIdx.x); k < nidx; k += (int)(gridDim.x * blockDim.x))
        hs_store(idx[k], has, has, XPG_HS_NOT_RUN, out_has, out_status);
}

// k_has_solution_batch over an index list. lds_bytes, slot_cells and tg_cell are the launch's: the largest of what hs_plan
// gives each system's own shape. Per system the layout is that shape's (six_vc_slot: fv at cell 0 and N behind it whatever the
// rows, obj / y / v behind N where this shape puts them; L / E / rest from the top of the LDS block); tg stays at tg_cell,
// behind the largest layout. Consecutive systems of a workgroup may lay slot and block out differently: the barrier at the top
// of vc_stage has every thread through with ALL of the block, the slot and hdr before a cell of the next layout is written,
// and a system that is refused meets no barrier and writes nothing but its own answer. A system whose own plan is past what
// the launch was sized for ends XPG_ERR_UNSUPPORTED alone.
template <class S> __global__ __launch_bounds__(256, 4)
void k_has_solution_ragged(int nidx, HsRagged sh, const S * __restrict__ vc, const S * __restrict__ eqs, const S * __restrict__ leq, int cols,
                           int is_unique, unsigned max_iter, unsigned lds_bytes, unsigned long long * __restrict__ slots,
                           unsigned long long slot_cells, unsigned long long tg_cell, int32_t * __restrict__ out_has,
                           int32_t * __restrict__ out_status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int hdr[4];                                       // [0]: the free variables, until all have read them; then nf_convert_eq's
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int n0 = cols - 1;                                     // (vc_prologue's lines, as k_has_solution_batch keeps them)
    S * const slot = (S *)(slots + (size_t)blockIdx.x * slot_cells);
    int * const fv = (int *)slot;
    const bool general = vc_scan<S>(vc, n0, cols, fv, hdr);
    const int nfree = hdr[0], n = n0 + nfree;
    if (general || tg_cell + (size_t)cols > (size_t)slot_cells) {
        hs_end_list(nidx, sh.idx, XPG_ERR_UNSUPPORTED, out_has, out_status);
        return;
    }
    S * const tg = slot + tg_cell;
    S * const work = (S *)lds;

    for (int k = (int)blockIdx.x; k < nidx; k += (int)gridDim.x) {
        const int b = sh.idx[k], leq_rows = sh.leq_rows[b], eq_rows = sh.eq_rows[b];
        const SixVcPlan up = six_vc_plan<S>(true, nfree, leq_rows, eq_rows, cols, true);
        const SixVcPlan down = six_vc_plan<S>(true, nfree, leq_rows, eq_rows, cols, false);
        const SixVcSlot sl = six_vc_slot(leq_rows, eq_rows, cols, nfree);
        if (leq_rows <= 0 || eq_rows < 0 || !up.device || !down.device || up.lds > (size_t)lds_bytes || down.lds > (size_t)lds_bytes ||
            sl.work_cells * 8 > (size_t)lds_bytes || sl.cells > (size_t)tg_cell) {
            if (tid == 0) hs_store(b, XPG_ERR_UNSUPPORTED, XPG_ERR_UNSUPPORTED, XPG_HS_NOT_RUN, out_has, out_status);
            continue;
        }
        S * const N = slot + sl.N; S * const obj = slot + sl.obj; S * const y = slot + sl.y; S * const vout = slot + sl.v;
        S * const L = work + sl.L; S * const E = work + sl.E; int * const rest = (int *)(work + sl.rest);
        vc_stage<S>(tid, nt, leq + sh.leq_off[b], leq_rows * cols, eqs + sh.eq_off[b], eq_rows * cols, 0, L, E);
        hs_objective<S>(L, leq_rows, E, eq_rows, cols, tg);
        const int nrest = vc_reshape<S>(L, leq_rows, cols, E, eq_rows, rest, hdr, tg, fv, nfree, obj, N);
        int has = 0, st[2] = {XPG_HS_NOT_RUN, XPG_HS_NOT_RUN};
        if (nrest < 0) {                                         // this system alone; it never meets the pivot loop
            has = st[0] = XPG_ERR_REF_UNDEFINED;
        } else {
            const int rows = leq_rows + 2 * nrest;
            for (int pass = 0; pass < 2 && has == 0; pass++) {   // maxm, then minm of what that left open
                const int is_max = pass == 0 ? 1 : 0;
                __syncthreads();                                 // pass 1 is through with the LDS block
                Small<S> P;
                sm_carve(P, lds, is_max ? rows : n, is_max ? n : rows);
                Source<S> src;
                src.leq = N; src.tgtf = obj; src.m = rows; src.cols = n + 1; src.is_max = is_max;
                st[pass] = sm_solve_lp<S>(P, src, max_iter, /*raw_sol=*/1, y, vout);
                has = hs_verdict(st[pass], is_unique != 0);
            }
        }
        if (tid == 0) hs_store(b, has, st[0], st[1], out_has, out_status);
    }
}

// k_has_solution_batch_hbm over an index list. Per system the slot is laid out as a uniform call of its shape lays it out
// (six_vc_hbm_slot with hs_hbm_tab of that shape: fv at cell 0, L behind it, E .. tab where this shape puts them); Rmax, ld,
// lds_bytes, slot_cells and tg_cell are the launch's -- the largest of the systems' own plans -- and tg stays at tg_cell, behind
// the largest layout. The barrier at the top of vc_stage separates two systems whatever their layouts, as above.
template <class S> __global__ __launch_bounds__(1024)
void k_has_solution_ragged_hbm(int nidx, HsRagged sh, const S * __restrict__ vc, const S * __restrict__ eqs, const S * __restrict__ leq, int cols,
                               int is_unique, unsigned max_iter, int nfree_cap, int Rmax, int ld, unsigned lds_bytes, unsigned long long * slots,
                               unsigned long long slot_cells, unsigned long long tg_cell, int32_t * __restrict__ out_has,
                               int32_t * __restrict__ out_status)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ int hdr[4];                                       // [0]: the free variables, until all have read them; then nf_convert_eq's
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const VcProlog<S> pr = vc_prologue<S>(vc, cols, slots, slot_cells, hdr);
    S * const slot = pr.slot; const int * const fv = pr.fv;
    const int nfree = pr.nfree, n = pr.n;
    if (pr.general || nfree > nfree_cap || tg_cell + (size_t)cols > (size_t)slot_cells) {
        hs_end_list(nidx, sh.idx, XPG_ERR_UNSUPPORTED, out_has, out_status);
        return;
    }
    S * const tg = slot + tg_cell;

    for (int k = (int)blockIdx.x; k < nidx; k += (int)gridDim.x) {
        const int b = sh.idx[k], leq_rows = sh.leq_rows[b], eq_rows = sh.eq_rows[b];
        const int rows_max = leq_rows + 2 * eq_rows;
        const HsHbmTab tb = hs_hbm_tab(leq_rows, eq_rows, cols, nfree_cap);
        const SixVcHbmSlot sl = six_vc_hbm_slot(leq_rows, eq_rows, cols, nfree_cap, tb.Rmax, tb.ld);
        if (leq_rows <= 0 || eq_rows < 0 || eq_rows > (int)SIX_VC_MAX_EQ || tb.Rmax > Rmax || tb.ld > ld ||
            hbm_side_bytes<S>(rows_max, n) > (size_t)lds_bytes || hbm_side_bytes<S>(n, rows_max) > (size_t)lds_bytes ||
            sl.cells > (size_t)tg_cell) {
            if (tid == 0) hs_store(b, XPG_ERR_UNSUPPORTED, XPG_ERR_UNSUPPORTED, XPG_HS_NOT_RUN, out_has, out_status);
            continue;
        }
        S * const L = slot + sl.L; S * const E = slot + sl.E; int * const rest = (int *)(slot + sl.rest);
        S * const N = slot + sl.N; S * const obj = slot + sl.obj; S * const y = slot + sl.y; S * const vout = slot + sl.v;
        S * const tab = slot + sl.tab;
        vc_stage<S>(tid, nt, leq + sh.leq_off[b], leq_rows * cols, eqs + sh.eq_off[b], eq_rows * cols, 0, L, E);
        hs_objective<S>(L, leq_rows, E, eq_rows, cols, tg);
        const int nrest = vc_reshape<S>(L, leq_rows, cols, E, eq_rows, rest, hdr, tg, fv, nfree, obj, N);
        int has = 0, st[2] = {XPG_HS_NOT_RUN, XPG_HS_NOT_RUN};
        if (nrest < 0) {
            has = st[0] = XPG_ERR_REF_UNDEFINED;
        } else {
            const int rows = leq_rows + 2 * nrest;
            for (int pass = 0; pass < 2 && has == 0; pass++) {   // maxm, then minm of what that left open
                __syncthreads();                                 // pass 1 is through with the LDS block and the tableau
                st[pass] = six_vc_hbm_solve<S>((XPG_AS_LDS unsigned char *)lds, (XPG_AS_GLOBAL S *)tab, tb.ld, (XPG_AS_GLOBAL const S *)N,
                                               (XPG_AS_GLOBAL const S *)obj, rows, n, pass == 0 ? 1 : 0, max_iter, (XPG_AS_GLOBAL S *)y,
                                               (XPG_AS_GLOBAL S *)vout).status;
                has = hs_verdict(st[pass], is_unique != 0);
            }
        }
        if (tid == 0) hs_store(b, has, st[0], st[1], out_has, out_status);
    }
}

// What xpg_has_solution_batch_* ask of their arguments: has_solution()'s shape rule, and the arrays the rows need.
inline bool hs_args_ok(const xpg_ctx * ctx, int nb, const void * leq, int leq_rows, const void * eqs, int eq_rows, const void * vc, int vc_rows,
                       int cols, int rhs, const void * out_has)
{
    return ctx && nb >= 0 && vc && cols >= 2 && rhs == cols - 1 && vc_rows == rhs && leq_rows >= 0 && eq_rows >= 0 &&
           !(leq_rows > 0 && !leq) && !(eq_rows > 0 && !eqs) && out_has;
}

// The launch for a plan on route 0 or 1; every pointer is a device pointer. nfree_cap: the free variables the plan was sized for.
template <class S>
int hs_launch(xpg_ctx * ctx, HsPlan g, int nfree_cap, int nb, const S * vc, const S * eqs, int eq_rows, const S * leq, int leq_rows, int cols,
              bool is_unique, unsigned max_iter, int32_t * out_has, int32_t * out_status)
{
    const int grid_cap = XPG_INT_HOOK("XPG_HS_GRID");            // tests: the grid-stride path at small nb
    if (grid_cap > 0 && g.grid > grid_cap) { g.grid = grid_cap; g.scratch = (size_t)g.grid * g.slot; }
    if (g.route == HS_ROUTE_LDS) {
        Scratch & slots = ctx->scratch[SCRATCH_SIX_VC];
        if (const int rc = scratch_reserve(ctx, slots, g.scratch, g.scratch, "hipMalloc(has_solution_batch scratch)")) return rc;
        XPG_HIP(ctx, lds_limit((const void *)k_has_solution_batch<S>, ctx->device, g.lds));
        hipLaunchKernelGGL((k_has_solution_batch<S>), dim3((unsigned)g.grid), dim3((unsigned)g.threads), g.lds, ctx->stream, nb, vc, eqs, eq_rows, leq,
                           leq_rows, cols, is_unique ? 1 : 0, max_iter, (unsigned)g.lds, (unsigned long long *)slots.buf,
                           (unsigned long long)(g.slot / 8), (unsigned long long)g.tg_cell, out_has, out_status);
    } else {
        Scratch & slots = ctx->scratch[SCRATCH_SIX_VC_HBM];
        if (const int rc = scratch_reserve(ctx, slots, g.scratch, g.scratch, "hipMalloc(has_solution_batch_hbm scratch)")) return rc;
        if (const int rc = hbm_static_lds_check(ctx, (const void *)k_has_solution_batch_hbm<S>, SIX_VC_HBM_LDS_STATIC,
                                                "k_has_solution_batch_hbm: static LDS above SIX_VC_HBM_LDS_STATIC"))
            return rc;
        XPG_HIP(ctx, lds_limit((const void *)k_has_solution_batch_hbm<S>, ctx->device, g.lds));
        hipLaunchKernelGGL((k_has_solution_batch_hbm<S>), dim3((unsigned)g.grid), dim3((unsigned)g.threads), g.lds, ctx->stream, nb, vc, eqs, eq_rows,
                           leq, leq_rows, cols, is_unique ? 1 : 0, max_iter, nfree_cap, g.Rmax, g.ld, (unsigned)g.lds,
                           (unsigned long long *)slots.buf, (unsigned long long)(g.slot / 8), out_has, out_status);
    }
    XPG_HIP(ctx, hipGetLastError());
    HsRoute & rt = hs_route();
    (g.route == HS_ROUTE_LDS ? rt.lds : rt.hbm) = nb; rt.grid = g.grid;
    return 0;
}

// Device arrays in and out, enqueue only (a scratch area that has to grow waits for the stream first). The host never sees
// vc: everything is sized for every variable free; is_int_sol is the host-array form's alone.
template <class S>
int has_solution_batch_dev(xpg_ctx * ctx, int nb, const S * leq, int leq_rows, const S * eqs, int eq_rows, const S * vc, int vc_rows, int cols,
                           int rhs, bool is_int, bool is_unique, unsigned max_iter, int32_t * out_has, int32_t * out_status)
{
    HsRoute & rt = hs_route();
    rt = HsRoute{0, 0, 0, -1, 0};
    if (!hs_args_ok(ctx, nb, leq, leq_rows, eqs, eq_rows, vc, vc_rows, cols, rhs, out_has) || is_int) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    if (leq_rows == 0) {
        const HsNoLeq e = hs_no_inequality(eq_rows);
        hipLaunchKernelGGL(k_hs_fill, dim3((unsigned)((nb + 255) / 256 < 1024 ? (nb + 255) / 256 : 1024)), dim3(256), 0, ctx->stream, nb, e.has, e.status0,
                           out_has, out_status);
        XPG_HIP(ctx, hipGetLastError());
        return 0;
    }
    const HsPlan g = hs_plan<S>(true, -1, leq_rows, eq_rows, cols, nb, ctx_cus(ctx));
    if (g.route == HS_ROUTE_OTHER) return XPG_ERR_UNSUPPORTED;
    return hs_launch<S>(ctx, g, cols - 1, nb, vc, eqs, eq_rows, leq, leq_rows, cols, is_unique, max_iter, out_has, out_status);
}

// Host arrays; synchronises once. single(b): has_solution() of system b (route 2, a function of another part of the library).
template <class S, class Single>
int has_solution_batch_host(xpg_ctx * ctx, int nb, const S * leq, int leq_rows, const S * eqs, int eq_rows, const S * vc, int vc_rows, int cols,
                            int rhs, bool is_unique, unsigned max_iter, int32_t * out_has, int32_t * out_status, Single single)
{
    HsRoute & rt = hs_route();
    rt = HsRoute{0, 0, 0, 0, 0};
    if (!hs_args_ok(ctx, nb, leq, leq_rows, eqs, eq_rows, vc, vc_rows, cols, rhs, out_has)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    if (leq_rows == 0) {
        const HsNoLeq e = hs_no_inequality(eq_rows);
        for (int b = 0; b < nb; b++) hs_store(b, e.has, e.status0, XPG_HS_NOT_RUN, out_has, out_status);
        return 0;
    }
    std::vector<int> fvar;
    const bool pattern = vc_sign_pattern(vc, vc_rows, cols, fvar);
    const int nfree = pattern ? (int)fvar.size() : 0;
    const HsPlan g = hs_plan<S>(pattern, nfree, leq_rows, eq_rows, cols, nb, ctx_cus(ctx));
    if (g.route == HS_ROUTE_OTHER) {                             // the statuses stay has_solution()'s own: XPG_HS_NOT_RUN here
        for (int b = 0; b < nb; b++) {
            const int has = single(b);
            if (has < 0 && has != XPG_ERR_REF_UNDEFINED) return has;
            hs_store(b, has, XPG_HS_NOT_RUN, XPG_HS_NOT_RUN, out_has, out_status);
            rt.host++;
        }
        return 0;
    }
    const size_t bl = (size_t)nb * leq_rows * cols * 8, be = (size_t)nb * eq_rows * cols * 8, bv = (size_t)vc_rows * cols * 8;
    DevBuf dl, de, dvc, dhas, dst;
    XPG_TRY(dl.alloc(ctx, bl)); XPG_TRY(de.alloc(ctx, be)); XPG_TRY(dvc.alloc(ctx, bv));
    XPG_TRY(dhas.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dst.alloc(ctx, (size_t)nb * 8));
    XPG_TRY(hipMemcpyAsync(dl.p, leq, bl, hipMemcpyHostToDevice, ctx->stream));
    if (eq_rows > 0) XPG_TRY(hipMemcpyAsync(de.p, eqs, be, hipMemcpyHostToDevice, ctx->stream));
    XPG_TRY(hipMemcpyAsync(dvc.p, vc, bv, hipMemcpyHostToDevice, ctx->stream));
    int rc = hs_launch<S>(ctx, g, nfree, nb, (const S *)dvc.p, (const S *)de.p, eq_rows, (const S *)dl.p, leq_rows, cols, is_unique, max_iter,
                          (int32_t *)dhas.p, (int32_t *)dst.p);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); rt = HsRoute{0, 0, 0, 0, 0}; return rc; }
    std::vector<int32_t> has((size_t)nb), st((size_t)nb * 2);       // staged, so a HIP call that fails leaves the caller's arrays untouched
    XPG_TRY(hipMemcpyAsync(has.data(), dhas.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(st.data(), dst.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < nb; b++) {
        hs_store(b, has[(size_t)b], st[2 * (size_t)b], st[2 * (size_t)b + 1], out_has, out_status);
        rt.second += st[2 * (size_t)b + 1] != XPG_HS_NOT_RUN;
    }
    return 0;
}

// is_int_sol = 1, host arrays: has_solution()'s two MIP walks for the whole batch -- walk(is_max, count, tgtf, eq, leq, status)
// is xpg_mip_batch_vc_hbm_rat32 with is_bin = 0 and no indicator -- maxm on all systems, minm on the compacted open ones.
template <class Walk>
int has_solution_batch_int(xpg_ctx * ctx, int nb, const R32 * leq, int leq_rows, const R32 * eqs, int eq_rows, const R32 * vc, int vc_rows,
                           int cols, int rhs, bool is_unique, int32_t * out_has, int32_t * out_status, Walk walk)
{
    HsRoute & rt = hs_route();
    rt = HsRoute{0, 0, 0, 0, 0};
    if (!hs_args_ok(ctx, nb, leq, leq_rows, eqs, eq_rows, vc, vc_rows, cols, rhs, out_has)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    if (leq_rows == 0) {
        const HsNoLeq e = hs_no_inequality(eq_rows);
        for (int b = 0; b < nb; b++) hs_store(b, e.has, e.status0, XPG_HS_NOT_RUN, out_has, out_status);
        return 0;
    }
    const size_t lc = (size_t)leq_rows * cols, ec = (size_t)eq_rows * cols;
    std::vector<R32> tg((size_t)nb * cols), cl, ce, ct;
    for (int b = 0; b < nb; b++) {
        const std::vector<R32> t = feasibility_objective(leq + b * lc, leq_rows, eq_rows ? eqs + b * ec : (const R32 *)0, eq_rows, cols, rhs);
        std::copy(t.begin(), t.end(), tg.begin() + (size_t)b * cols);
    }
    std::vector<int32_t> st((size_t)nb), st2;
    std::vector<int> open;
    if (const int rc = walk(1, nb, tg.data(), eqs, leq, st.data())) return rc;
    for (int b = 0; b < nb; b++) {
        hs_store(b, hs_verdict(st[(size_t)b], is_unique), st[(size_t)b], XPG_HS_NOT_RUN, out_has, out_status);
        if (out_has[b] == 0) open.push_back(b);
    }
    if (open.empty()) return 0;
    const int no = (int)open.size();
    cl.resize(no * lc); ce.resize(no * ec); ct.resize((size_t)no * cols); st2.resize((size_t)no);
    for (int t = 0; t < no; t++) {
        const size_t b = (size_t)open[(size_t)t];
        std::copy(leq + b * lc, leq + (b + 1) * lc, cl.begin() + t * lc);
        if (ec) std::copy(eqs + b * ec, eqs + (b + 1) * ec, ce.begin() + t * ec);
        std::copy(tg.begin() + b * cols, tg.begin() + (b + 1) * cols, ct.begin() + (size_t)t * cols);
    }
    if (const int rc = walk(0, no, ct.data(), ec ? ce.data() : (const R32 *)0, cl.data(), st2.data())) return rc;
    for (int t = 0; t < no; t++) {
        const int b = open[(size_t)t];
        hs_store(b, hs_verdict(st2[(size_t)t], is_unique), st[(size_t)b], st2[(size_t)t], out_has, out_status);
    }
    rt.second = no;
    return 0;
}

// ---- mixed shapes: the host half ------------------------------------------------------------------------------------------------
// What the calling thread's last xpg_has_solution_batch_ragged_rat32 call did (xpg_has_solution_batch_ragged_last_route):
// systems on the LDS-resident kernel / the device-memory kernel / answered per system, systems whose second solve ran, the grids
// of the two launches (0 without one), systems answered without a solve (no inequality).
struct HsRaggedRoute { long long lds, hbm, host, second, grid_lds, grid_hbm, no_solve; };
inline HsRaggedRoute & hs_ragged_route() { static thread_local HsRaggedRoute r = {0, 0, 0, 0, 0, 0, 0}; return r; }

enum { HS_ROUTE_NO_SOLVE = 3 };
// THE plan of a ragged call (the launches and xpg_test_has_solution_batch_ragged_plan both ask it). Every system is routed by
// hs_plan of its OWN shape -- inside a ragged call a system takes the route a uniform call of its shape takes -- and a launch is
// sized by the largest of what hs_plan gives its systems, size by size (never by the plan of the envelope shape: that may
// leave the route its systems are on). The grid follows hs_plan's rules on those maxima and the launch's count: every rule in
// them is a minimum of terms that fall as a size grows, so it is the smallest grid hs_plan gives a system for that count.
// idx: the systems of the launch by descending leq_rows + 2 eq_rows, ties by index (arrival: in the order given -- the A/B
// of tools/lab asks that through a test hook).
struct HsRaggedLaunch {
    int count, threads, Rmax, ld, grid;
    size_t lds, slot, tg_cell;
    std::vector<int32_t> idx;
};
struct HsRaggedPlan { std::vector<int32_t> route; HsRaggedLaunch at[2]; long long host, no_solve; };
template <class S>
inline HsRaggedPlan hs_ragged_plan(bool pattern, int nfree, int nb, const int32_t * leq_rows, const int32_t * eq_rows, int cols, int num_cus,
                                   bool arrival = false)
{
    HsRaggedPlan p;
    p.route.assign((size_t)nb, HS_ROUTE_OTHER);
    p.host = p.no_solve = 0;
    for (HsRaggedLaunch & q : p.at) { q.count = q.threads = q.Rmax = q.ld = q.grid = 0; q.lds = q.slot = q.tg_cell = 0; }
    std::map<std::pair<int, int>, HsPlan> seen;                  // a SCoP has a handful of shapes
    for (int b = 0; b < nb; b++) {
        if (leq_rows[b] == 0) { p.route[(size_t)b] = HS_ROUTE_NO_SOLVE; p.no_solve++; continue; }
        const std::pair<int, int> key(leq_rows[b], eq_rows[b]);
        auto it = seen.find(key);
        if (it == seen.end()) it = seen.emplace(key, hs_plan<S>(pattern, nfree, key.first, key.second, cols, 1, num_cus)).first;
        const HsPlan & g = it->second;
        p.route[(size_t)b] = g.route;
        if (g.route == HS_ROUTE_OTHER) { p.host++; continue; }
        HsRaggedLaunch & q = p.at[g.route];
        q.count++; q.idx.push_back(b);
        q.lds = std::max(q.lds, g.lds); q.slot = std::max(q.slot, g.slot); q.tg_cell = std::max(q.tg_cell, g.tg_cell);
        q.threads = std::max(q.threads, g.threads); q.Rmax = std::max(q.Rmax, g.Rmax); q.ld = std::max(q.ld, g.ld);
    }
    for (int r = 0; r < 2; r++) {
        HsRaggedLaunch & q = p.at[r];
        if (q.count == 0) continue;
        q.grid = r == HS_ROUTE_LDS ? (int)six_vc_grid(q.lds, q.count, q.slot) : six_vc_hbm_grid(true, q.lds, q.slot, q.count, num_cus);
        if (!arrival)
            std::stable_sort(q.idx.begin(), q.idx.end(), [&](int32_t x, int32_t y) {
                return leq_rows[x] + 2ll * eq_rows[x] > leq_rows[y] + 2ll * eq_rows[y];
            });
    }
    return p;
}

// The shape rule of the ragged call: hs_args_ok on the largest rows, the shape and offset arrays there, no negative entry.
inline bool hs_ragged_args_ok(const xpg_ctx * ctx, int nb, const void * leq, const int32_t * leq_rows, const long long * leq_off, const void * eqs,
                              const int32_t * eq_rows, const long long * eq_off, const void * vc, int vc_rows, int cols, int rhs,
                              const void * out_has)
{
    if (nb > 0 && (!leq_rows || !eq_rows || !leq_off)) return false;
    int lmax = 0, emax = 0;
    for (int b = 0; b < nb; b++) {
        if (leq_rows[b] < 0 || eq_rows[b] < 0 || leq_off[b] < 0) return false;
        if (eq_rows[b] > 0 && (!eq_off || eq_off[b] < 0)) return false;
        lmax = std::max(lmax, (int)leq_rows[b]); emax = std::max(emax, (int)eq_rows[b]);
    }
    return hs_args_ok(ctx, nb, leq, lmax, eqs, emax, vc, vc_rows, cols, rhs, out_has);
}

// The two launches of a ragged plan, enqueue only; every pointer is a device pointer, sh.idx the start of BOTH index lists
// (the LDS launch's, then the device-memory launch's).
template <class S>
int hs_ragged_launch(xpg_ctx * ctx, HsRaggedPlan & p, int nfree, HsRagged sh, const S * vc, const S * eqs, const S * leq, int cols, bool is_unique,
                     unsigned max_iter, int32_t * out_has, int32_t * out_status)
{
    const int grid_cap = XPG_INT_HOOK("XPG_HS_GRID");            // tests: the grid-stride path at small nb
    for (HsRaggedLaunch & q : p.at) if (grid_cap > 0 && q.grid > grid_cap) q.grid = grid_cap;
    if (const HsRaggedLaunch & q = p.at[HS_ROUTE_LDS]; q.count > 0) {
        Scratch & slots = ctx->scratch[SCRATCH_SIX_VC];
        const size_t need = (size_t)q.grid * q.slot;
        if (const int rc = scratch_reserve(ctx, slots, need, need, "hipMalloc(has_solution_batch_ragged scratch)")) return rc;
        XPG_HIP(ctx, lds_limit((const void *)k_has_solution_ragged<S>, ctx->device, q.lds));
        hipLaunchKernelGGL((k_has_solution_ragged<S>), dim3((unsigned)q.grid), dim3((unsigned)q.threads), q.lds, ctx->stream, q.count, sh, vc, eqs,
                           leq, cols, is_unique ? 1 : 0, max_iter, (unsigned)q.lds, (unsigned long long *)slots.buf,
                           (unsigned long long)(q.slot / 8), (unsigned long long)q.tg_cell, out_has, out_status);
        XPG_HIP(ctx, hipGetLastError());
    }
    if (const HsRaggedLaunch & q = p.at[HS_ROUTE_HBM]; q.count > 0) {
        Scratch & slots = ctx->scratch[SCRATCH_SIX_VC_HBM];
        const size_t need = (size_t)q.grid * q.slot;
        if (const int rc = scratch_reserve(ctx, slots, need, need, "hipMalloc(has_solution_batch_ragged_hbm scratch)")) return rc;
        if (const int rc = hbm_static_lds_check(ctx, (const void *)k_has_solution_ragged_hbm<S>, SIX_VC_HBM_LDS_STATIC,
                                                "k_has_solution_ragged_hbm: static LDS above SIX_VC_HBM_LDS_STATIC"))
            return rc;
        XPG_HIP(ctx, lds_limit((const void *)k_has_solution_ragged_hbm<S>, ctx->device, q.lds));
        HsRagged hb = sh;
        hb.idx = sh.idx + p.at[HS_ROUTE_LDS].count;
        hipLaunchKernelGGL((k_has_solution_ragged_hbm<S>), dim3((unsigned)q.grid), dim3((unsigned)q.threads), q.lds, ctx->stream, q.count, hb, vc,
                           eqs, leq, cols, is_unique ? 1 : 0, max_iter, nfree, q.Rmax, q.ld, (unsigned)q.lds, (unsigned long long *)slots.buf,
                           (unsigned long long)(q.slot / 8), (unsigned long long)q.tg_cell, out_has, out_status);
        XPG_HIP(ctx, hipGetLastError());
    }
    return 0;
}

// Host arrays; synchronises once. single(b): has_solution() of system b (route 2, a function of another part of the library).
// Order: the systems that need no launch are answered first (an error there returns with nothing enqueued); then the arrays go
// up as they lie -- leq, eq and vc one copy each, the shape, offset and index arrays as one block --, both launches are
// enqueued, the answers come down and the stream is waited for once. The caller's arrays are written at the very end.
template <class S, class Single>
int has_solution_ragged_host(xpg_ctx * ctx, int nb, const S * leq, const int32_t * leq_rows, const long long * leq_off, const S * eqs,
                             const int32_t * eq_rows, const long long * eq_off, const S * vc, int vc_rows, int cols, int rhs, bool is_unique,
                             unsigned max_iter, int32_t * out_has, int32_t * out_status, Single single)
{
    HsRaggedRoute & rt = hs_ragged_route();
    rt = HsRaggedRoute{0, 0, 0, 0, 0, 0, 0};
    if (!hs_ragged_args_ok(ctx, nb, leq, leq_rows, leq_off, eqs, eq_rows, eq_off, vc, vc_rows, cols, rhs, out_has)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    std::vector<int> fvar;
    const bool pattern = vc_sign_pattern(vc, vc_rows, cols, fvar);
    const int nfree = pattern ? (int)fvar.size() : 0;
    HsRaggedPlan p = hs_ragged_plan<S>(pattern, nfree, nb, leq_rows, eq_rows, cols, ctx_cus(ctx), XPG_INT_HOOK("XPG_HS_RAGGED_ARRIVAL") != 0);
    std::vector<int32_t> has((size_t)nb, 0), st((size_t)nb * 2, (int32_t)XPG_HS_NOT_RUN);
    for (int b = 0; b < nb; b++) {
        if (p.route[(size_t)b] == HS_ROUTE_NO_SOLVE) {
            const HsNoLeq e = hs_no_inequality(eq_rows[b]);
            hs_store(b, e.has, e.status0, XPG_HS_NOT_RUN, has.data(), st.data());
        } else if (p.route[(size_t)b] == HS_ROUTE_OTHER) {       // the statuses stay has_solution()'s own: XPG_HS_NOT_RUN here
            const int h = single(b);
            if (h < 0 && h != XPG_ERR_REF_UNDEFINED) return h;
            has[(size_t)b] = h;
        }
    }
    const HsRaggedLaunch & ql = p.at[HS_ROUTE_LDS]; const HsRaggedLaunch & qh = p.at[HS_ROUTE_HBM];
    if (ql.count + qh.count > 0) {
        size_t lcells = 0, ecells = 0;                           // the extent of the concatenated arrays
        for (int b = 0; b < nb; b++) {
            lcells = std::max(lcells, (size_t)leq_off[b] + (size_t)leq_rows[b] * cols);
            if (eq_rows[b] > 0) ecells = std::max(ecells, (size_t)eq_off[b] + (size_t)eq_rows[b] * cols);
        }
        // one block: leq_off [nb] | eq_off [nb] (8 bytes each) | leq_rows [nb] | eq_rows [nb] | idx [count + count] (4 bytes each)
        const size_t nidx = (size_t)ql.count + (size_t)qh.count, meta_bytes = (size_t)nb * 24 + nidx * 4;
        std::vector<long long> meta((meta_bytes + 7) / 8, 0);
        long long * const m_lo = meta.data(); long long * const m_eo = m_lo + nb;
        int32_t * const m_lr = (int32_t *)(m_eo + nb); int32_t * const m_er = m_lr + nb; int32_t * const m_idx = m_er + nb;
        for (int b = 0; b < nb; b++) {
            m_lo[b] = leq_off[b]; m_eo[b] = eq_rows[b] > 0 ? eq_off[b] : 0;
            m_lr[b] = leq_rows[b]; m_er[b] = eq_rows[b];
        }
        std::copy(ql.idx.begin(), ql.idx.end(), m_idx);
        std::copy(qh.idx.begin(), qh.idx.end(), m_idx + ql.count);
        const size_t bv = (size_t)vc_rows * cols * 8;
        DevBuf dl, de, dvc, dmeta, dhas, dst;
        XPG_TRY(dl.alloc(ctx, lcells * 8)); XPG_TRY(de.alloc(ctx, ecells * 8)); XPG_TRY(dvc.alloc(ctx, bv)); XPG_TRY(dmeta.alloc(ctx, meta.size() * 8));
        XPG_TRY(dhas.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dst.alloc(ctx, (size_t)nb * 8));
        XPG_TRY(hipMemcpyAsync(dl.p, leq, lcells * 8, hipMemcpyHostToDevice, ctx->stream));
        if (ecells > 0) XPG_TRY(hipMemcpyAsync(de.p, eqs, ecells * 8, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dvc.p, vc, bv, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dmeta.p, meta.data(), meta.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        const long long * const d_lo = (const long long *)dmeta.p;
        const int32_t * const d_lr = (const int32_t *)(d_lo + 2 * (size_t)nb);
        const HsRagged sh = { d_lr + 2 * (size_t)nb, d_lr, d_lr + nb, d_lo, d_lo + nb };
        const int rc = hs_ragged_launch<S>(ctx, p, nfree, sh, (const S *)dvc.p, (const S *)de.p, (const S *)dl.p, cols, is_unique, max_iter,
                                           (int32_t *)dhas.p, (int32_t *)dst.p);
        if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
        std::vector<int32_t> ghas((size_t)nb), gst((size_t)nb * 2);
        XPG_TRY(hipMemcpyAsync(ghas.data(), dhas.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipMemcpyAsync(gst.data(), dst.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        for (int b = 0; b < nb; b++)
            if (p.route[(size_t)b] == HS_ROUTE_LDS || p.route[(size_t)b] == HS_ROUTE_HBM) {
                hs_store(b, ghas[(size_t)b], gst[2 * (size_t)b], gst[2 * (size_t)b + 1], has.data(), st.data());
                rt.second += gst[2 * (size_t)b + 1] != XPG_HS_NOT_RUN;
            }
    }
    for (int b = 0; b < nb; b++) hs_store(b, has[(size_t)b], st[2 * (size_t)b], st[2 * (size_t)b + 1], out_has, out_status);
    rt.lds = ql.count; rt.hbm = qh.count; rt.host = p.host; rt.no_solve = p.no_solve; rt.grid_lds = ql.grid; rt.grid_hbm = qh.grid;
    return 0;
}

// is_int_sol = 1: the shape classes on the host, in order of first sight, each packed and handed to batch(rows of leq, rows
// of eq, count, leq, eq, has, status [count][2]) -- xpg_has_solution_batch_rat32 with is_int_sol = 1, has_solution_batch_int's
// composition unchanged. Fusing the integer walks of different shapes stays open.
template <class Batch>
int has_solution_ragged_int(xpg_ctx * ctx, int nb, const R32 * leq, const int32_t * leq_rows, const long long * leq_off, const R32 * eqs,
                            const int32_t * eq_rows, const long long * eq_off, const R32 * vc, int vc_rows, int cols, int rhs,
                            int32_t * out_has, int32_t * out_status, Batch batch)
{
    HsRaggedRoute & rt = hs_ragged_route();
    rt = HsRaggedRoute{0, 0, 0, 0, 0, 0, 0};
    if (!hs_ragged_args_ok(ctx, nb, leq, leq_rows, leq_off, eqs, eq_rows, eq_off, vc, vc_rows, cols, rhs, out_has)) return XPG_ERR_SHAPE;
    std::vector<std::pair<std::pair<int, int>, std::vector<int> > > groups;
    for (int b = 0; b < nb; b++) {
        const std::pair<int, int> key(leq_rows[b], eq_rows[b]);
        size_t g = 0;
        while (g < groups.size() && groups[g].first != key) g++;
        if (g == groups.size()) groups.push_back(std::make_pair(key, std::vector<int>()));
        groups[g].second.push_back(b);
    }
    std::vector<int32_t> has((size_t)nb, 0), st((size_t)nb * 2, (int32_t)XPG_HS_NOT_RUN);
    long long second = 0, no_solve = 0;
    for (const auto & grp : groups) {
        const int lr = grp.first.first, er = grp.first.second, n = (int)grp.second.size();
        const size_t lc = (size_t)lr * cols, ec = (size_t)er * cols;
        std::vector<R32> L((size_t)n * lc), E((size_t)n * ec);
        std::vector<int32_t> h((size_t)n, 0), s((size_t)n * 2, (int32_t)XPG_HS_NOT_RUN);
        for (int k = 0; k < n; k++) {
            const int b = grp.second[(size_t)k];
            if (lc) std::copy(leq + leq_off[b], leq + leq_off[b] + lc, L.begin() + (size_t)k * lc);
            if (ec) std::copy(eqs + eq_off[b], eqs + eq_off[b] + ec, E.begin() + (size_t)k * ec);
        }
        if (const int rc = batch(lr, er, n, lc ? L.data() : (const R32 *)0, ec ? E.data() : (const R32 *)0, h.data(), s.data())) return rc;
        for (int k = 0; k < n; k++) {
            const size_t b = (size_t)grp.second[(size_t)k];
            has[b] = h[(size_t)k]; st[2 * b] = s[2 * (size_t)k]; st[2 * b + 1] = s[2 * (size_t)k + 1];
            second += s[2 * (size_t)k + 1] != XPG_HS_NOT_RUN;
        }
        if (lr == 0) no_solve += n;
    }
    for (int b = 0; b < nb; b++) hs_store(b, has[(size_t)b], st[2 * (size_t)b], st[2 * (size_t)b + 1], out_has, out_status);
    rt.second = second; rt.no_solve = no_solve;
    return 0;
}

} // namespace xpg
