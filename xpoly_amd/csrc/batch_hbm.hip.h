// Batches of LPs whose slack form does NOT fit one CU's LDS (xpg_six_batch_hbm_*): the first refused fp64 shape of
// xpg_six_batch_* is about 100 inequalities x 100 variables, a deeper loop nest's dependence system. One workgroup still
// owns one LP from the caller's arrays to the answer, and every step of SIX::maxm / minm is the code of the LDS-resident
// kernel (batch_kernels.hip.h: sm_build, sm_phase_one_*, sm_solve's generic branch, sm_solve_lp, instantiated with
// HBM = true) -- only the tableau moves:
//   tableau   tab[R][ld] in a scratch slot in global memory that belongs to the WORKGROUP, not the LP (a workgroup walks its
//             LPs one after the other, as k_six_batch_vc's do): slots start on 256-byte lines, the scratch of a launch is
//             grid x slot whatever nb is, and the grid is cut so that it stays under BATCH_HBM_SCRATCH_MAX. ld = the widest
//             live width (V + R + 2, stage 1's auxiliary column included) rounded up to an even number of cells: every row
//             starts 16-byte aligned and a pair of adjacent columns is one 16-byte access.
//   LDS       everything else, by a carve of its own (hbm_carve): obj, e, x, k, the constant column's mirror, the basis
//             maps, rowcnt / colcnt, the pivot-pair table, the reduction scratch. A 100 x 100 LP: 15 KB.
//   pivot     sm_pivot_hbm below: the sweep in 16-byte loads and stores, a thread owning two adjacent columns with their e_j
//             in registers, k_i an LDS broadcast, four rows in flight per thread. The constant column is mirrored in LDS
//             (P.bcol) by whoever writes it, so the ratio test walks only the entering column at row stride.
// A workgroup only ever reads its own slot: __syncthreads() orders everything, there is no cross-workgroup traffic.
// The arithmetic per cell is sm_pivot's (multiply, then add; the q_scaled shortcuts; the q_* forms under P.cn), so status,
// optimum and solution are bit for bit those of the LDS kernel and of the single-problem entry points.
#pragma once
#include "batch_kernels.hip.h"

namespace xpg {

// Which route the LPs of the calling thread's last xpg_six_batch_hbm_* call took (xpg_six_batch_hbm_last_route).
struct BatchHbmRoute { long long lds, hbm, grid; };
inline BatchHbmRoute & batch_hbm_route() { static thread_local BatchHbmRoute r = {0, 0, 0}; return r; }

#define BATCH_HBM_SCRATCH_MAX ((size_t)256 << 20)
// Threads per workgroup, and wavefronts resident per CU (the kernel's registers allow 16: __launch_bounds__(1024)), which
// with the threads gives the workgroups -- LPs in flight -- per CU. The starting point, to be settled by
// tools/lab/run_batch_hbm_ab.sh (XPG_BATCH_HBM_THREADS / XPG_BATCH_HBM_WAVES on the hooks build select the variants).
enum { BATCH_HBM_THREADS = 256, BATCH_HBM_WAVES_PER_CU = 16 };
enum { HBM_ROUTE_LDS = 0, HBM_ROUTE_HBM = 1, HBM_ROUTE_REFUSED = 2 };

// The LDS of one LP on the HBM route: every array of small_lds_bytes but the tableau, the three rows padded to 16-byte
// multiples (the sweep reads e_j in pairs), and the mirror of the constant column.
template <class S> __host__ __device__ inline size_t hbm_side_bytes(int R, int V)
{
    const size_t Wmax = (size_t)V + 1 + (size_t)R + 1, nmax = Wmax - 1, pw = (nmax + 31) / 32;
    size_t b = ((Wmax + 1) & ~(size_t)1) * 8 * 3;             // obj, e, x
    b += (((size_t)R + 1) & ~(size_t)1) * 8 * 2;              // k, bcol
    b += 16 * sizeof(Cand<S>);                                // sh_c
    b += nmax * 4 * 3;                                        // bv2eq, rowcnt, colcnt
    b += (size_t)R * 4;                                       // eq2bv
    b += nmax * pw * 4;                                       // ppt
    b += 16 * 4 + 8 * 4;                                      // sh_i, sh_w
    b += ((nmax + 3) & ~(size_t)3) * 2;                       // nv, bv
    return (b + 15) & ~(size_t)15;
}
template <class S> __device__ __forceinline__ void hbm_carve(Small<S> & P, unsigned char * lds, S * slot, int R, int V, int ld)
{
    const int Wmax = V + 1 + R + 1, nmax = Wmax - 1;
    const size_t row = (size_t)((Wmax + 1) & ~1) * 8, col = (size_t)((R + 1) & ~1) * 8;
    unsigned char * p = lds;
    P.tab = slot;
    P.obj = (S *)p; p += row;
    P.e = (S *)p; p += row;
    P.x = (S *)p; p += row;
    P.k = (S *)p; p += col;
    P.bcol = (S *)p; p += col;
    P.sh_c = (Cand<S> *)p; p += 16 * sizeof(Cand<S>);
    P.bv2eq = (int *)p; p += (size_t)nmax * 4;
    P.rowcnt = (int *)p; p += (size_t)nmax * 4;
    P.colcnt = (int *)p; p += (size_t)nmax * 4;
    P.eq2bv = (int *)p; p += (size_t)R * 4;
    P.pw = (nmax + 31) / 32;
    P.ppt = (uint32_t *)p; p += (size_t)nmax * P.pw * 4;
    P.sh_i = (int *)p; p += 16 * 4;
    P.sh_w = (int *)p; p += 8 * 4;
    P.nv = (uint8_t *)p; p += (size_t)((nmax + 3) & ~3);
    P.bv = (uint8_t *)p;
    P.ld = ld;
}

// Address spaces of the pointers that cross a __noinline__ call boundary (six_batch_vc_hbm.hip.h, mip_tree_hbm.hip.h): behind
// it the side arrays stay ds_* and the tableau global_* accesses (through generic pointers both became flat_*).
#define XPG_AS_LDS __attribute__((address_space(3)))
#define XPG_AS_GLOBAL __attribute__((address_space(1)))

// The rules every route on a tableau in device memory shares (k_batch_hbm, k_six_batch_vc_hbm, k_mip_tree_hbm).
// ld: the widest live width (V + R + 2) rounded up to an even number of cells; a tableau slot starts on a 256-byte line.
__host__ __device__ inline size_t hbm_ld(int R, int V) { return ((size_t)V + (size_t)R + 2 + 1) & ~(size_t)1; }
inline size_t hbm_slot_bytes(int R, size_t ld) { return ((size_t)R * ld * 8 + 255) & ~(size_t)255; }
// The grid: workgroups per CU by the wavefronts resident there, cut by what 160 KB of LDS hold (lds: dynamic plus static
// bytes of one workgroup), at least one; times the CUs, cut by the workgroups whose scratch (each bytes) fits
// scratch_max and by nb, at least one.
inline long long hbm_grid(int num_cus, int threads, int waves_per_cu, size_t lds, size_t each, size_t scratch_max, int nb)
{
    long long per_cu = waves_per_cu * 64 / threads;
    const long long by_lds = (long long)(((size_t)160 * 1024) / lds);
    if (per_cu > by_lds) per_cu = by_lds;
    if (per_cu < 1) per_cu = 1;
    long long grid = (long long)num_cus * per_cu;
    const long long by_scratch = (long long)(scratch_max / each);
    if (grid > by_scratch) grid = by_scratch;
    if (grid > nb) grid = nb;
    if (grid < 1) grid = 1;
    return grid;
}
// What the code object of `kernel` really holds in static LDS against the figure its plan counted: a __shared__ array
// added anywhere below the kernel is a clean error before the launch, not a plan that over-admits at the 160 KB edge.
inline int hbm_static_lds_check(xpg_ctx * ctx, const void * kernel, size_t counted, const char * what)
{
    static std::mutex mu;
    static std::map<const void *, size_t> held;
    std::lock_guard<std::mutex> g(mu);
    auto it = held.find(kernel);
    if (it == held.end()) {
        hipFuncAttributes fa;
        it = held.emplace(kernel, hipFuncGetAttributes(&fa, kernel) == hipSuccess ? (size_t)fa.sharedSizeBytes : (size_t)0).first;
    }
    if (it->second > counted) { ctx->err = what; return XPG_ERR_UNSUPPORTED; }
    return 0;
}

// THE rule (the launch and xpg_test_batch_hbm_geometry both ask it): an LP that fits one CU's LDS takes k_batch exactly as
// xpg_six_batch_* launches it; otherwise k_batch_hbm, as long as the side arrays fit 160 KB beside the kernel's static LDS
// and one slot fits the scratch cap; anything else is refused before any launch.
struct HbmGeom {
    int route;              // HBM_ROUTE_*
    size_t lds;             // route 0: small_lds_bytes; else hbm_side_bytes
    size_t slot;            // bytes of one workgroup's tableau slot (0 on route 0)
    int ld, threads, grid;
    size_t scratch;         // grid x slot
};
template <class S> inline HbmGeom batch_hbm_geometry(int R, int V, int nb, int num_cus, int threads = 0, int waves_per_cu = 0)
{
    HbmGeom g;
    if (small_lds_fits<S>(R, V)) {
        const BatchGeom b = batch_geometry<S>(R, V, nb, num_cus);
        g.route = HBM_ROUTE_LDS; g.lds = b.lds; g.slot = 0; g.ld = V + R + 2; g.threads = b.threads; g.grid = b.grid; g.scratch = 0;
        return g;
    }
    const size_t ld = hbm_ld(R, V);
    g.lds = hbm_side_bytes<S>(R, V);
    g.slot = hbm_slot_bytes(R, ld);
    g.ld = (int)ld;
    g.threads = threads > 0 ? threads : BATCH_HBM_THREADS;
    if (g.lds + SMALL_LDS_STATIC > (size_t)160 * 1024 || g.slot > BATCH_HBM_SCRATCH_MAX) {
        g.route = HBM_ROUTE_REFUSED; g.grid = 0; g.scratch = 0;
        return g;
    }
    g.route = HBM_ROUTE_HBM;
    g.grid = (int)hbm_grid(num_cus, g.threads, waves_per_cu > 0 ? waves_per_cu : BATCH_HBM_WAVES_PER_CU, g.lds + SMALL_LDS_STATIC, g.slot,
                           BATCH_HBM_SCRATCH_MAX, nb);
    g.scratch = (size_t)g.grid * g.slot;
    return g;
}

// SIX::pivot (lpsol.h:1456-1511) on a tableau in global memory; all threads participate. sm_pivot's arithmetic cell by cell.
template <class S> struct alignas(16) Cell2 { S a, b; };
template <class S> __device__ __forceinline__ void sm_pivot_hbm(Small<S> & P, int nv, int bv)
{
    const int tid = (int)threadIdx.x, nt = (int)blockDim.x;
    const int r = P.bv2eq[bv], W = P.W, ld = P.ld, R = P.R, rhs = P.rhs;
    S * const tab = P.tab;
    const S piv = tab[r * ld + nv];
    const S cnv = P.obj[nv];
    __syncthreads();
    const S s = q_div(P.cn, one<S>(), piv);
    const int smode = scale_mode(s), cmode = scale_mode(cnv);
    // staging writes LDS only: the scaled pivot row -> e, the objective row, -column -> k (k_r = 0: the sweep puts e there)
    for (int j = tid; j < W; j += nt) {
        const S ej = q_scaled(P.cn, tab[r * ld + j], s, smode);
        P.e[j] = ej;
        S t = q_mul(P.cn, ej, minus_one<S>());
        if (j >= rhs) t = neg(t);
        t = q_scaled(P.cn, t, cnv, cmode);
        P.obj[j] = q_add(P.cn, t, P.obj[j]);
    }
    for (int i = tid; i < R; i += nt) P.k[i] = i != r ? neg(tab[i * ld + nv]) : zero<S>();
    __syncthreads();
    // sweep: NP column pairs; a thread owns a pair (both e_j in registers), groups of cw threads take alternate rows,
    // consecutive threads touch consecutive 16-byte cells of a row. Four rows are loaded before the first is used. The last
    // pair of an odd width holds one live column: its other cell (padding, or a column stage 1 has dropped) is stored back
    // as it was read and never interpreted.
    {
        const int NP = (W + 1) >> 1, ld2 = ld >> 1;
        const int cw = NP < nt ? NP : nt, ny = nt / cw, tx = tid % cw, ty = tid / cw;
        const bool cn = P.cn;
        if (ty < ny)
            for (int p = tx; p < NP; p += cw) {
                const int j = 2 * p;
                const bool two = j + 1 < W;
                const S e0 = P.e[j], e1 = two ? P.e[j + 1] : zero<S>();
                const int mirror = j == rhs ? 0 : (two && j + 1 == rhs ? 1 : -1);
                Cell2<S> * const col = (Cell2<S> *)tab + p;
                auto put = [&](int i, const Cell2<S> & c, S k) {
                    Cell2<S> o;
                    o.a = i == r ? e0 : q_fma(cn, c.a, k, e0);
                    if (two) o.b = i == r ? e1 : q_fma(cn, c.b, k, e1);
                    else o.b = c.b;
                    col[i * ld2] = o;
                    if (mirror >= 0) P.bcol[i] = mirror ? o.b : o.a;
                };
                int i = ty;
                for (; i + 3 * ny < R; i += 4 * ny) {
                    const int i1 = i + ny, i2 = i + 2 * ny, i3 = i + 3 * ny;
                    const Cell2<S> c0 = col[i * ld2], c1 = col[i1 * ld2], c2 = col[i2 * ld2], c3 = col[i3 * ld2];
                    const S k0 = P.k[i], k1 = P.k[i1], k2 = P.k[i2], k3 = P.k[i3];
                    put(i, c0, k0); put(i1, c1, k1); put(i2, c2, k2); put(i3, c3, k3);
                }
                for (; i < R; i += ny) { const Cell2<S> c = col[i * ld2]; put(i, c, P.k[i]); }
            }
    }
    if (tid == 0) {
        P.nv[nv] = 0; P.nv[bv] = 1; P.bv[nv] = 1; P.bv[bv] = 0;
        P.eq2bv[r] = nv; P.bv2eq[nv] = r; P.bv2eq[bv] = -1;
        XPG_TRACE_PIVOT("hbm", nv, bv, r);
    }
    P.pivots++;
    __syncthreads();
}

// One workgroup per LP, grid-stride over the batch; the workgroup's tableau slot is reused from LP to LP (sm_build writes
// every live cell before anything reads it).
template <class S> __global__ __launch_bounds__(1024)
void k_batch_hbm(int nb, const S * tgtf, const S * leq, int m, int cols, int is_max, unsigned max_iter,
                 unsigned long long * slots, unsigned long long slot_cells, int ld,
                 int32_t * out_status, S * out_v, S * out_sol, uint32_t * out_pivots)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int n = cols - 1;
    Small<S> P;
    hbm_carve(P, lds, (S *)(slots + (size_t)blockIdx.x * slot_cells), is_max ? m : n, is_max ? n : m, ld);
    for (int lp = (int)blockIdx.x; lp < nb; lp += (int)gridDim.x) {
        __syncthreads();                                         // the LP before is through with the LDS block and the slot
        Source<S> src;
        src.leq = leq + (size_t)lp * m * cols; src.tgtf = tgtf + (size_t)lp * cols;
        src.m = m; src.cols = cols; src.is_max = is_max;
        const int status = sm_solve_lp<S, true>(P, src, max_iter, 0, out_sol + (size_t)lp * cols, out_v + lp);
        if (threadIdx.x == 0) {
            out_status[lp] = status;
            if (out_pivots) out_pivots[lp] = P.pivots;
        }
    }
}

// Device arrays in and out, enqueue only (a scratch area that has to grow waits for the stream first).
template <class S>
int batch_hbm_dev(xpg_ctx * ctx, int is_max, int nb, const S * tgtf, const S * leq, int m, int cols, unsigned max_iter,
                  int32_t * out_status, S * out_v, S * out_sol, uint32_t * out_pivots)
{
    BatchHbmRoute & rt = batch_hbm_route();
    rt = BatchHbmRoute{0, 0, 0};
    if (!ctx || nb < 0 || !tgtf || !leq || m <= 0 || cols < 2 || !out_status || !out_v || !out_sol)
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const int n = cols - 1;
    const int R = is_max ? m : n, V = is_max ? n : m;
    const int threads_hook = XPG_INT_HOOK("XPG_BATCH_HBM_THREADS"), waves_hook = XPG_INT_HOOK("XPG_BATCH_HBM_WAVES");   // A/B runs (tools/lab)
    const int grid_cap = XPG_INT_HOOK("XPG_BATCH_HBM_GRID");
    const int threads = threads_hook >= 64 && threads_hook <= 1024 && threads_hook % 64 == 0 ? threads_hook : 0;
    HbmGeom g = batch_hbm_geometry<S>(R, V, nb, ctx_cus(ctx), threads, waves_hook);
    if (g.route == HBM_ROUTE_REFUSED) return XPG_ERR_UNSUPPORTED;
    if (g.route == HBM_ROUTE_LDS) {
        const int rc = batch_dev<S>(ctx, is_max, nb, tgtf, leq, m, cols, max_iter, out_status, out_v, out_sol, out_pivots, 0);
        if (rc == 0) rt = BatchHbmRoute{nb, 0, g.grid};
        return rc;
    }
    if (grid_cap > 0 && g.grid > grid_cap) { g.grid = grid_cap; g.scratch = (size_t)g.grid * g.slot; }
    Scratch & slots = ctx->scratch[SCRATCH_BATCH_HBM];
    if (const int rc = scratch_reserve(ctx, slots, g.scratch, g.scratch, "hipMalloc(six_batch_hbm scratch)")) return rc;
    if (const int rc = hbm_static_lds_check(ctx, (const void *)k_batch_hbm<S>, SMALL_LDS_STATIC, "k_batch_hbm: static LDS above SMALL_LDS_STATIC")) return rc;
    XPG_HIP(ctx, lds_limit((const void *)k_batch_hbm<S>, ctx->device, g.lds));
    hipLaunchKernelGGL((k_batch_hbm<S>), dim3((unsigned)g.grid), dim3((unsigned)g.threads), g.lds, ctx->stream, nb, tgtf, leq, m, cols,
                       is_max ? 1 : 0, max_iter, (unsigned long long *)slots.buf, (unsigned long long)(g.slot / 8), g.ld,
                       out_status, out_v, out_sol, out_pivots);
    XPG_HIP(ctx, hipGetLastError());
    rt = BatchHbmRoute{0, nb, g.grid};
    return 0;
}

// Host arrays; synchronises once. An LP that fits LDS goes through batch_host, the call xpg_six_batch_* makes.
template <class S>
int batch_hbm_host(xpg_ctx * ctx, int is_max, int nb, const S * tgtf, const S * leq, int m, int cols, unsigned max_iter,
                   int32_t * out_status, S * out_v, S * out_sol)
{
    BatchHbmRoute & rt = batch_hbm_route();
    rt = BatchHbmRoute{0, 0, 0};
    if (!ctx || nb < 0 || !tgtf || !leq || m <= 0 || cols < 2 || !out_status || !out_v || !out_sol)
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const int n = cols - 1;
    const int R = is_max ? m : n, V = is_max ? n : m;
    const HbmGeom g = batch_hbm_geometry<S>(R, V, nb, ctx_cus(ctx));
    if (g.route == HBM_ROUTE_REFUSED) return XPG_ERR_UNSUPPORTED;
    if (g.route == HBM_ROUTE_LDS) {
        const int rc = batch_host<S>(ctx, is_max, nb, tgtf, leq, m, cols, max_iter, out_status, out_v, out_sol);
        if (rc == 0) rt = BatchHbmRoute{nb, 0, g.grid};
        return rc;
    }
    BatchIo io;
    if (const int rc = io.up(ctx, nb, tgtf, nullptr, nullptr, 0, leq, m, cols)) return rc;
    const int rc = batch_hbm_dev<S>(ctx, is_max, nb, (const S *)io.dt.p, (const S *)io.dl.p, m, cols, max_iter, (int32_t *)io.dst.p, (S *)io.dv.p,
                                    (S *)io.ds.p, nullptr);
    if (rc) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    return io.down(ctx, nb, cols, out_status, out_v, out_sol);
}

} // namespace xpg
