// C ABI of libxpoly_amd.so (include/xpoly_amd.h), the core: handle, K1 pivot, the device-resident LP (every loop of
// lp_*.hip.h), warm-started MIP, test and debug hooks. One of the library's eight sources (build.py).
#include <new>
#include "scalar.hip.h"
#include "ctx.hip.h"
#include "lp_kernels.hip.h"
#include "lp_pipe_r32.hip.h"
#include "lp_fused_r32.hip.h"
#include "lp_host.hip.h"
#include "warm_mip.hip.h"
#include "warm_mip_batch.hip.h"

using namespace xpg;

struct xpg_lp { LpBase * impl; };

extern "C" {

const char * xpg_version(void) { return "xpoly_amd 0.1 (gfx950)"; }

int xpg_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int xpg_create(xpg_ctx ** out, int device)
{
    if (!out) return XPG_ERR_SHAPE;
    *out = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n)
        return XPG_ERR_NO_DEVICE;
    xpg::DeviceGuard bind(device);
    xpg_ctx * c = new (std::nothrow) xpg_ctx();
    if (!c) return XPG_ERR_ALLOC;
    c->device = device;
    c->rowbuf = c->colbuf = 0; c->st = 0; c->row_cap = c->col_cap = 0;
    c->stage = 0; c->stage_cap = 0;
    c->hstage = 0; c->hstage_cap = 0;
    // XPG_LOOP: "block" / "pipe" force the blocked / the pipelined loop whatever the size (unset: chosen by size; a value
    // beginning with 's', once the names of loops the product never ran, reads as unset)
    const char * lm = xpg_env("XPG_LOOP");
    if (lm && lm[0] == 's') lm = nullptr;
    c->loop_mode = lm && lm[0] == 'b' ? 3 : 0;          // "block": B pivots per sweep (lp_blocked.hip.h), else pipelined
    const char * ch = xpg_env("XPG_CHAIN");               // "0": launch-per-stage chain, for A/B runs
    c->chain = ch ? atoi(ch) : 1;
    const char * cx = xpg_hook("XPG_CHAIN_XCD");
    c->chain_local = cx ? (atoi(cx) != 0 ? 1 : 0) : 1;
    const char * cf = xpg_hook("XPG_CHAIN_FOLD");
    c->chain_fold = cf ? (atoi(cf) != 0 ? 1 : 0) : 1;
    const char * cta = xpg_hook("XPG_CHAIN_TEST_ABORT");
    c->chain_test_abort = cta ? atoi(cta) : 0;
    c->num_cus = 0;
    if (hipDeviceGetAttribute(&c->num_cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) c->num_cus = 0;
    c->loop_auto = lm ? 0 : 1;                         // unset: blocked loop for large fp64 tableaux, else pipelined
    const char * bl = xpg_env("XPG_BLOCK");
    c->block_len = bl ? atoi(bl) : BLK_DEFAULT;
    if (c->block_len < 1) c->block_len = 1;
    if (c->block_len > BLK_MAX) c->block_len = BLK_MAX;
    c->prof_cap = 0; c->prof_n = 0; c->prof_stride = 1; c->prof_seen = 0;
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return XPG_ERR_HIP; }
    if (hipMalloc((void **)&c->st, sizeof(LoopState)) != hipSuccess) { (void)hipStreamDestroy(c->stream); delete c; return XPG_ERR_ALLOC; }
    *out = c;
    return 0;
}

void xpg_destroy(xpg_ctx * ctx)
{
    if (!ctx) return;
    XPG_BIND(ctx);
    (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : ctx->ev0) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev1) (void)hipEventDestroy(e);
    if (ctx->rowbuf) (void)hipFree(ctx->rowbuf);
    if (ctx->colbuf) (void)hipFree(ctx->colbuf);
    if (ctx->st) (void)hipFree(ctx->st);
    if (ctx->stage) (void)hipFree(ctx->stage);
    if (ctx->hstage) (void)hipHostFree(ctx->hstage);
    if (ctx->hpack) (void)hipHostFree(ctx->hpack);
    if (ctx->hred) (void)hipHostFree(ctx->hred);
    if (ctx->slice_buf) (void)hipFree(ctx->slice_buf);
    for (Scratch & s : ctx->scratch) s.release();
    for (xpg_ctx * l : ctx->lanes) xpg_destroy(l);
    ctx->lanes.clear();
    for (auto & b : ctx->dev_cache) (void)hipFree(b.first);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int xpg_profile_begin(xpg_ctx * ctx, int cap, int stride)
{
    XPG_BIND(ctx);
    if (!ctx || cap < 0 || stride < 1) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    while ((int)ctx->ev0.size() < cap) {
        hipEvent_t a, b;
        XPG_HIP(ctx, hipEventCreate(&a));
        XPG_HIP(ctx, hipEventCreate(&b));
        ctx->ev0.push_back(a); ctx->ev1.push_back(b);
    }
    ctx->prof_cap = cap; ctx->prof_n = 0; ctx->prof_stride = stride; ctx->prof_seen = 0;
    return 0;
}

int xpg_profile_end(xpg_ctx * ctx, int * launches, double * total_ms)
{
    XPG_BIND(ctx);
    if (!ctx) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    double sum = 0.0;
    for (int i = 0; i < ctx->prof_n; i++) {
        float ms = 0.f;
        XPG_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0[i], ctx->ev1[i]));
        sum += ms;
    }
    if (launches) *launches = ctx->prof_n;
    if (total_ms) *total_ms = sum;
    ctx->prof_cap = 0; ctx->prof_n = 0;
    return 0;
}

const char * xpg_last_error(const xpg_ctx * ctx) { return ctx ? ctx->err.c_str() : "null context"; }
void * xpg_stream(const xpg_ctx * ctx) { return ctx ? (void *)ctx->stream : 0; }

int xpg_sync(xpg_ctx * ctx)
{
    XPG_BIND(ctx);
    if (!ctx) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int xpg_malloc(xpg_ctx * ctx, void ** dptr, size_t bytes)
{
    XPG_BIND(ctx);
    if (!ctx || !dptr) return XPG_ERR_SHAPE;
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 8);
    if (e != hipSuccess) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return XPG_ERR_ALLOC; }
    return 0;
}
int xpg_free(xpg_ctx * ctx, void * dptr)
{
    XPG_BIND(ctx);
    if (!ctx) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipFree(dptr));
    return 0;
}
int xpg_upload(xpg_ctx * ctx, void * dst_dev, const void * src_host, size_t bytes)
{
    XPG_BIND(ctx);
    if (!ctx) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int xpg_download(xpg_ctx * ctx, void * dst_host, const void * src_dev, size_t bytes)
{
    XPG_BIND(ctx);
    if (!ctx) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

} // extern "C"

// ---- K1 on caller-owned device tableaux --------------------------------------------
namespace {

int ensure_scratch(xpg_ctx * ctx, int m, int W)
{
    const size_t rb = (size_t)round_up(W, 16) * 8, cb = (size_t)round_up(m, 16) * 8;
    if (rb > ctx->row_cap) {
        if (ctx->rowbuf) XPG_HIP(ctx, hipFree(ctx->rowbuf));
        ctx->rowbuf = 0; ctx->row_cap = 0;
        if (hipMalloc(&ctx->rowbuf, rb) != hipSuccess) { ctx->err = "hipMalloc(rowbuf)"; return XPG_ERR_ALLOC; }
        ctx->row_cap = rb;
    }
    if (cb > ctx->col_cap) {
        if (ctx->colbuf) XPG_HIP(ctx, hipFree(ctx->colbuf));
        ctx->colbuf = 0; ctx->col_cap = 0;
        if (hipMalloc(&ctx->colbuf, cb) != hipSuccess) { ctx->err = "hipMalloc(colbuf)"; return XPG_ERR_ALLOC; }
        ctx->col_cap = cb;
    }
    return 0;
}

template <class S> __global__ void k_stage_pivot(LpView<S> v, int row, int col)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    LoopState * st = v.st;
    st->status = ST_RUNNING; st->row = row; st->col = col; st->leave = 0;
    st->cnv_bits = to_bits(v.obj[col]);
    st->piv_bits = to_bits(v.tab[(size_t)row * v.ld + col]);
}

template <class S>
int pivot_dev(xpg_ctx * ctx, S * tab, int m, int W, int ld, S * obj, int rhs, int row, int col)
{
    if (!ctx || !tab || !obj || m <= 0 || W <= 1 || ld < W || row < 0 || row >= m || col < 0 ||
        col >= W || rhs < 0 || rhs >= W)
        return XPG_ERR_SHAPE;
    // the fp64 sweep uses 16-byte accesses: rows must start 16-byte aligned
    if (is_f64<S>::value && ((ld & 1) || ((uintptr_t)tab & 15))) return XPG_ERR_SHAPE;
    int rc = ensure_scratch(ctx, m, W);
    if (rc) return rc;
    LpView<S> v;
    memset(&v, 0, sizeof(v));
    v.tab = tab; v.m = m; v.W = W; v.ld = ld; v.rhs = rhs; v.obj = obj;
    v.rowbuf = (S *)ctx->rowbuf; v.colbuf = (S *)ctx->colbuf; v.st = ctx->st;
    hipLaunchKernelGGL((k_stage_pivot<S>), dim3(1), dim3(64), 0, ctx->stream, v, row, col);
    const int span = W > m ? W : m;
    hipLaunchKernelGGL((k_prep<S>), dim3((span + 255) / 256), dim3(256), 0, ctx->stream, v, 0, 0, 0);
    launch_update<S>(ctx, v, 0);
    XPG_HIP(ctx, hipGetLastError());
    return 0;
}

template <class S>
int pivot_host(xpg_ctx * ctx, S * tab, int m, int W, S * obj, int rhs, int row, int col)
{
    if (!ctx || !tab || !obj || m <= 0 || W <= 1) return XPG_ERR_SHAPE;
    const int ld = round_up(W, 16);
    S * d_tab = 0; S * d_obj = 0;
    XPG_HIP(ctx, hipMalloc((void **)&d_tab, (size_t)m * ld * sizeof(S)));
    if (hipMalloc((void **)&d_obj, (size_t)ld * sizeof(S)) != hipSuccess) { (void)hipFree(d_tab); return XPG_ERR_ALLOC; }
    int rc = 0;
    hipError_t e = hipMemcpy2DAsync(d_tab, (size_t)ld * sizeof(S), tab, (size_t)W * sizeof(S),
                                    (size_t)W * sizeof(S), m, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_obj, obj, (size_t)W * sizeof(S), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) rc = pivot_dev<S>(ctx, d_tab, m, W, ld, d_obj, rhs, row, col);
    if (e == hipSuccess && rc == 0)
        e = hipMemcpy2DAsync(tab, (size_t)W * sizeof(S), d_tab, (size_t)ld * sizeof(S),
                             (size_t)W * sizeof(S), m, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && rc == 0) e = hipMemcpyAsync(obj, d_obj, (size_t)W * sizeof(S), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_tab); (void)hipFree(d_obj);
    if (e != hipSuccess) { ctx->err = hipGetErrorString(e); return XPG_ERR_HIP; }
    return rc;
}

} // namespace

extern "C" {

int xpg_pivot_f64_dev(xpg_ctx * ctx, double * tab, int m, int W, int ld, double * obj,
                      int rhs_idx, int row, int col)
{
    XPG_BIND(ctx); return pivot_dev<F64>(ctx, (F64 *)tab, m, W, ld, (F64 *)obj, rhs_idx, row, col); }
int xpg_pivot_rat32_dev(xpg_ctx * ctx, xpg_rat32 * tab, int m, int W, int ld, xpg_rat32 * obj,
                        int rhs_idx, int row, int col)
{
    XPG_BIND(ctx); return pivot_dev<R32>(ctx, (R32 *)tab, m, W, ld, (R32 *)obj, rhs_idx, row, col); }
int xpg_pivot_f64(xpg_ctx * ctx, double * tab, int m, int W, double * obj, int rhs_idx, int row, int col)
{
    XPG_BIND(ctx); return pivot_host<F64>(ctx, (F64 *)tab, m, W, (F64 *)obj, rhs_idx, row, col); }
int xpg_pivot_rat32(xpg_ctx * ctx, xpg_rat32 * tab, int m, int W, xpg_rat32 * obj, int rhs_idx, int row, int col)
{
    XPG_BIND(ctx); return pivot_host<R32>(ctx, (R32 *)tab, m, W, (R32 *)obj, rhs_idx, row, col); }

// ---- device-resident LP ---------------------------------------------------------------
int xpg_lp_create(xpg_ctx * ctx, int kind, const void * leq, int m, int cols, const void * tgtf,
                  const void * vc_diag, const void * vc_rhs, int src_on_device, xpg_lp ** out)
{
    XPG_BIND(ctx);
    if (!ctx || !out || !leq || !tgtf || m <= 0 || cols < 2 || (kind != 0 && kind != 1))
        return XPG_ERR_SHAPE;
    *out = 0;
    xpg_lp * h = new (std::nothrow) xpg_lp();
    if (!h) return XPG_ERR_ALLOC;
    int rc;
    if (kind == 0) {
        Lp<F64> * p = new (std::nothrow) Lp<F64>();
        if (!p) { delete h; return XPG_ERR_ALLOC; }
        p->ctx = ctx; p->kind = 0; h->impl = p;
        rc = p->create(leq, m, cols, tgtf, vc_diag, vc_rhs, src_on_device);
    } else {
        Lp<R32> * p = new (std::nothrow) Lp<R32>();
        if (!p) { delete h; return XPG_ERR_ALLOC; }
        p->ctx = ctx; p->kind = 1; h->impl = p;
        rc = p->create(leq, m, cols, tgtf, vc_diag, vc_rhs, src_on_device);
    }
    if (rc) { delete h->impl; delete h; return rc; }
    *out = h;
    return 0;
}

void xpg_lp_destroy(xpg_lp * lp)
{
    if (!lp) return;
    XPG_BIND(lp->impl ? lp->impl->ctx : (xpg_ctx *)0);
    if (lp->impl) { (void)hipStreamSynchronize(lp->impl->ctx->stream); delete lp->impl; }
    delete lp;
}

#define XPG_DISPATCH(lp, expr)                                                   \
    do {                                                                         \
        if (!(lp) || !(lp)->impl) return XPG_ERR_SHAPE;                          \
        XPG_BIND((lp)->impl->ctx);                                               \
        if ((lp)->impl->kind == 0) { Lp<F64> * p = (Lp<F64> *)(lp)->impl; return expr; } \
        Lp<R32> * p = (Lp<R32> *)(lp)->impl; return expr;                        \
    } while (0)

int xpg_lp_two_stage(xpg_lp * lp, unsigned max_iter) { XPG_DISPATCH(lp, p->two_stage(max_iter)); }
int xpg_lp_begin(xpg_lp * lp) { XPG_DISPATCH(lp, p->begin()); }
int xpg_lp_iterate(xpg_lp * lp, unsigned pivots) { XPG_DISPATCH(lp, p->iterate(pivots)); }
int xpg_lp_read(xpg_lp * lp, void * tab, void * obj, uint8_t * nvset, uint8_t * bvset,
                int32_t * bv2eq, int32_t * eq2bv, void * maxv, void * sol)
{ XPG_DISPATCH(lp, p->read(tab, obj, nvset, bvset, bv2eq, eq2bv, maxv, sol)); }

int xpg_lp_shape(xpg_lp * lp, int * rows, int * W, int * rhs_idx)
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    int m, w, r;
    if (lp->impl->kind == 0) { Lp<F64> * p = (Lp<F64> *)lp->impl; m = p->v.m; w = p->v.W; r = p->v.rhs; }
    else { Lp<R32> * p = (Lp<R32> *)lp->impl; m = p->v.m; w = p->v.W; r = p->v.rhs; }
    if (rows) *rows = m;
    if (W) *W = w;
    if (rhs_idx) *rhs_idx = r;
    return 0;
}

int xpg_lp_set_options(xpg_lp * lp, int pricing, double feas_rel_tol)
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    XPG_BIND(lp->impl->ctx);
    if (lp->impl->kind == 0) return ((Lp<F64> *)lp->impl)->set_options(pricing, feas_rel_tol);
    return ((Lp<R32> *)lp->impl)->set_options(pricing, feas_rel_tol);
}

int xpg_lp_pivots_done(xpg_lp * lp, unsigned * out)
{
    if (!lp || !lp->impl || !out) return XPG_ERR_SHAPE;
    XPG_BIND(lp->impl->ctx);
    LoopState hs;
    int rc;
    if (lp->impl->kind == 0) rc = ((Lp<F64> *)lp->impl)->read_state(&hs);
    else rc = ((Lp<R32> *)lp->impl)->read_state(&hs);
    if (rc) return rc;
    *out = hs.total_pivots;
    return 0;
}

int xpg_lp_counters(xpg_lp * lp, unsigned * sweeps_full, unsigned * sweeps_partial)
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    XPG_BIND(lp->impl->ctx);
    LoopState hs;
    int rc;
    if (lp->impl->kind == 0) rc = ((Lp<F64> *)lp->impl)->read_state(&hs);
    else rc = ((Lp<R32> *)lp->impl)->read_state(&hs);
    if (rc) return rc;
    if (sweeps_full) *sweeps_full = hs.blk.sweeps_full;
    if (sweeps_partial) *sweeps_partial = hs.blk.sweeps_part;
    return 0;
}

// Host-side views of two pieces of launch geometry, for the CPU test suite (no device needed): the blocked sweep's
// workgroup -> tile map (every tile of a strips x rowblocks tableau exactly once, whatever the shape) and the leading
// dimension a device tableau of W live columns gets.
int xpg_test_sweep_tile(int strips, int rowblocks, int rev, int lid, int * bx, int * by)
{
    if (!bx || !by || strips <= 0 || rowblocks <= 0) return XPG_ERR_SHAPE;
    if (lid < 0) return blk_sweep_grid(strips, rowblocks);      // lid < 0: the grid size
    int x = -1, y = -1;
    const bool live = blk_sweep_tile(lid, strips, rowblocks, rev, x, y);
    *bx = x; *by = y;
    return live ? 1 : 0;
}
int xpg_test_pick_ld(int W) { return W > 0 ? pick_ld(W) : XPG_ERR_SHAPE; }
// r32_loop_plan (lp_host.hip.h) for a Rational tableau of m x W: forced = 0 no XPG_R32_LOOP, 1 "fused", 2 "pipe".
int xpg_test_r32_loop_plan(int m, int W, int forced, int32_t * out, int n)
{
    if (!out || n < 0 || m <= 0 || W <= 0 || forced < R32_FORCE_NONE || forced > R32_FORCE_PIPE) return XPG_ERR_SHAPE;
    const R32LoopPlan p = r32_loop_plan(m, W, forced);
    const int32_t f[11] = { p.fused, p.fN, p.fNP, p.fgx, p.fgy, p.frows, p.pN, p.pNP, p.pgx, p.pgy, p.prows };
    return copy_fields(out, n, f);
}
} // extern "C"
namespace xpg { namespace {
__global__ __launch_bounds__(256) void k_test_canon_ops(int n, const R32 * a, const R32 * k, const R32 * e, R32 * out_fma, R32 * out_div)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (out_fma) out_fma[i] = fma_canon(a[i], k[i], e[i]);
    if (out_div) out_div[i] = k[i].num == 0 ? R32(0, 1) : div_canon(a[i], k[i]);
}
__global__ __launch_bounds__(256) void k_test_any_ops(int n, const R32 * a, const R32 * b, R32 * out_mul, R32 * out_add, R32 * out_div)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (out_mul) out_mul[i] = mul_any(a[i], b[i]);
    if (out_add) out_add[i] = add_any(a[i], b[i]);
    if (out_div) out_div[i] = div_any(a[i], b[i]);
}
} }
extern "C" {
int xpg_test_any_ops_rat32(xpg_ctx * ctx, int n, const xpg_rat32 * a, const xpg_rat32 * b, xpg_rat32 * out_mul, xpg_rat32 * out_add,
                           xpg_rat32 * out_div)
{
    if (!ctx || n < 0 || !a || !b) return XPG_ERR_SHAPE;
    XPG_BIND(ctx);
    if (n == 0) return 0;
    const size_t bytes = (size_t)n * sizeof(R32);
    DevBuf d;
    XPG_HIP(ctx, d.alloc(ctx, 5 * bytes));
    R32 * base = (R32 *)d.p;
    XPG_HIP(ctx, hipMemcpyAsync(base, a, bytes, hipMemcpyHostToDevice, ctx->stream));
    XPG_HIP(ctx, hipMemcpyAsync(base + n, b, bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_test_any_ops, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, base, base + n,
                       out_mul ? base + 2 * (size_t)n : (R32 *)0, out_add ? base + 3 * (size_t)n : (R32 *)0, out_div ? base + 4 * (size_t)n : (R32 *)0);
    if (out_mul) XPG_HIP(ctx, hipMemcpyAsync(out_mul, base + 2 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_add) XPG_HIP(ctx, hipMemcpyAsync(out_add, base + 3 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_div) XPG_HIP(ctx, hipMemcpyAsync(out_div, base + 4 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int xpg_test_canon_ops_rat32(xpg_ctx * ctx, int n, const xpg_rat32 * a, const xpg_rat32 * k, const xpg_rat32 * e,
                             xpg_rat32 * out_fma, xpg_rat32 * out_div)
{
    if (!ctx || n < 0 || !a || !k || !e) return XPG_ERR_SHAPE;
    XPG_BIND(ctx);
    if (n == 0) return 0;
    const R32 * in[3] = { (const R32 *)a, (const R32 *)k, (const R32 *)e };
    for (int t = 0; t < 3; t++)
        for (int i = 0; i < n; i++)
            if (!canonical(in[t][i])) { ctx->err = "xpg_test_canon_ops_rat32: operand not canonical"; return XPG_ERR_SHAPE; }
    const size_t bytes = (size_t)n * sizeof(R32);
    DevBuf d;
    XPG_HIP(ctx, d.alloc(ctx, 5 * bytes));
    R32 * base = (R32 *)d.p;
    for (int t = 0; t < 3; t++) XPG_HIP(ctx, hipMemcpyAsync(base + (size_t)t * n, in[t], bytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_test_canon_ops, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, base, base + n, base + 2 * (size_t)n,
                       out_fma ? base + 3 * (size_t)n : (R32 *)0, out_div ? base + 4 * (size_t)n : (R32 *)0);
    if (out_fma) XPG_HIP(ctx, hipMemcpyAsync(out_fma, base + 3 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (out_div) XPG_HIP(ctx, hipMemcpyAsync(out_div, base + 4 * (size_t)n, bytes, hipMemcpyDeviceToHost, ctx->stream));
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int xpg_lp_chain_aborts(xpg_lp * lp, unsigned * aborts, int * chain_off, unsigned * runs)
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    XPG_BIND(lp->impl->ctx);
    if (runs) *runs = 0;
    if (lp->impl->kind != 0) { if (aborts) *aborts = 0; if (chain_off) *chain_off = 0; return 0; }
    Lp<F64> * p = (Lp<F64> *)lp->impl;
    LoopState hs;
    const int rc = p->read_state(&hs);
    if (rc) return rc;
    if (aborts) *aborts = hs.blk.ch_aborts;
    if (chain_off) *chain_off = p->chain_off ? 1 : 0;
    if (runs) *runs = hs.blk.ch_runs;
    return 0;
}

int xpg_lp_loop_info(xpg_lp * lp, int32_t * out, int n)
{
    if (!lp || !lp->impl || !out || n < 0) return XPG_ERR_SHAPE;
    int32_t f[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (lp->impl->kind == 0) ((Lp<F64> *)lp->impl)->loop_info(f);
    else ((Lp<R32> *)lp->impl)->loop_info(f);
    return copy_fields(out, n, f);
}

#ifdef XPG_STAMPS
// diagnostic builds only (not declared in the header): the phase tick sums of the blocked loop
int xpg_lp_debug(xpg_lp * lp, unsigned long long * out8)
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    LoopState hs;
    int rc = lp->impl->kind == 0 ? ((Lp<F64> *)lp->impl)->read_state(&hs) : ((Lp<R32> *)lp->impl)->read_state(&hs);
    if (rc) return rc;
    for (int k = 0; k < 8; k++) out8[k] = hs.blk.dbg[k];
    return 0;
}
// the staged rows / columns of the last batch: E[BLK_MAX][ld], K[m][BLK_MAX]; *ld receives the leading dimension and
// *blk_max the stage capacity (BLK_MAX). The caller says how many stages its arrays were sized for (`cap`, from a first
// call with E = K = NULL); a capacity that is not the library's is refused instead of overrunning the caller's heap.
int xpg_lp_debug_staged(xpg_lp * lp, double * E, double * K, int * ld, int * blk_max, int cap)
{
    if (!lp || !lp->impl || lp->impl->kind != 0) return XPG_ERR_SHAPE;
    Lp<F64> * p = (Lp<F64> *)lp->impl;
    xpg_ctx * ctx = p->ctx;
    if (ld) *ld = p->v.ld;
    if (blk_max) *blk_max = BLK_MAX;
    if ((E || K) && cap != BLK_MAX) return XPG_ERR_SHAPE;
    if (E) XPG_HIP(ctx, hipMemcpy(E, p->v.blkE, (size_t)BLK_MAX * p->v.ld * 8, hipMemcpyDeviceToHost));
    if (K) XPG_HIP(ctx, hipMemcpy(K, p->v.blkK, (size_t)p->v.m * BLK_MAX * 8, hipMemcpyDeviceToHost));
    return 0;
}
int xpg_lp_debug_counts(xpg_lp * lp, int * rowcnt, int * colcnt, int n)
{
    if (!lp || !lp->impl || lp->impl->kind != 0) return XPG_ERR_SHAPE;
    Lp<F64> * p = (Lp<F64> *)lp->impl;
    xpg_ctx * ctx = p->ctx;
    XPG_HIP(ctx, hipMemcpy(rowcnt, p->v.rowcnt, (size_t)n * 4, hipMemcpyDeviceToHost));
    XPG_HIP(ctx, hipMemcpy(colcnt, p->v.colcnt, (size_t)n * 4, hipMemcpyDeviceToHost));
    return 0;
}
int xpg_lp_debug_chain_ts(xpg_lp * lp, unsigned long long * out, int * blk_max, int cap)   // [4][BLK_MAX][8]; cap as above
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    xpg_ctx * ctx = lp->impl->ctx;
    if (blk_max) *blk_max = BLK_MAX;
    if (!out) return 0;
    if (cap != BLK_MAX) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ch_ts), sizeof(unsigned long long) * 4 * BLK_MAX * 8));
    return 0;
}
int xpg_lp_debug_rows(xpg_lp * lp, double * out)              // [4][8192]
{
    if (!lp || !lp->impl) return XPG_ERR_SHAPE;
    xpg_ctx * ctx = lp->impl->ctx;
    XPG_HIP(ctx, hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dbg_rows), sizeof(double) * 4 * 8192));
    return 0;
}
#endif

int xpg_lp_chain_folds(xpg_lp * lp, unsigned * folds)
{
    if (!lp || !lp->impl || !folds) return XPG_ERR_SHAPE;
    XPG_BIND(lp->impl->ctx);
    *folds = 0;
    if (lp->impl->kind != 0) return 0;
    LoopState hs;
    const int rc = ((Lp<F64> *)lp->impl)->read_state(&hs);
    if (rc) return rc;
    *folds = hs.blk.ch_folds;
    return 0;
}

int xpg_lp_trace(xpg_lp * lp, int32_t * pairs, int cap_pairs, int * n_pairs)
{
    if (!lp || !lp->impl || !n_pairs) return XPG_ERR_SHAPE;
    xpg_ctx * ctx = lp->impl->ctx;
    XPG_BIND(ctx);
    LoopState hs;
    int rc; int * d_trace; int cap;
    if (lp->impl->kind == 0) { Lp<F64> * p = (Lp<F64> *)lp->impl; rc = p->read_state(&hs); d_trace = p->v.trace; cap = p->v.trace_cap; }
    else { Lp<R32> * p = (Lp<R32> *)lp->impl; rc = p->read_state(&hs); d_trace = p->v.trace; cap = p->v.trace_cap; }
    if (rc) return rc;
    int n = (int)hs.total_pivots;
    *n_pairs = n;
    if (n > cap) n = cap;
    if (n > cap_pairs) n = cap_pairs;
    if (pairs && n > 0) {
        XPG_HIP(ctx, hipMemcpyAsync(pairs, d_trace, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int xpg_trim(xpg_ctx * ctx)
{
    XPG_BIND(ctx);
    if (!ctx) return XPG_ERR_SHAPE;
    XPG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (auto & b : ctx->dev_cache) (void)hipFree(b.first);
    ctx->dev_cache.clear(); ctx->dev_cache_bytes = 0;
    if (ctx->hpack) { (void)hipHostFree(ctx->hpack); ctx->hpack = 0; ctx->hpack_cap = 0; }
    if (ctx->hred) { (void)hipHostFree(ctx->hred); ctx->hred = 0; ctx->hred_cap = 0; }
    for (Scratch & s : ctx->scratch) s.release();
    return 0;
}

int xpg_mip_warm_f64(xpg_ctx * ctx, int is_max, const double * tgtf, const double * leq, int leq_rows, int cols, int is_bin,
                     double * out_v, double * out_sol, long long * out_stats)
{
    XPG_BIND(ctx);
    if (!ctx || !tgtf || !leq || leq_rows <= 0 || cols < 2 || !out_v) return XPG_ERR_SHAPE;
    std::vector<double> obj(tgtf, tgtf + cols);
    if (!is_max) for (int j = 0; j < cols; j++) obj[(size_t)j] = -obj[(size_t)j];       // min c.x = -max (-c).x
    WarmMip W(ctx);
    WarmStats S;
    double v = 0.0;
    const int st = W.solve(obj.data(), leq, leq_rows, cols, is_bin != 0, &v, out_sol, S);
    if (out_stats) { out_stats[0] = S.nodes; out_stats[1] = S.dual_pivots; out_stats[2] = S.root_pivots; out_stats[3] = S.max_depth; }
    if (st == XPG_IP_SUCC) *out_v = is_max ? v : -v;
    else *out_v = 0.0;
    return st;
}

int xpg_mip_warm_batch_f64(xpg_ctx * ctx, int nb, int is_max, const double * tgtf, const double * leq, int leq_rows, int cols, int is_bin,
                           int32_t * out_status, double * out_v, double * out_sol, long long * out_stats)
{
    XPG_BIND(ctx);
    return warm_mip_batch(ctx, nb, is_max, tgtf, leq, leq_rows, cols, is_bin, out_status, out_v, out_sol, out_stats);
}
// host-only test view: what xpg_mip_warm_batch_f64 would launch nb trees of that shape with (wb_plan, the launch's own rule)
int xpg_test_warm_batch_geometry(int rows, int cols, int is_bin, int nb, long long * out, int n)
{
    if (!out || n < 0 || rows <= 0 || cols < 2 || nb <= 0) return XPG_ERR_SHAPE;
    const WbPlan P = wb_plan(rows, cols, is_bin, nb);
    const long long f[9] = { (long long)P.lds, P.refused, P.S.depth_cap, P.S.mcap, P.S.wcap, (long long)P.S.snap_stride, (long long)P.S.tree_stride,
                             P.chunk, P.launches };
    return copy_fields(out, n, f);
}

} // extern "C"
