// Host launch wrappers of lineq_kernels.hip.h: stage the caller's host arrays
// through HBM, one wavefront per system, results back. No arithmetic here.
#pragma once
#include <hip/hip_runtime.h>
#include <chrono>
#include "ctx.hip.h"
#include "lineq_kernels.hip.h"

namespace xpg {


// mode 0: removeIdenRow, 1: reduce -- in place on mats[nb][rows][cols]. The *_dev forms take device arrays and
// only enqueue (the caller synchronises the handle's stream); the host-array forms stage through them.
inline int lineq_reduce_batch_dev(xpg_ctx * ctx, int nb, R32 * d_mats, int rows, int cols, int rhs, int mode,
                                  int is_intersect, int32_t * d_rows, int32_t * d_ok)
{
    if (!ctx || nb < 0 || !d_mats || rows <= 0 || cols <= 0 || !d_rows || !d_ok || (mode == 1 && (rhs < 0 || rhs >= cols)))
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const size_t lds = lineq_lds_bytes(rows, cols);
    if (lds > 160 * 1024 || rows > 32767) return XPG_ERR_UNSUPPORTED;
    const LineqGeom q = lineq_geom(nb, rows > cols ? rows : cols, lds);
    XPG_TRY(lds_limit((const void *)k_reduce_batch, ctx->device, q.lds));
    hipLaunchKernelGGL(k_reduce_batch, dim3(q.grid), q.block, q.lds, ctx->stream, nb, d_mats, rows,
                       cols, rhs, mode, is_intersect, (int *)d_rows, (int *)d_ok, q.sys_lds);
    XPG_TRY(hipGetLastError());
    return 0;
}
// Pinned host memory of one of the handle's staging buffers: grows, never shrinks, freed with the handle.
inline int pinned_reserve(xpg_ctx * ctx, void *& buf, size_t & buf_cap, size_t bytes, const char * what)
{
    if (bytes <= buf_cap) return 0;
    const size_t cap = bytes + bytes / 4 + 4096;
    void * fresh = 0;
    if (hipHostMalloc(&fresh, cap, hipHostMallocDefault) != hipSuccess) { ctx->err = std::string("hipHostMalloc(") + what + ")"; return XPG_ERR_ALLOC; }
    if (buf) (void)hipHostFree(buf);
    buf = fresh; buf_cap = cap;
    return 0;
}
// The pinned buffer of a packed-result call: hpack, what the *view of a packed entry point points into; or, `internal`,
// hred -- for the calls that copy their results out before they return (the in-place reduce forms, the ragged fme) and
// must leave that view alone (include/xpoly_amd.h: valid until the next packed call).
inline int hpack_reserve(xpg_ctx * ctx, size_t bytes, bool internal = false)
{
    return internal ? pinned_reserve(ctx, ctx->hred, ctx->hred_cap, bytes, "in-place staging")
                    : pinned_reserve(ctx, ctx->hpack, ctx->hpack_cap, bytes, "packed results");
}
inline char * hpack_buf(xpg_ctx * ctx, bool internal) { return (char *)(internal ? ctx->hred : ctx->hpack); }

// THE way up of a packed call on nb systems of ONE shape (reduce, fme, projection, levels, fused calcBound), and the buffers of
// its way down. The systems go up once: small batches (<= 4 MB) through the handle's pinned buffer -- one memcpy, then a true
// asynchronous copy --, large ones straight from the caller's pages (the runtime's own staging is faster than a single-threaded
// memcpy of tens of MB). The pinned buffer (hpack, or hred when `internal`: hpack_reserve) is laid out as [meta_al: row offsets
// [nres + 1], then the ints as on the device][in_stage: the staged input][room: the result slots where they are small (<= 512 KB)
// and come down whole; in_place: the input's size, k_pack_rows writes there]. dints: rows [nres], then nv verdict arrays [nb].
// dout: the nres result slots, bo bytes (none in_place: the kernel works in di).
struct PackedUp {
    DevBuf di, dout, dints, doff;
    int nb, nres, nv; size_t bo, meta_al, in_stage; bool small_out, internal;
    int32_t * d_rows() const { return (int32_t *)dints.p; }
    int32_t * d_verdict(int v) const { return (int32_t *)dints.p + nres + (size_t)v * nb; }
    size_t ints_bytes() const { return ((size_t)nres + (size_t)nv * nb) * 4; }
    char * h_room(xpg_ctx * ctx) const { return hpack_buf(ctx, internal) + meta_al + in_stage; }
};
// `more` (transformed nests; else none): a second host array that travels behind the first -- di holds [bi_first bytes of
// mats][more_bytes of more], staged and sent as ONE block where the two are small together, else one copy each.
inline int packed_up_bytes(xpg_ctx * ctx, int nb, const void * mats, size_t bi_first, const void * more, size_t more_bytes, int nres, int nv,
                           size_t bo, bool in_place, bool internal, PackedUp & u)
{
    const size_t bi = bi_first + more_bytes;
    const bool small_in = bi <= ((size_t)4 << 20);
    u.nb = nb; u.nres = nres; u.nv = nv; u.bo = bo; u.internal = internal;
    u.meta_al = ((size_t)(nres + 1) * 8 + u.ints_bytes() + 255) & ~(size_t)255;
    u.in_stage = small_in ? bi : 0;
    u.small_out = !in_place && bo <= ((size_t)512 << 10);
    XPG_TRY(u.di.alloc(ctx, bi)); XPG_TRY(u.dints.alloc(ctx, u.ints_bytes())); XPG_TRY(u.doff.alloc(ctx, (size_t)(nres + 1) * 8));
    if (!in_place) XPG_TRY(u.dout.alloc(ctx, bo));
    if (const int rc = hpack_reserve(ctx, u.meta_al + u.in_stage + (in_place ? bi : u.small_out ? bo : 0), internal)) return rc;
    if (small_in) {
        char * stage = hpack_buf(ctx, internal) + u.meta_al;
        memcpy(stage, mats, bi_first);
        if (more_bytes) memcpy(stage + bi_first, more, more_bytes);
        XPG_TRY(hipMemcpyAsync(u.di.p, stage, bi, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    XPG_TRY(hipMemcpyAsync(u.di.p, mats, bi_first, hipMemcpyHostToDevice, ctx->stream));
    if (more_bytes) XPG_TRY(hipMemcpyAsync((char *)u.di.p + bi_first, more, more_bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
inline int packed_up(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int nres, int nv, size_t bo, bool in_place, bool internal,
                     PackedUp & u)
{
    return packed_up_bytes(ctx, nb, mats, (size_t)nb * rows * cols * 8, (const void *)0, 0, nres, nv, bo, in_place, internal, u);
}

// Lineq::reduce / removeIdenRow for nb host systems with a PACKED result (round 6): row_offsets[nb + 1] (in rows) and the
// surviving rows of every system back to back. The systems go up once (packed_up), are reduced in place in HBM, and k_pack_rows
// writes the survivors STRAIGHT INTO the handle's pinned host buffer (hipHostMalloc memory is mapped on the device: coalesced
// 16-byte stores over the link), so the row counts, the verdicts, the offsets and the rows are all there after ONE
// synchronisation -- no device slots come back, nothing is allocated per call beyond the handle's cached blocks. `out` (may be
// NULL) receives a copy of the rows, *view (may be NULL) the pinned buffer itself (valid until the handle's next packed call),
// out_rows (may be NULL) the per-system counts. `internal`: staged through hred instead (hpack_reserve), for the in-place form below.
inline int lineq_reduce_batch_packed(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int rhs, int mode, int is_intersect,
                                     R32 * out, long long out_cap_rows, const R32 ** view, long long * row_offsets,
                                     int32_t * out_rows, int32_t * out_ok, bool internal = false)
{
    if (view) *view = 0;
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols <= 0 || !row_offsets || (mode == 1 && (rhs < 0 || rhs >= cols || !out_ok)) ||
        (out && out_cap_rows < 0))
        return XPG_ERR_SHAPE;
    if (nb == 0) { row_offsets[0] = 0; return 0; }
    PackedUp u;
    if (const int rc = packed_up(ctx, nb, mats, rows, cols, nb, 1, 0, true, internal, u)) return rc;
    char * hp = hpack_buf(ctx, internal), * hrows_out = u.h_room(ctx);   // where the survivors land
    if (const int rc = lineq_reduce_batch_dev(ctx, nb, (R32 *)u.di.p, rows, cols, rhs, mode, is_intersect, u.d_rows(), u.d_verdict(0))) return rc;
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(1024), 0, ctx->stream, nb, (const int *)u.d_rows(), (long long *)u.doff.p);
    hipLaunchKernelGGL(k_pack_rows, dim3(nb < 4096 ? nb : 4096), dim3(256), 0, ctx->stream, nb, (const R32 *)u.di.p, rows, cols,
                       (const int *)u.d_rows(), (const long long *)u.doff.p, (R32 *)hrows_out);
    XPG_TRY(hipGetLastError());
    long long * h_off = (long long *)hp; int32_t * h_rows = (int32_t *)(hp + (size_t)(nb + 1) * 8), * h_ok = h_rows + nb;
    XPG_TRY(hipMemcpyAsync(h_off, u.doff.p, (size_t)(nb + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(h_rows, u.dints.p, u.ints_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(row_offsets, h_off, (size_t)(nb + 1) * 8);
    if (out_rows) memcpy(out_rows, h_rows, (size_t)nb * 4);
    if (out_ok && mode == 1) memcpy(out_ok, h_ok, (size_t)nb * 4);
    const long long total = row_offsets[nb];
    if (out && out_cap_rows < total) return XPG_ERR_SHAPE;
    if (out && total > 0) memcpy(out, hrows_out, (size_t)total * cols * 8);
    if (view && total > 0) *view = (const R32 *)hrows_out;
    return 0;
}
// The in-place form of the reference's signature (Lineq::reduce(m, ...) overwrites m): the packed call above, then the
// survivors of system b copied to the front of its slot. Rows of a slot behind out_rows[b] keep the caller's input.
inline int lineq_reduce_batch(xpg_ctx * ctx, int nb, R32 * mats, int rows, int cols, int rhs, int mode,
                              int is_intersect, int32_t * out_rows, int32_t * out_ok)
{
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols <= 0 || !out_rows || (mode == 1 && (rhs < 0 || rhs >= cols)))
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    std::vector<long long> off((size_t)nb + 1);
    std::vector<int32_t> ok_tmp;
    if (mode == 1 && !out_ok) { ok_tmp.resize((size_t)nb); out_ok = ok_tmp.data(); }
    const R32 * view = 0;
    const int rc = lineq_reduce_batch_packed(ctx, nb, mats, rows, cols, rhs, mode, is_intersect, (R32 *)0, 0, &view, off.data(), out_rows, out_ok,
                                             true);
    if (rc) return rc;
    const size_t rowb = (size_t)cols * 8, slot = (size_t)rows * rowb;
    for (int b = 0; b < nb; b++)
        if (out_rows[b] > 0) memcpy((char *)mats + (size_t)b * slot, (const char *)view + (size_t)off[(size_t)b] * rowb, (size_t)out_rows[b] * rowb);
    return 0;
}

// LDS of one system in k_fme_batch and the rows of its result area. Occupancy beats residency here: the result of
// a system is read and written a few times per row (pair sums, hash, classification, compaction) and its HBM slot
// is L2-resident, while every KB of LDS per system is fewer systems per CU for a kernel that waits on dependent
// gcd chains. Measured at 40 x 13 (16 384 systems): whole cap-row result in LDS (54 KB, 2 per CU) 8.0 M systems/s;
// a result area for the typical result in 32 KB 14.6 M; in 20 KB 20.2 M; NO result area (9 KB: the normalised
// input and the scratch) 27.9 M. So the result stays in LDS only while the whole layout is small (<= 12 KB: the
// 16 x 9 class), and otherwise the area holds just the row factors of the normalisation.
struct FmeLds { int cap_lds; size_t lds; };
inline FmeLds fme_lds(int cap, int cap_in, int cols)
{
    const int capx = cap > cap_in ? cap : cap_in;
    const size_t scratch = lineq_lds_bytes(capx, cols) - (size_t)capx * cols * 8 + 16;
    const size_t tmp = (size_t)cap_in * cols * 8;
    const size_t full = (size_t)cap * cols * 8 + tmp + scratch;
    FmeLds f;
    if (full <= (size_t)12 * 1024) { f.cap_lds = cap; f.lds = full; return f; }
    f.cap_lds = (cap_in + cols - 1) / cols;                       // room for one factor per input row
    if (f.cap_lds > cap) f.cap_lds = cap;
    f.lds = (size_t)f.cap_lds * cols * 8 + tmp + scratch;
    return f;
}
// d_outs must be zeroed by the caller where it wants zeros past a result's last row (the host form does).
inline int lineq_fme_batch_dev(xpg_ctx * ctx, int nb, const R32 * d_mats, int rows, int cols, int rhs, int u,
                               int darkshadow, R32 * d_outs, int cap, int32_t * d_rows, int32_t * d_ok)
{
    if (!ctx || nb < 0 || !d_mats || !d_outs || rows <= 0 || cols <= 1 || rhs < 1 || rhs >= cols || u < 0 || u >= rhs ||
        cap < rows || !d_rows || !d_ok)
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const FmeLds fl = fme_lds(cap, rows, cols);
    if (fl.lds > 160 * 1024 || cap > 32767) return XPG_ERR_UNSUPPORTED;
    const LineqGeom q = lineq_geom(nb, 64, fl.lds);
    XPG_TRY(lds_limit((const void *)k_fme_batch, ctx->device, q.lds));
    hipLaunchKernelGGL(k_fme_batch, dim3(q.grid), q.block, q.lds, ctx->stream, nb, d_mats, rows,
                       (const int *)0, cols, rhs, u, darkshadow, d_outs, cap, (int *)d_rows, (int *)d_ok,
                       fl.cap_lds, (int *)0, q.sys_lds);
    XPG_TRY(hipGetLastError());
    return 0;
}
inline int lineq_fme_batch(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int rhs, int u,
                           int darkshadow, R32 * outs, int cap, int32_t * out_rows, int32_t * out_ok)
{
    if (!ctx || nb < 0 || !mats || !outs || rows <= 0 || cols <= 1 || cap < rows || !out_rows || !out_ok) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const size_t bi = (size_t)nb * rows * cols * 8, bo = (size_t)nb * cap * cols * 8;
    DevBuf di, dout, dr, dk;
    XPG_TRY(di.alloc(ctx, bi)); XPG_TRY(dout.alloc(ctx, bo)); XPG_TRY(dr.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dk.alloc(ctx, (size_t)nb * 4));
    XPG_TRY(hipMemcpyAsync(di.p, mats, bi, hipMemcpyHostToDevice, ctx->stream));
    XPG_TRY(hipMemsetAsync(dout.p, 0, bo, ctx->stream));
    const int rc = lineq_fme_batch_dev(ctx, nb, (const R32 *)di.p, rows, cols, rhs, u, darkshadow, (R32 *)dout.p, cap,
                                       (int32_t *)dr.p, (int32_t *)dk.p);
    if (rc) return rc;
    XPG_TRY(hipMemcpyAsync(outs, dout.p, bo, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(out_rows, dr.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(out_ok, dk.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// The way down of a uniform packed call (fme, projection, levels, fused calcBound), after its kernel is enqueued: u.dout
// [nres][cap][cols] holds each result's live rows at the front of its slot, u.dints their counts and, behind them, the u.nv
// verdict arrays [nb] that `verdicts` names in the same order -- ONE copy brings all the ints down. small_out: the slots come down
// with them and are packed on the host -- one synchronisation, no scan / pack launches (a handful of systems: the drop-in adapter
// eliminates one per call). Else k_rows_scan, one synchronisation for the offsets, k_pack_rows, and only live rows cross the link.
// short_msg != NULL: a negative count (a result that needs -count rows) ends the call with XPG_ERR_UNSUPPORTED, the count in
// row_offsets[0] and the verdicts not written. A buffer too small (XPG_ERR_SHAPE) still gets its offsets and verdicts.
inline void no_lap(const char *) {}
template <class Lap>
inline int packed_rows_down(xpg_ctx * ctx, PackedUp & u, int cols, int cap, const char * short_msg, R32 * out, long long out_cap_rows,
                            const R32 ** view, long long * row_offsets, int32_t * const * verdicts, Lap lap)
{
    const int nres = u.nres;
    long long * h_off = (long long *)hpack_buf(ctx, u.internal);
    int32_t * h_rows = (int32_t *)(h_off + nres + 1);
    XPG_TRY(hipMemcpyAsync(h_rows, u.dints.p, u.ints_bytes(), hipMemcpyDeviceToHost, ctx->stream));
    const auto verdicts_out = [&]() {
        for (int v = 0; v < u.nv; v++) memcpy(verdicts[v], h_rows + nres + (size_t)v * u.nb, (size_t)u.nb * 4);
    };
    if (u.small_out) {
        char * hs = u.h_room(ctx);
        XPG_TRY(hipMemcpyAsync(hs, u.dout.p, u.bo, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        long long tot = 0;
        for (int b = 0; b < nres; b++) {
            if (short_msg && h_rows[b] < 0) { ctx->err = short_msg; row_offsets[0] = h_rows[b]; return XPG_ERR_UNSUPPORTED; }
            row_offsets[b] = tot; tot += h_rows[b];
        }
        row_offsets[nres] = tot;
        verdicts_out();
        if (out && out_cap_rows < tot) return XPG_ERR_SHAPE;
        const size_t rowb = (size_t)cols * 8;
        for (int b = 0; b < nres; b++) {                           // forward moves: a destination never lies above its source
            const size_t nbytes = (size_t)(row_offsets[b + 1] - row_offsets[b]) * rowb;
            if (out) memcpy((char *)out + (size_t)row_offsets[b] * rowb, hs + (size_t)b * cap * rowb, nbytes);
            if (view) memmove(hs + (size_t)row_offsets[b] * rowb, hs + (size_t)b * cap * rowb, nbytes);
        }
        if (view) *view = (const R32 *)hs;
        return 0;
    }
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(1024), 0, ctx->stream, nres, (const int *)u.d_rows(), (long long *)u.doff.p);
    XPG_TRY(hipMemcpyAsync(h_off, u.doff.p, (size_t)(nres + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    if (short_msg)
        for (int b = 0; b < nres; b++)
            if (h_rows[b] < 0) { ctx->err = short_msg; row_offsets[0] = h_rows[b]; return XPG_ERR_UNSUPPORTED; }
    memcpy(row_offsets, h_off, (size_t)(nres + 1) * 8);
    verdicts_out();
    const long long total = row_offsets[nres];
    if (out && out_cap_rows < total) return XPG_ERR_SHAPE;
    if (total == 0 || (!out && !view)) return 0;                   // (neither: a sizing call)
    const size_t bp = (size_t)total * cols * 8;
    lap("scan+meta");
    DevBuf dpk;
    XPG_TRY(dpk.alloc(ctx, bp));
    hipLaunchKernelGGL(k_pack_rows, dim3(nres < 4096 ? nres : 4096), dim3(256), 0, ctx->stream, nres, (const R32 *)u.dout.p, cap, cols,
                       (const int *)u.d_rows(), (const long long *)u.doff.p, (R32 *)dpk.p);
    XPG_TRY(hipGetLastError());
    lap("pack");
    if (view) {                                                    // into pinned memory; the caller's copy, if any, from there
        const int rc = hpack_reserve(ctx, bp, u.internal);
        if (rc) return rc;
        char * hv = hpack_buf(ctx, u.internal);
        XPG_TRY(hipMemcpyAsync(hv, dpk.p, bp, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        if (out) memcpy(out, hv, bp);
        *view = (const R32 *)hv;
    } else {
        XPG_TRY(hipMemcpyAsync(out, dpk.p, bp, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
    }
    lap("d2h");
    return 0;
}

// Lineq::fme for nb systems with a PACKED result: row_offsets[nb + 1] (rows, not bytes) and the
// live rows of every system back to back, instead of nb worst-case slots of cap_rows rows (the typical result is a
// third of the worst case: 751 MB of slots against 267 MB of rows for 16 384 systems of 40 x 13). The systems go up and
// the rows come down through pinned memory; `out` (optional) receives a copy, *view (optional) the pinned buffer itself,
// valid until the next packed call on this handle. Returns 0; XPG_ERR_SHAPE when `out` holds fewer than the
// row_offsets[nb] rows needed (row_offsets is filled: the caller can size its buffer and call again). `internal`: staged
// through hred (hpack_reserve), for a caller that copies the rows out of *view before it returns.
inline int lineq_fme_batch_packed(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int rhs, int u, int darkshadow,
                                  int cap, R32 * out, long long out_cap_rows, const R32 ** view, long long * row_offsets,
                                  int32_t * out_ok, bool internal = false)
{
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols <= 1 || !row_offsets || !out_ok || (out && out_cap_rows < 0)) return XPG_ERR_SHAPE;
    if (view) *view = 0;
    if (nb == 0) { row_offsets[0] = 0; return 0; }
    if (cap <= 0) cap = rows * rows / 4 + rows + 1;                  // every (positive, negative) pair + the rows without u
    if (cap < rows) cap = rows;
    static const bool dbg = xpg_hook("XPG_LINEQ_DEBUG") != 0;
    const auto T0 = std::chrono::steady_clock::now();
    auto lap = [&](const char * what) { if (dbg) { (void)hipStreamSynchronize(ctx->stream); fprintf(stderr, "  fme_packed %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count()); } };
    PackedUp up;
    if (const int rc = packed_up(ctx, nb, mats, rows, cols, nb, 1, (size_t)nb * cap * cols * 8, false, internal, up)) return rc;
    lap("h2d");
    if (const int rc = lineq_fme_batch_dev(ctx, nb, (const R32 *)up.di.p, rows, cols, rhs, u, darkshadow, (R32 *)up.dout.p, cap, up.d_rows(),
                                           up.d_verdict(0))) return rc;
    lap("kernel");
    return packed_rows_down(ctx, up, cols, cap, "fme: a result needs more rows than cap_rows", out, out_cap_rows, view, row_offsets, &out_ok, lap);
}

// ---- THE plan of a fused call of this family (projection, levels, calcBound; one shape or mixed; the hull's producer) ------------
// One struct, and ONE rule for the capacities and the envelope (lineq_plan_rule); the five named rules below it -- project_plan,
// levels_plan, bounds_plan, ragged_chain_plan, bounds_ragged_plan -- are their own argument checks and per-system sums followed by
// one call of it. The launch and the xpg_test_lineq_*_plan view of a family ask the same named rule.
//   rows, cols   the envelope: the most rows and the widest system of the batch (one shape: its own)
//   slots        results of the call (cap_out rows of the system's OWN cols each), out_bytes their bytes
//   steps        elimination steps of the batch (calcBound), of one system (the uniform calcBound)
struct LineqPlan {
    int launches, rows, cols, cap, cap_out, cap_lds; LineqGeom q; long long seats, slots, steps; size_t seat_bytes, out_bytes;
    int inv_at;         // transformed nests: where the inverse's scratch starts in a system's LDS block (0: in the walk's areas)
};
// What tells the families apart in the rule: cap_rows <= 0 is fme's worst case rows^2 / 4 + rows + 1 (every positive-negative pair
// and the rows without the variable) or the packed calcBound's 4 * rows + 16; cap_out_rows <= 0 is cap, or min(cap, 4 * rows + 16)
// where the output slots follow nb * n_elim and not the grid (levels: at the projection's worst case the slots of 1024 nests of
// 60 rows and depth 6 would be gigabytes); a seat has two cap-row slots or three (calcBound: two sides and the held prefix); and
// the ragged kernels' seat is the workgroup (fme's whole wave), so they refuse a geometry with several systems per workgroup.
// inv_n > 0 (transformed nests): the system also inverts an inv_n x inv_n matrix before its walk begins. That scratch
// (transform_inv_bytes) is dead before the walk loads its input and the walk's result and input areas are idle until then: it
// lies IN those areas where they hold it (inv_at 0, no byte added) and else behind the walk's own scratch, its bytes added to the
// system's LDS before the 160 KB rule and the geometry.
struct PlanKind { bool fme_cap, levels_out; int seat_slots; bool seat_is_workgroup; int inv_n; };
inline PlanKind kind_chain(bool levels, bool ragged) { const PlanKind k = {true, levels, 2, ragged, 0}; return k; }
inline PlanKind kind_bounds(bool ragged) { const PlanKind k = {false, false, 3, ragged, 0}; return k; }
inline PlanKind kind_transform(int n) { const PlanKind k = {true, true, 2, false, n}; return k; }
// The rule. cap_out_rows above cap: cap. The LDS layout is fme_lds(cap, cap, cols), the rule calcBound's chains run under --
// measured for k_fme_batch, not again for the chain kernels. Returns 0 or XPG_ERR_UNSUPPORTED: rows or cap
// above 32767 (rows are indexed as short; the guard on rows keeps rows * rows an int), LDS over 160 KB, a seat that is no workgroup.
inline int lineq_plan_rule(int nb, int rows, int cols, int cap_rows, int cap_out_rows, const PlanKind & k, LineqPlan & p)
{
    p.launches = 1; p.rows = rows; p.cols = cols;
    if (rows > 32767) return XPG_ERR_UNSUPPORTED;
    const int few = 4 * rows + 16;
    p.cap = cap_rows > 0 ? cap_rows : (k.fme_cap ? rows * rows / 4 + rows + 1 : few);
    if (p.cap < rows) p.cap = rows;
    p.cap_out = cap_out_rows > p.cap ? p.cap : cap_out_rows;
    if (cap_out_rows <= 0) p.cap_out = k.levels_out && few < p.cap ? few : p.cap;
    if (p.cap > 32767) return XPG_ERR_UNSUPPORTED;
    const FmeLds fl = fme_lds(p.cap, p.cap, cols);
    size_t lds = fl.lds;
    p.inv_at = 0;
    if (k.inv_n > 0 && transform_inv_bytes(k.inv_n) > ((size_t)fl.cap_lds + p.cap) * cols * 8) {
        p.inv_at = (int)((fl.lds + 15) & ~(size_t)15);
        lds = (size_t)p.inv_at + transform_inv_bytes(k.inv_n);
    }
    if (lds > 160 * 1024) return XPG_ERR_UNSUPPORTED;
    p.cap_lds = fl.cap_lds;
    p.q = lineq_geom(nb, 64, lds);
    if (k.seat_is_workgroup && p.q.G != 1) return XPG_ERR_UNSUPPORTED;
    p.seats = (long long)p.q.grid * p.q.G;
    p.seat_bytes = (size_t)p.seats * k.seat_slots * (size_t)p.cap * cols * 8;
    return 0;
}
inline void plan_slots(LineqPlan & p, long long slots, long long cells, long long steps)
{
    p.slots = slots; p.steps = steps; p.out_bytes = (size_t)cells * (size_t)p.cap_out * 8;
}
// A projection of nb systems of one shape (k_fme_chain_batch): one result per system.
inline int project_plan(int nb, int rows, int cols, int cap_rows, int cap_out_rows, LineqPlan & p)
{
    if (nb <= 0 || rows <= 0 || cols <= 1) return XPG_ERR_SHAPE;
    if (const int rc = lineq_plan_rule(nb, rows, cols, cap_rows, cap_out_rows, kind_chain(false, false), p)) return rc;
    plan_slots(p, nb, (long long)nb * cols, 0);
    return 0;
}
// The projection that keeps every level (k_fme_levels_batch): the walk, the seats and the geometry are the projection's, the
// results are one per system and list entry (out_bytes: the level slots).
inline int levels_plan(int nb, int rows, int cols, int n_elim, int cap_rows, int cap_out_rows, LineqPlan & p)
{
    if (n_elim <= 0) return XPG_ERR_SHAPE;
    if (n_elim > FME_CHAIN_MAX) return XPG_ERR_UNSUPPORTED;
    if (nb <= 0 || rows <= 0 || cols <= 1) return XPG_ERR_SHAPE;
    if (const int rc = lineq_plan_rule(nb, rows, cols, cap_rows, cap_out_rows, kind_chain(true, false), p)) return rc;
    plan_slots(p, (long long)nb * n_elim, (long long)nb * n_elim * cols, 0);
    return 0;
}
// A fused calcBound (k_calc_bound_batch): one result per system and variable; a system takes rhs - 1 prefix steps and
// rhs (rhs - 1) / 2 tail steps.
inline int bounds_plan(int nb, int rows, int cols, int rhs, int cap_rows, int cap_out_rows, LineqPlan & p)
{
    if (nb <= 0 || rows <= 0 || cols <= 1 || rhs < 1 || rhs >= cols) return XPG_ERR_SHAPE;
    if (const int rc = lineq_plan_rule(nb, rows, cols, cap_rows, cap_out_rows, kind_bounds(false), p)) return rc;
    plan_slots(p, (long long)nb * rhs, (long long)nb * rhs * cols, (long long)(rhs - 1) * (rhs + 2) / 2);
    return 0;
}

// Transformed nests (k_transform_levels_batch): levels_plan with n_elim = rhs - 1, which may be 0, and rhs slots a system --
// the transformed nest itself, then one per step. A level's slot holds at least the nest's rows: the default min(cap, 4 * rows +
// 16) does, an explicit cap_out_rows under rows is refused. The inverse's scratch: PlanKind's inv_n.
inline int transform_plan(int nb, int rows, int cols, int rhs, int cap_rows, int cap_out_rows, LineqPlan & p)
{
    if (nb <= 0 || rows <= 0 || cols <= 1 || rhs < 1 || rhs >= cols) return XPG_ERR_SHAPE;
    if (rhs - 1 > FME_CHAIN_MAX) return XPG_ERR_UNSUPPORTED;
    if (cap_out_rows > 0 && cap_out_rows < rows) return XPG_ERR_SHAPE;
    if (const int rc = lineq_plan_rule(nb, rows, cols, cap_rows, cap_out_rows, kind_transform(rhs), p)) return rc;
    plan_slots(p, (long long)nb * rhs, (long long)nb * rhs * cols, 0);
    return 0;
}

// ---- THE route record: what the calling thread's last call of a family did (xpg_lineq_*_last_route) ---------------------------
// One record type, one thread_local record per family (they are independent: a caller reads one after calling another). A call
// clears its family's record when it begins and writes it once its launch is enqueued; the shared pieces below (the enqueue
// functions, the ways up and down) write none -- the hull calls launch the ragged kernels and leave the ragged records alone.
// plan_figures turns a plan into the figures; the launch site and the family's xpg_test_lineq_*_plan view both call it, the view
// showing the capacities the plan settled on behind the route's figures:
//   family          the route's figures                                                         the view adds
//   PROJECT         launches (1) grid groups sys_lds cap_lds seat_bytes                         cap cap_out
//   LEVELS          the same six, level_bytes (bytes of the level slots)                        cap cap_out
//   RAGGED          the same six, out_bytes (bytes of the output slots)                         cap cap_out cols rows (the envelope)
//   BOUNDS          the same six, steps (elimination steps per system)                          cap cap_out
//   BOUNDS_RAGGED   the same six, out_bytes, steps (of the whole batch)                         cap cap_out cols rows
//   TRANSFORM       the same six, level_bytes (bytes of the level slots, rhs a system)             cap cap_out inv_at
//   HULL            producer launches (1), k_group_reduce launches (1), its grid and LDS bytes   cap cap_out cap_hull lds_rows ecols
//                   per workgroup, groups at home in LDS / in a device slot, bytes of the         (hull_figures, lineq_hull_host.hip.h;
//                   producer's seats / of the device slots / of the output slots, and the         the view has no `gathered`)
//                   rows gathered over all groups (counted after the call; not a plan figure)
// groups: systems per workgroup; sys_lds: LDS bytes per system; seat_bytes: bytes of seat slots the launch was given.
enum { ROUTE_PROJECT, ROUTE_LEVELS, ROUTE_RAGGED, ROUTE_BOUNDS, ROUTE_BOUNDS_RAGGED, ROUTE_HULL, ROUTE_TRANSFORM, ROUTE_FAMILIES };
enum { ROUTE_MAX = 10, FIGURES_MAX = 16 };
struct LineqRoute { long long f[ROUTE_MAX]; };
const int ROUTE_FIGURES[ROUTE_FAMILIES] = {6, 7, 7, 7, 8, 10, 7};
inline LineqRoute & lineq_route(int family) { static thread_local LineqRoute r[ROUTE_FAMILIES] = {}; return r[family]; }
inline void route_clear(int family) { lineq_route(family) = LineqRoute(); }
inline void route_write(int family, const long long * f)
{
    for (int k = 0; k < ROUTE_FIGURES[family]; k++) lineq_route(family).f[k] = f[k];
}
inline int figures_out(long long * out, int n, const long long * f, int have)
{
    for (int k = 0; k < n && k < have; k++) out[k] = f[k];
    return 0;
}
inline int route_out(int family, long long * out, int n)
{
    return out && n >= 0 ? figures_out(out, n, lineq_route(family).f, ROUTE_FIGURES[family]) : XPG_ERR_SHAPE;
}
// The figures of a plan (the table above, the hull's row apart): the route's, then the view's. Returns how many there are.
inline int plan_figures(int family, const LineqPlan & p, long long * f)
{
    const bool ragged = family == ROUTE_RAGGED || family == ROUTE_BOUNDS_RAGGED;
    int n = 0;
    f[n++] = p.launches; f[n++] = p.q.grid; f[n++] = p.q.G; f[n++] = p.q.sys_lds; f[n++] = p.cap_lds; f[n++] = (long long)p.seat_bytes;
    if (family == ROUTE_LEVELS || family == ROUTE_TRANSFORM || ragged) f[n++] = (long long)p.out_bytes;
    if (family == ROUTE_BOUNDS || family == ROUTE_BOUNDS_RAGGED) f[n++] = p.steps;
    f[n++] = p.cap; f[n++] = p.cap_out;
    if (ragged) { f[n++] = p.cols; f[n++] = p.rows; }
    if (family == ROUTE_TRANSFORM) f[n++] = p.inv_at;
    return n;
}
inline void route_write(int family, const LineqPlan & p) { long long f[FIGURES_MAX]; plan_figures(family, p, f); route_write(family, f); }
// (a plan view: rc is the named rule's answer for p -- an error is the view's answer)
inline int plan_out(int family, int rc, const LineqPlan & p, long long * out, int n)
{
    long long f[FIGURES_MAX];
    return rc ? rc : figures_out(out, n, f, plan_figures(family, p, f));
}

// ---- projection: a list of variables eliminated in ONE launch (k_fme_chain_batch), and the projection that keeps every level: the
// same walk, the rows after EACH step stored (k_fme_levels_batch) ---------------------------------------------------------------
inline int project_check(int cols, int rhs, const int32_t * elim, int n_elim)
{
    if (cols <= 1 || rhs < 1 || rhs >= cols || !elim || n_elim <= 0) return XPG_ERR_SHAPE;
    for (int k = 0; k < n_elim; k++) if (elim[k] < 0 || elim[k] >= rhs) return XPG_ERR_SHAPE;
    return n_elim > FME_CHAIN_MAX ? XPG_ERR_UNSUPPORTED : 0;
}
// Device arrays, enqueue only; `p` is the plan of what was launched (launches == 0: nothing). Projection: d_outs
// [nb][cap_out_rows][cols] receives the live rows of each result (nothing behind them), d_rows [nb]. Levels: d_outs
// [nb][n_elim][cap_out_rows][cols], level k of system b in slot (b, k), d_rows [nb][n_elim]. d_ok / d_steps [nb] as the kernels
// write them. The seats' slots are the handle's (grow-only, one area for both). The row stride of d_outs is the caller's, who laid
// d_outs out with it: cap_rows < rows or cap_out_rows > cap_rows is XPG_ERR_SHAPE, nothing is defaulted or clamped but (projection)
// cap_out_rows <= 0, which stands for cap_rows; levels refuse that too.
inline int chain_batch_enqueue(xpg_ctx * ctx, bool levels, int nb, const R32 * d_mats, int rows, int cols, int rhs, const int32_t * elim,
                               int n_elim, int darkshadow, int cap_rows, int cap_out_rows, R32 * d_outs, int32_t * d_rows, int32_t * d_ok,
                               int32_t * d_steps, LineqPlan & p)
{
    p = LineqPlan();
    if (const int rc = project_check(cols, rhs, elim, n_elim)) return rc;          // the list's rules first: they need no handle
    if (!ctx || nb < 0 || !d_mats || !d_outs || rows <= 0 || !d_rows || !d_ok || !d_steps) return XPG_ERR_SHAPE;
    if (cap_rows < rows || cap_out_rows > cap_rows || (levels && cap_out_rows <= 0)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    if (levels && (long long)nb * n_elim > INT_MAX) return XPG_ERR_UNSUPPORTED;
    LineqPlan q;
    if (const int rc = levels ? levels_plan(nb, rows, cols, n_elim, cap_rows, cap_out_rows, q) : project_plan(nb, rows, cols, cap_rows, cap_out_rows, q))
        return rc;
    Scratch & slots = ctx->scratch[SCRATCH_LINEQ_PROJECT];
    if (const int rc = scratch_reserve(ctx, slots, q.seat_bytes, q.seat_bytes, levels ? "hipMalloc(lineq_levels seats)" : "hipMalloc(lineq_project seats)"))
        return rc;
    ElimList el;
    el.n = n_elim;
    for (int k = 0; k < FME_CHAIN_MAX; k++) el.u[k] = k < n_elim ? elim[k] : 0;
    const auto kernel = levels ? k_fme_levels_batch : k_fme_chain_batch;
    XPG_TRY(lds_limit((const void *)kernel, ctx->device, q.q.lds));
    hipLaunchKernelGGL(kernel, dim3(q.q.grid), q.q.block, q.q.lds, ctx->stream, nb, d_mats, rows, cols, rhs, el, darkshadow, (R32 *)slots.buf,
                       q.cap, d_outs, q.cap_out, (int *)d_rows, (int *)d_ok, (int *)d_steps, q.cap_lds, q.q.sys_lds);
    XPG_TRY(hipGetLastError());
    p = q;
    return 0;
}
inline int lineq_chain_batch_dev(xpg_ctx * ctx, bool levels, int nb, const R32 * d_mats, int rows, int cols, int rhs, const int32_t * elim,
                                 int n_elim, int darkshadow, int cap_rows, int cap_out_rows, R32 * d_outs, int32_t * d_rows, int32_t * d_ok,
                                 int32_t * d_steps)
{
    const int family = levels ? ROUTE_LEVELS : ROUTE_PROJECT;
    route_clear(family);
    LineqPlan p;
    const int rc = chain_batch_enqueue(ctx, levels, nb, d_mats, rows, cols, rhs, elim, n_elim, darkshadow, cap_rows, cap_out_rows, d_outs, d_rows,
                                       d_ok, d_steps, p);
    if (rc == 0) route_write(family, p);
    return rc;
}
// Host arrays with a PACKED result, as lineq_fme_batch_packed: one upload (packed_up), the one launch, and packed_rows_down --
// k_rows_scan / k_pack_rows and one synchronisation before the rows come down (none after it where the slots are small enough to
// come down with the counts). Projection: row_offsets [nb + 1]. Levels: row_offsets [nb * n_elim + 1], entry b * n_elim + k where
// level k of system b starts (the layout of lineq_bounds_batch_packed). A system that ends with out_ok <= 0 contributes no rows (at
// any level); the others are packed all the same. XPG_ERR_SHAPE when `out` holds fewer than the rows needed (row_offsets, out_ok
// and out_steps are filled); neither out nor view: a sizing call.
inline int lineq_chain_batch_packed(xpg_ctx * ctx, bool levels, int nb, const R32 * mats, int rows, int cols, int rhs, const int32_t * elim,
                                    int n_elim, int darkshadow, int cap_rows, int cap_out_rows, R32 * out, long long out_cap_rows,
                                    const R32 ** view, long long * row_offsets, int32_t * out_ok, int32_t * out_steps)
{
    const int family = levels ? ROUTE_LEVELS : ROUTE_PROJECT;
    if (view) *view = 0;
    route_clear(family);
    if (const int rc = project_check(cols, rhs, elim, n_elim)) return rc;          // the list's rules first: they need no handle
    if (!ctx || nb < 0 || !mats || rows <= 0 || !row_offsets || !out_ok || !out_steps || (out && out_cap_rows < 0)) return XPG_ERR_SHAPE;
    if (nb == 0) { row_offsets[0] = 0; return 0; }
    LineqPlan p;
    if (const int rc = levels ? levels_plan(nb, rows, cols, n_elim, cap_rows, cap_out_rows, p) : project_plan(nb, rows, cols, cap_rows, cap_out_rows, p))
        return rc;
    if (p.slots > INT_MAX) return XPG_ERR_UNSUPPORTED;
    PackedUp u;
    if (const int rc = packed_up(ctx, nb, mats, rows, cols, (int)p.slots, 2, p.out_bytes, false, false, u)) return rc;
    if (const int rc = chain_batch_enqueue(ctx, levels, nb, (const R32 *)u.di.p, rows, cols, rhs, elim, n_elim, darkshadow, p.cap, p.cap_out,
                                           (R32 *)u.dout.p, u.d_rows(), u.d_verdict(0), u.d_verdict(1), p)) return rc;
    route_write(family, p);
    int32_t * const verdicts[2] = {out_ok, out_steps};
    return packed_rows_down(ctx, u, cols, p.cap_out, (const char *)0, out, out_cap_rows, view, row_offsets, verdicts, no_lap);
}

// ---- limits of transformed loop nests: T^-1, A * T^-1 and every level in one launch of k_transform_levels_batch -------------------
// What both forms refuse before they look at the handle: rhs_idx outside [1, cols), a mode that is neither 0 nor 1.
inline int transform_check(int cols, int rhs, int mode)
{
    return cols <= 1 || rhs < 1 || rhs >= cols || (mode != 0 && mode != 1) ? XPG_ERR_SHAPE : 0;
}
// Device arrays, enqueue only; `p` is the plan of what was launched (launches == 0: nothing). d_nests [nb][rows][cols], or one
// rows x cols nest where shared_nest; d_tmats [nb][rhs][rhs]; d_outs [nb][rhs][cap_out_rows][cols], level 0 the transformed nest;
// d_rows [nb][rhs]; d_ok / d_steps / d_kind [nb]; d_det [nb] (written in mode 0 only); d_mult [nb][rhs][rhs]. The capacities are
// the caller's, as chain_batch_enqueue states them for the levels, and a level's slot holds the nest: cap_out_rows < rows is
// XPG_ERR_SHAPE. The seats' slots are the projection's.
inline int transform_enqueue(xpg_ctx * ctx, int nb, const R32 * d_nests, int shared_nest, const R32 * d_tmats, int rows, int cols, int rhs,
                             int mode, int cap_rows, int cap_out_rows, R32 * d_outs, int32_t * d_rows, int32_t * d_ok, int32_t * d_steps,
                             int32_t * d_kind, R32 * d_det, R32 * d_mult, LineqPlan & p)
{
    p = LineqPlan();
    if (const int rc = transform_check(cols, rhs, mode)) return rc;
    if (!ctx || nb < 0 || rows <= 0 || !d_outs || !d_rows || !d_ok || !d_steps || !d_kind || !d_mult || (mode == 0 && !d_det)) return XPG_ERR_SHAPE;
    if (nb > 0 && (!d_nests || !d_tmats)) return XPG_ERR_SHAPE;
    if (cap_rows < rows || cap_out_rows > cap_rows || cap_out_rows < rows) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    if ((long long)nb * rhs > INT_MAX) return XPG_ERR_UNSUPPORTED;
    LineqPlan q;
    if (const int rc = transform_plan(nb, rows, cols, rhs, cap_rows, cap_out_rows, q)) return rc;
    Scratch & slots = ctx->scratch[SCRATCH_LINEQ_PROJECT];
    if (const int rc = scratch_reserve(ctx, slots, q.seat_bytes, q.seat_bytes, "hipMalloc(lineq_transform seats)")) return rc;
    XPG_TRY(lds_limit((const void *)k_transform_levels_batch, ctx->device, q.q.lds));
    hipLaunchKernelGGL(k_transform_levels_batch, dim3(q.q.grid), q.q.block, q.q.lds, ctx->stream, nb, d_nests, shared_nest ? 1 : 0, d_tmats,
                       rows, cols, rhs, mode, (R32 *)slots.buf, q.cap, d_outs, q.cap_out, (int *)d_rows, (int *)d_ok, (int *)d_steps,
                       (int *)d_kind, d_det, d_mult, q.cap_lds, q.inv_at, q.q.sys_lds);
    XPG_TRY(hipGetLastError());
    p = q;
    return 0;
}
inline int lineq_transform_batch_dev(xpg_ctx * ctx, int nb, const R32 * d_nests, int shared_nest, const R32 * d_tmats, int rows, int cols,
                                     int rhs, int mode, int cap_rows, int cap_out_rows, R32 * d_outs, int32_t * d_rows, int32_t * d_ok,
                                     int32_t * d_steps, int32_t * d_kind, R32 * d_det, R32 * d_mult)
{
    route_clear(ROUTE_TRANSFORM);
    LineqPlan p;
    const int rc = transform_enqueue(ctx, nb, d_nests, shared_nest, d_tmats, rows, cols, rhs, mode, cap_rows, cap_out_rows, d_outs, d_rows, d_ok,
                                     d_steps, d_kind, d_det, d_mult, p);
    if (rc == 0) route_write(ROUTE_TRANSFORM, p);
    return rc;
}
// Host arrays with a PACKED result, as lineq_chain_batch_packed: the nests (one where shared_nest) and the transformations go up
// as one block (packed_up_bytes), the one launch, and packed_rows_down with its one synchronisation before the rows come down.
// row_offsets [nb * rhs + 1], entry b * rhs + k where level k of system b starts, level 0 the transformed nest. The determinants
// and the multipliers come down through the handle's second pinned buffer under the same synchronisation; out_det is written in
// mode 0 only. A buffer too small (XPG_ERR_SHAPE) still gets its offsets, verdicts, determinants and multipliers.
inline int lineq_transform_batch_packed(xpg_ctx * ctx, int nb, const R32 * nests, int shared_nest, const R32 * tmats, int rows, int cols,
                                        int rhs, int mode, int cap_rows, int cap_out_rows, R32 * out, long long out_cap_rows,
                                        const R32 ** view, long long * row_offsets, int32_t * out_ok, int32_t * out_steps,
                                        int32_t * out_kind, R32 * out_det, R32 * out_mult)
{
    if (view) *view = 0;
    route_clear(ROUTE_TRANSFORM);
    if (const int rc = transform_check(cols, rhs, mode)) return rc;
    if (!ctx || nb < 0 || rows <= 0 || !row_offsets || !out_ok || !out_steps || !out_kind || !out_mult || (mode == 0 && !out_det) ||
        (out && out_cap_rows < 0) || (nb > 0 && (!nests || !tmats)))
        return XPG_ERR_SHAPE;
    if (nb == 0) { row_offsets[0] = 0; return 0; }
    LineqPlan p;
    if (const int rc = transform_plan(nb, rows, cols, rhs, cap_rows, cap_out_rows, p)) return rc;
    if (p.slots > INT_MAX) return XPG_ERR_UNSUPPORTED;
    const size_t b_nests = (size_t)(shared_nest ? 1 : nb) * rows * cols * 8, b_t = (size_t)nb * rhs * rhs * 8, b_det = (size_t)nb * 8;
    PackedUp u;
    if (const int rc = packed_up_bytes(ctx, nb, nests, b_nests, tmats, b_t, (int)p.slots, 3, p.out_bytes, false, false, u)) return rc;
    DevBuf dmore;                                                  // determinants [nb], then multipliers [nb][rhs][rhs]
    XPG_TRY(dmore.alloc(ctx, b_det + b_t));
    if (const int rc = hpack_reserve(ctx, b_det + b_t, true)) return rc;
    XPG_TRY(hipMemsetAsync(dmore.p, 0, b_det + b_t, ctx->stream));    // (a system of kind 1 or 2 has no multiplier: zeros)
    if (const int rc = transform_enqueue(ctx, nb, (const R32 *)u.di.p, shared_nest, (const R32 *)((char *)u.di.p + b_nests), rows, cols, rhs, mode,
                                         p.cap, p.cap_out, (R32 *)u.dout.p, u.d_rows(), u.d_verdict(0), u.d_verdict(1), u.d_verdict(2),
                                         (R32 *)dmore.p, (R32 *)((char *)dmore.p + b_det), p)) return rc;
    route_write(ROUTE_TRANSFORM, p);
    char * const hmore = hpack_buf(ctx, true);
    XPG_TRY(hipMemcpyAsync(hmore, dmore.p, b_det + b_t, hipMemcpyDeviceToHost, ctx->stream));
    int32_t * const verdicts[3] = {out_ok, out_steps, out_kind};
    const int rc = packed_rows_down(ctx, u, cols, p.cap_out, (const char *)0, out, out_cap_rows, view, row_offsets, verdicts, no_lap);
    if (rc == 0 || rc == XPG_ERR_SHAPE) {
        if (mode == 0) memcpy(out_det, hmore, b_det);
        memcpy(out_mult, hmore + b_det, b_t);
    }
    return rc;
}

// ---- projection / levels for systems of MIXED shapes and lists: one launch of k_fme_chain_ragged ---------------------------------
// The plan of a ragged call, decided before anything is launched: every system's list under project_check's rules (a shape error
// anywhere wins over a list too long anywhere, as inside one list), then the ENVELOPE -- the widest system's cols, the capacities
// of the system with the most rows -- under the rule of project_plan / levels_plan, so that a batch whose shapes all agree gets
// exactly the uniform plan. The output slots follow the systems, cap_out x OWN cols cells each: one per system, or (levels) one
// per list entry.
//   rhs_idx NULL: the last column of each system. elim_offsets [nb + 1], elim_offsets[0] == 0, system b's list is
//   elim[elim_offsets[b] .. elim_offsets[b + 1]).
inline int ragged_chain_plan(int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx, const int32_t * elim,
                             const int32_t * elim_offsets, bool levels, int cap_rows, int cap_out_rows, LineqPlan & p)
{
    if (nb <= 0 || !rows || !cols || !elim_offsets || elim_offsets[0] != 0) return XPG_ERR_SHAPE;
    bool too_long = false;
    long long cells = 0;
    int erows = 0, ecols = 0;
    for (int b = 0; b < nb; b++) {
        if (rows[b] <= 0 || elim_offsets[b + 1] < elim_offsets[b]) return XPG_ERR_SHAPE;
        const int n = elim_offsets[b + 1] - elim_offsets[b];
        const int rc = project_check(cols[b], rhs_idx ? rhs_idx[b] : cols[b] - 1, elim ? elim + elim_offsets[b] : elim, n);
        if (rc == XPG_ERR_SHAPE) return rc;
        too_long |= rc != 0;
        if (cols[b] > ecols) ecols = cols[b];
        if (rows[b] > erows) erows = rows[b];
        cells += (long long)(levels ? n : 1) * cols[b];
    }
    if (too_long) return XPG_ERR_UNSUPPORTED;
    if (const int rc = lineq_plan_rule(nb, erows, ecols, cap_rows, cap_out_rows, kind_chain(levels, true), p)) return rc;
    plan_slots(p, levels ? elim_offsets[nb] : nb, cells, 0);
    return 0;
}
// The block a ragged packed call (chain, levels, calcBound, hull) sends up, and the buffers of its way down. ONE upload:
// [descriptors][lists: nlist entries of `elim`, none where nlist == 0][the systems, gathered back to back], built in the handle's
// pinned buffer behind meta_bytes kept for what comes down first (ragged_meta of the results that come down) and, with small
// slots, in front of room for the slots themselves. list(b, at, n, per), asked once per system in order, gives the descriptor's
// list_at and list_n and the number of result slots of system b (cap_out x OWN cols cells each, following the systems' order:
// out_off). dints: rows [nres], then nv verdict arrays [nb].
struct RaggedUp {
    DevBuf dup, dout, dints, dcells, doff;
    int nb, nres, nv, cap_out; size_t up_al, meta_al, bo; bool small_out;
    RaggedSys * hd; const RaggedSys * d_sys; const int * d_lists; const R32 * d_mats;
    int * d_rows() const { return (int *)dints.p; }
    int * d_verdict(int v) const { return (int *)dints.p + nres + (size_t)v * nb; }
};
// cell offsets [nres + 1], then the ints as on the device: counts [nres] and nv verdict arrays [n]
inline size_t ragged_meta(int nres, int n, int nv) { return (size_t)(nres + 1) * 8 + ((size_t)nres + (size_t)n * nv) * 4; }
template <class List>
inline int ragged_up(xpg_ctx * ctx, int nb, const R32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                     const int32_t * rhs_idx, const int32_t * elim, int nlist, List list, int nres, int nv, int cap_out, size_t out_bytes,
                     size_t meta_bytes, RaggedUp & u)
{
    const size_t b_desc = (size_t)nb * sizeof(RaggedSys), b_list = ((size_t)nlist * 4 + 7) & ~(size_t)7;
    size_t in_cells = 0;
    for (int b = 0; b < nb; b++) in_cells += (size_t)rows[b] * cols[b];
    const size_t b_up = b_desc + b_list + in_cells * 8;
    u.nb = nb; u.nres = nres; u.nv = nv; u.cap_out = cap_out; u.bo = out_bytes;
    u.up_al = (b_up + 255) & ~(size_t)255; u.meta_al = (meta_bytes + 255) & ~(size_t)255;
    u.small_out = u.bo <= ((size_t)512 << 10);
    XPG_TRY(u.dup.alloc(ctx, b_up)); XPG_TRY(u.dout.alloc(ctx, u.bo)); XPG_TRY(u.dints.alloc(ctx, (size_t)(nres + nv * (size_t)nb) * 4));
    XPG_TRY(u.dcells.alloc(ctx, (size_t)nres * 4)); XPG_TRY(u.doff.alloc(ctx, (size_t)(nres + 1) * 8));
    if (const int rc = hpack_reserve(ctx, u.meta_al + u.up_al + (u.small_out ? u.bo : 0))) return rc;
    char * hup = hpack_buf(ctx, false) + u.meta_al;
    u.hd = (RaggedSys *)hup;
    long long in_at = 0, out_at = 0;
    for (int b = 0; b < nb; b++) {
        int at, n, per;
        list(b, at, n, per);
        const size_t c = (size_t)rows[b] * cols[b];
        u.hd[b] = RaggedSys{in_at, out_at, rows[b], cols[b], rhs_idx ? rhs_idx[b] : cols[b] - 1, at, n, 0};
        memcpy(hup + b_desc + b_list + (size_t)in_at * 8, (const void *)(mats + offsets[b]), c * 8);
        in_at += (long long)c;
        out_at += (long long)per * cap_out * cols[b];
    }
    if (nlist) memcpy(hup + b_desc, elim, (size_t)nlist * 4);
    XPG_TRY(hipMemcpyAsync(u.dup.p, hup, b_up, hipMemcpyHostToDevice, ctx->stream));
    u.d_sys = (const RaggedSys *)u.dup.p;
    u.d_lists = (const int *)((char *)u.dup.p + b_desc);
    u.d_mats = (const R32 *)((char *)u.dup.p + b_desc + b_list);
    return 0;
}
// What a ragged way down brings, said by the call that launched: the n descriptors whose out_off / list_at / list_n place the
// results in the slot buffer, on the host and on the device (the systems of a ragged call; the GROUPS of a hull call, whose
// regions are the members' slots), the slot buffer and its bytes, the ints (counts [nres], then nv verdict arrays [n]) with the
// scratch of the scan (dcells [nres], doff [nres + 1]), cap_out, and where the slots sit in the pinned block when they are small
// enough to come down whole.
struct RaggedDown {
    const RaggedSys * hd, * d_sys; const DevBuf * dout; size_t bo; const DevBuf * dints, * dcells, * doff;
    int nres, nv, cap_out; size_t slots_at; bool small_out;
};
inline RaggedDown ragged_down(const RaggedUp & u)
{
    const RaggedDown d = {u.hd, u.d_sys, &u.dout, u.bo, &u.dints, &u.dcells, &u.doff, u.nres, u.nv, u.cap_out, u.meta_al + u.up_al, u.small_out};
    return d;
}
// The way down of a ragged packed call, after its kernel is enqueued: one synchronisation before the rows travel. With small
// slots they come down with the counts and are packed here; else k_ragged_cells / k_rows_scan give the offsets under that
// synchronisation and k_pack_ragged sends the live cells alone. per_entry: a descriptor has list_n results, the first at list_at
// (levels, calcBound: the kernels' levels mode); else one, result b. cols [n]: the width of each descriptor's results. verdicts:
// the d.nv arrays [n] that follow the counts.
inline int ragged_rows_down(xpg_ctx * ctx, int n, const int32_t * cols, const RaggedDown & d, bool per_entry, R32 * outs, long long outs_cap_cells,
                            const R32 ** view, long long * out_cell_offsets, int32_t * out_rows, int32_t * const * verdicts)
{
    const int nres = d.nres;
    char * hp = hpack_buf(ctx, false);
    long long * h_off = (long long *)hp;
    int32_t * h_ints = (int32_t *)(hp + (size_t)(nres + 1) * 8);
    XPG_TRY(hipMemcpyAsync(h_ints, d.dints->p, (size_t)(nres + d.nv * (size_t)n) * 4, hipMemcpyDeviceToHost, ctx->stream));
    const auto verdicts_out = [&]() {
        memcpy(out_rows, h_ints, (size_t)nres * 4);
        for (int v = 0; v < d.nv; v++) memcpy(verdicts[v], h_ints + nres + (size_t)v * n, (size_t)n * 4);
    };
    if (d.small_out) {
        char * hs = hp + d.slots_at;
        XPG_TRY(hipMemcpyAsync(hs, d.dout->p, d.bo, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        verdicts_out();
        long long tot = 0;
        for (int b = 0; b < n; b++)
            for (int k = 0, first = per_entry ? d.hd[b].list_at : b; k < (per_entry ? d.hd[b].list_n : 1); k++) {
                out_cell_offsets[first + k] = tot; tot += (long long)out_rows[first + k] * cols[b];
            }
        out_cell_offsets[nres] = tot;
        if (outs && outs_cap_cells < tot) return XPG_ERR_SHAPE;
        for (int b = 0; b < n; b++)                                  // forward moves: a destination never lies above its source
            for (int k = 0, first = per_entry ? d.hd[b].list_at : b; k < (per_entry ? d.hd[b].list_n : 1); k++) {
                const char * src = hs + ((size_t)d.hd[b].out_off + (size_t)k * d.cap_out * cols[b]) * 8;
                const size_t nbytes = (size_t)(out_cell_offsets[first + k + 1] - out_cell_offsets[first + k]) * 8;
                if (outs) memcpy((char *)outs + (size_t)out_cell_offsets[first + k] * 8, src, nbytes);
                if (view) memmove(hs + (size_t)out_cell_offsets[first + k] * 8, src, nbytes);
            }
        if (view && tot > 0) *view = (const R32 *)hs;
        return 0;
    }
    hipLaunchKernelGGL(k_ragged_cells, dim3((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024), dim3(256), 0, ctx->stream, n, d.d_sys, per_entry ? 1 : 0,
                       (const int *)d.dints->p, (int *)d.dcells->p);
    hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(1024), 0, ctx->stream, nres, (const int *)d.dcells->p, (long long *)d.doff->p);
    XPG_TRY(hipGetLastError());
    XPG_TRY(hipMemcpyAsync(h_off, d.doff->p, (size_t)(nres + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    verdicts_out();
    memcpy(out_cell_offsets, h_off, (size_t)(nres + 1) * 8);
    const long long total = out_cell_offsets[nres];
    if (outs && outs_cap_cells < total) return XPG_ERR_SHAPE;
    if (total == 0 || (!outs && !view)) return 0;                    // (neither: a sizing call)
    const size_t bp = (size_t)total * 8;
    DevBuf dpk;
    XPG_TRY(dpk.alloc(ctx, bp));
    hipLaunchKernelGGL(k_pack_ragged, dim3(n < 4096 ? n : 4096), dim3(256), 0, ctx->stream, n, d.d_sys, per_entry ? 1 : 0, (const R32 *)d.dout->p,
                       d.cap_out, (const int *)d.dcells->p, (const long long *)d.doff->p, (R32 *)dpk.p);
    XPG_TRY(hipGetLastError());
    if (view) {                                                      // into pinned memory; the caller's copy, if any, from there
        if (const int rc = hpack_reserve(ctx, bp)) return rc;
        char * hv = hpack_buf(ctx, false);
        XPG_TRY(hipMemcpyAsync(hv, dpk.p, bp, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        if (outs) memcpy(outs, hv, bp);
        *view = (const R32 *)hv;
    } else {
        XPG_TRY(hipMemcpyAsync(outs, dpk.p, bp, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}
// THE launch of k_fme_chain_ragged<KEEP_LEVELS> and of k_calc_bound_ragged (enqueue only, no route record: the ragged packed
// calls and the hull call both launch through them): the systems of `up` under plan p, the seats at `seats` (reserved by the
// caller before anything of the call is enqueued), the results into up.dout, the counts and verdicts into up.dints in the order
// the ways down read them -- ok, steps; ok, chain, steps.
template <bool KEEP_LEVELS>
inline int chain_ragged_enqueue(xpg_ctx * ctx, const LineqPlan & p, const RaggedUp & up, int darkshadow, void * seats)
{
    XPG_TRY(lds_limit((const void *)k_fme_chain_ragged<KEEP_LEVELS>, ctx->device, p.q.lds));
    hipLaunchKernelGGL(k_fme_chain_ragged<KEEP_LEVELS>, dim3(p.q.grid), p.q.block, p.q.lds, ctx->stream, up.nb, up.d_sys, up.d_lists, up.d_mats,
                       darkshadow, (R32 *)seats, p.cap, p.cols, (R32 *)up.dout.p, p.cap_out, up.d_rows(), up.d_verdict(0), up.d_verdict(1), p.cap_lds);
    XPG_TRY(hipGetLastError());
    return 0;
}
inline int calc_bound_ragged_enqueue(xpg_ctx * ctx, const LineqPlan & p, const RaggedUp & up, void * seats)
{
    XPG_TRY(lds_limit((const void *)k_calc_bound_ragged, ctx->device, p.q.lds));
    hipLaunchKernelGGL(k_calc_bound_ragged, dim3(p.q.grid), p.q.block, p.q.lds, ctx->stream, up.nb, up.d_sys, up.d_mats, (R32 *)seats, p.cap, p.cols,
                       (R32 *)up.dout.p, p.cap_out, up.d_rows(), up.d_verdict(0), up.d_verdict(1), up.d_verdict(2), p.cap_lds);
    XPG_TRY(hipGetLastError());
    return 0;
}
// Host arrays with a PACKED result in CELLS (the rows differ in width; the convention of xpg_lineq_fme_batch_ragged_rat32):
// out_cell_offsets [slots + 1] and out_rows [slots], slots = nb (projection: result b) or elim_offsets[nb] (levels: level k of
// system b at elim_offsets[b] + k). ONE upload (ragged_up), ONE launch, and one synchronisation before the rows travel
// (ragged_rows_down). A system with out_ok <= 0 contributes no cells, the others are packed all the same. XPG_ERR_SHAPE
// where `outs` holds fewer than out_cell_offsets[slots] cells (offsets, counts and verdicts are filled); neither outs nor
// view: a sizing call.
inline int lineq_chain_ragged_packed(xpg_ctx * ctx, int nb, const R32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                     const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, bool levels, int darkshadow,
                                     int cap_rows, int cap_out_rows, R32 * outs, long long outs_cap_cells, const R32 ** view,
                                     long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok, int32_t * out_steps)
{
    if (view) *view = 0;
    route_clear(ROUTE_RAGGED);
    if (nb < 0 || !out_cell_offsets) return XPG_ERR_SHAPE;
    if (nb == 0) { out_cell_offsets[0] = 0; return 0; }
    LineqPlan p;
    if (const int rc = ragged_chain_plan(nb, rows, cols, rhs_idx, elim, elim_offsets, levels, cap_rows, cap_out_rows, p)) return rc;
    if (!ctx || !mats || !offsets || !out_rows || !out_ok || !out_steps || (outs && outs_cap_cells < 0)) return XPG_ERR_SHAPE;
    for (int b = 0; b < nb; b++) if (offsets[b] < 0) return XPG_ERR_SHAPE;
    Scratch & seats = ctx->scratch[SCRATCH_LINEQ_PROJECT];
    if (const int rc = scratch_reserve(ctx, seats, p.seat_bytes, p.seat_bytes, "hipMalloc(lineq_ragged seats)")) return rc;
    RaggedUp up;
    const auto list = [&](int b, int & at, int & n, int & per) { at = elim_offsets[b]; n = elim_offsets[b + 1] - at; per = levels ? n : 1; };
    if (const int rc = ragged_up(ctx, nb, mats, rows, cols, offsets, rhs_idx, elim, elim_offsets[nb], list, (int)p.slots, 2, p.cap_out, p.out_bytes,
                                 ragged_meta((int)p.slots, nb, 2), up)) return rc;
    if (const int rc = levels ? chain_ragged_enqueue<true>(ctx, p, up, darkshadow, seats.buf) : chain_ragged_enqueue<false>(ctx, p, up, darkshadow, seats.buf))
        return rc;
    route_write(ROUTE_RAGGED, p);
    int32_t * const verdicts[2] = {out_ok, out_steps};
    return ragged_rows_down(ctx, nb, cols, ragged_down(up), levels, outs, outs_cap_cells, view, out_cell_offsets, out_rows, verdicts);
}

// Lineq::calcBound (linsys.cpp:1047-1078) for nb systems at once: for every variable j the
// other variables are eliminated innermost-first by chained k_fme_batch launches that stay on
// the device (ragged row counts travel in an int array). bounds is [nb][rhs][cap][cols],
// out_rows [nb][rhs]; out_ok[b] = 1, 0 (inconsistent) or -needed_rows (cap too small).
// Packed form (round 5; row_offsets != NULL): the nb * rhs results back to back -- row_offsets[b * rhs + j] is where the bounds
// of variable j of system b start (in rows), row_offsets[nb * rhs] the total -- instead of nb * rhs worst-case slots of `cap` rows:
// the slots stay in HBM, k_rows_scan / k_pack_rows compact them there (as for the packed fme), only live rows cross the link.
// `bounds` (may be NULL) has room for bounds_cap_rows rows; `view` (may be NULL) receives a pointer into the handle's pinned buffer.
inline int lineq_calc_bound_batch(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int rhs, int cap,
                                  R32 * bounds, int32_t * out_rows, int32_t * out_ok,
                                  long long * row_offsets = nullptr, long long bounds_cap_rows = 0, const R32 ** view = nullptr)
{
    const bool packed = row_offsets != nullptr;
    if (view) *view = 0;
    if (!ctx || nb < 0 || !mats || (!bounds && !packed) || rows <= 0 || cols <= 1 || rhs < 1 || rhs >= cols || cap < rows ||
        (!out_rows && !packed) || !out_ok)
        return XPG_ERR_SHAPE;
    if (nb == 0) { if (packed) row_offsets[0] = 0; return 0; }
    const FmeLds fl = fme_lds(cap, cap, cols);
    if (fl.lds > 160 * 1024 || cap > 32767) return XPG_ERR_UNSUPPORTED;
    const size_t slot = (size_t)cap * cols * 8, bsz = (size_t)nb * slot;
    DevBuf d0, da, db, ra, rb, step_ok, chain, dres, drows;
    XPG_TRY(d0.alloc(ctx, bsz)); XPG_TRY(da.alloc(ctx, bsz)); XPG_TRY(db.alloc(ctx, bsz));
    XPG_TRY(ra.alloc(ctx, (size_t)nb * 4)); XPG_TRY(rb.alloc(ctx, (size_t)nb * 4)); XPG_TRY(step_ok.alloc(ctx, (size_t)nb * 4));
    XPG_TRY(chain.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dres.alloc(ctx, bsz * rhs)); XPG_TRY(drows.alloc(ctx, (size_t)nb * rhs * 4));
    // the input, repacked to the [nb][cap][cols] slot layout
    XPG_TRY(hipMemsetAsync(d0.p, 0, bsz, ctx->stream));
    XPG_TRY(hipMemcpy2DAsync(d0.p, slot, mats, (size_t)rows * cols * 8, (size_t)rows * cols * 8, nb,
                             hipMemcpyHostToDevice, ctx->stream));
    std::vector<int32_t> ones(nb, 1), init_rows(nb, rows);
    XPG_TRY(hipMemcpyAsync(chain.p, ones.data(), (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream));
    const LineqGeom q = lineq_geom(nb, 64, fl.lds);
    XPG_TRY(lds_limit((const void *)k_fme_batch, ctx->device, q.lds));
    for (int j = 0; j < rhs; j++) {
        void * cur = d0.p; void * cur_rows = ra.p;
        XPG_TRY(hipMemcpyAsync(ra.p, init_rows.data(), (size_t)nb * 4, hipMemcpyHostToDevice, ctx->stream));
        bool flip = false;
        for (int i = rhs - 1; i >= 0; i--) {
            if (i == j) continue;
            void * nxt = flip ? da.p : db.p;
            void * nxt_rows = (cur_rows == ra.p) ? rb.p : ra.p;
            hipLaunchKernelGGL(k_fme_batch, dim3(q.grid), q.block, q.lds, ctx->stream, nb, (const R32 *)cur, cap,
                               (const int *)cur_rows, cols, rhs, i, 0, (R32 *)nxt, cap, (int *)nxt_rows,
                               (int *)step_ok.p, fl.cap_lds, (int *)chain.p, q.sys_lds);
            cur = nxt; cur_rows = nxt_rows; flip = !flip;
        }
        XPG_TRY(hipGetLastError());
        // bounds of variable j: slot j of every system
        XPG_TRY(hipMemcpy2DAsync((char *)dres.p + (size_t)j * slot, slot * rhs, cur, slot, slot, nb,
                                 hipMemcpyDeviceToDevice, ctx->stream));
        XPG_TRY(hipMemcpy2DAsync((char *)drows.p + (size_t)j * 4, (size_t)rhs * 4, cur_rows, 4, 4, nb,
                                 hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (packed) {
        const int nres = nb * rhs;
        DevBuf doff, dpk;
        XPG_TRY(doff.alloc(ctx, (size_t)(nres + 1) * 8));
        XPG_TRY(hipMemcpyAsync(out_ok, chain.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        bool short_cap = false, some_bad = false;
        for (int b = 0; b < nb; b++) { short_cap |= out_ok[b] < 0; some_bad |= out_ok[b] == 0; }
        if (short_cap) {                                           // a step needs more rows than cap (out_ok[b] = -rows needed): nothing to pack
            for (int k = 0; k <= nres; k++) row_offsets[k] = 0;
            return 0;
        }
        if (some_bad) {
            // an inconsistent system's chains hold whatever its last good step left: they count as empty
            std::vector<int32_t> hrows((size_t)nres);
            XPG_TRY(hipMemcpyAsync(hrows.data(), drows.p, (size_t)nres * 4, hipMemcpyDeviceToHost, ctx->stream));
            XPG_TRY(hipStreamSynchronize(ctx->stream));
            for (int b = 0; b < nb; b++)
                if (out_ok[b] == 0) for (int j = 0; j < rhs; j++) hrows[(size_t)b * rhs + j] = 0;
            XPG_TRY(hipMemcpyAsync(drows.p, hrows.data(), (size_t)nres * 4, hipMemcpyHostToDevice, ctx->stream));
            XPG_TRY(hipStreamSynchronize(ctx->stream));            // (hrows is about to go out of scope)
        }
        hipLaunchKernelGGL(k_rows_scan, dim3(1), dim3(1024), 0, ctx->stream, nres, (const int *)drows.p, (long long *)doff.p);
        XPG_TRY(hipMemcpyAsync(row_offsets, doff.p, (size_t)(nres + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        const long long total = row_offsets[nres];
        if (bounds && bounds_cap_rows < total) return XPG_ERR_SHAPE;
        if (total == 0 || (!bounds && !view)) return 0;
        const size_t bp = (size_t)total * cols * 8;
        XPG_TRY(dpk.alloc(ctx, bp));
        hipLaunchKernelGGL(k_pack_rows, dim3(nres < 4096 ? nres : 4096), dim3(256), 0, ctx->stream, nres, (const R32 *)dres.p, cap, cols,
                           (const int *)drows.p, (const long long *)doff.p, (R32 *)dpk.p);
        XPG_TRY(hipGetLastError());
        if (view) {
            const int rc = hpack_reserve(ctx, bp);
            if (rc) return rc;
            XPG_TRY(hipMemcpyAsync(ctx->hpack, dpk.p, bp, hipMemcpyDeviceToHost, ctx->stream));
            XPG_TRY(hipStreamSynchronize(ctx->stream));
            if (bounds) memcpy(bounds, ctx->hpack, bp);
            *view = (const R32 *)ctx->hpack;
        } else {
            XPG_TRY(hipMemcpyAsync(bounds, dpk.p, bp, hipMemcpyDeviceToHost, ctx->stream));
            XPG_TRY(hipStreamSynchronize(ctx->stream));
        }
        return 0;
    }
    XPG_TRY(hipMemcpyAsync(bounds, dres.p, bsz * rhs, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(out_rows, drows.p, (size_t)nb * rhs * 4, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(out_ok, chain.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- calcBound fused: every chain of every system in ONE launch (k_calc_bound_batch) -----------------------------------------
// Device arrays, enqueue only: d_outs [nb][rhs][cap_out_rows][cols] receives the live rows of variable j's bounds in slot
// (b, j), d_rows [nb][rhs] their counts, d_ok / d_chain / d_steps [nb] as the kernel writes them. As lineq_chain_batch_dev:
// the seats' slots are the handle's (grow-only, an area of their own), the row stride of d_outs is the caller's -- cap_rows <
// rows or cap_out_rows > cap_rows is XPG_ERR_SHAPE, only cap_out_rows <= 0 stands for cap_rows.
inline int lineq_bounds_batch_dev(xpg_ctx * ctx, int nb, const R32 * d_mats, int rows, int cols, int rhs, int cap_rows, int cap_out_rows,
                                  R32 * d_outs, int32_t * d_rows, int32_t * d_ok, int32_t * d_chain, int32_t * d_steps)
{
    route_clear(ROUTE_BOUNDS);
    if (!ctx || nb < 0 || !d_mats || !d_outs || rows <= 0 || cols <= 1 || rhs < 1 || rhs >= cols || !d_rows || !d_ok || !d_chain || !d_steps)
        return XPG_ERR_SHAPE;
    if (cap_rows < rows || cap_out_rows > cap_rows) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    LineqPlan p;
    if (const int rc = bounds_plan(nb, rows, cols, rhs, cap_rows, cap_out_rows, p)) return rc;
    Scratch & slots = ctx->scratch[SCRATCH_LINEQ_BOUNDS];
    if (const int rc = scratch_reserve(ctx, slots, p.seat_bytes, p.seat_bytes, "hipMalloc(lineq_bounds seats)")) return rc;
    XPG_TRY(lds_limit((const void *)k_calc_bound_batch, ctx->device, p.q.lds));
    hipLaunchKernelGGL(k_calc_bound_batch, dim3(p.q.grid), p.q.block, p.q.lds, ctx->stream, nb, d_mats, rows, cols, rhs, (R32 *)slots.buf,
                       p.cap, d_outs, p.cap_out, (int *)d_rows, (int *)d_ok, (int *)d_chain, (int *)d_steps, p.cap_lds, p.q.sys_lds);
    XPG_TRY(hipGetLastError());
    route_write(ROUTE_BOUNDS, p);
    return 0;
}
// Host arrays with a PACKED result in the layout of the packed calcBound: row_offsets [nb * rhs + 1], entry b * rhs + j where
// the bounds of variable j of system b start. One upload (packed_up), the one launch, packed_rows_down over the nb * rhs results
// and the three verdict arrays [nb]. A system with out_ok <= 0 contributes no rows, the others are packed all the same; out /
// view / sizing call as lineq_chain_batch_packed.
inline int lineq_bounds_batch_packed(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int rhs, int cap_rows, int cap_out_rows,
                                     R32 * out, long long out_cap_rows, const R32 ** view, long long * row_offsets, int32_t * out_ok,
                                     int32_t * out_chain, int32_t * out_steps)
{
    if (view) *view = 0;
    route_clear(ROUTE_BOUNDS);
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols <= 1 || rhs < 1 || rhs >= cols || !row_offsets || !out_ok || !out_chain || !out_steps ||
        (out && out_cap_rows < 0))
        return XPG_ERR_SHAPE;
    if (nb == 0) { row_offsets[0] = 0; return 0; }
    LineqPlan p;
    if (const int rc = bounds_plan(nb, rows, cols, rhs, cap_rows, cap_out_rows, p)) return rc;
    if (p.slots > INT_MAX) return XPG_ERR_UNSUPPORTED;
    PackedUp u;
    if (const int rc = packed_up(ctx, nb, mats, rows, cols, (int)p.slots, 3, p.out_bytes, false, false, u)) return rc;
    if (const int rc = lineq_bounds_batch_dev(ctx, nb, (const R32 *)u.di.p, rows, cols, rhs, p.cap, p.cap_out, (R32 *)u.dout.p, u.d_rows(),
                                              u.d_verdict(0), u.d_verdict(1), u.d_verdict(2))) return rc;
    int32_t * const verdicts[3] = {out_ok, out_chain, out_steps};
    return packed_rows_down(ctx, u, cols, p.cap_out, (const char *)0, out, out_cap_rows, view, row_offsets, verdicts, no_lap);
}

// ---- calcBound fused for systems of MIXED shapes: one launch of k_calc_bound_ragged -------------------------------------------
// The plan of a ragged calcBound call, decided before anything is launched: every system under bounds_plan's shape rules, then
// the ENVELOPE -- the widest system's cols, the most rows -- under bounds_plan's rule, so that a batch whose shapes all agree
// gets exactly the uniform plan. The output slots follow the systems, cap_out x OWN cols cells per variable; `steps` is the sum
// over the systems. rhs_idx NULL: the last column of each system.
inline int bounds_ragged_plan(int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx, int cap_rows, int cap_out_rows,
                              LineqPlan & p)
{
    if (nb <= 0 || !rows || !cols) return XPG_ERR_SHAPE;
    long long cells = 0, slots = 0, steps = 0;
    int erows = 0, ecols = 0;
    for (int b = 0; b < nb; b++) {
        const int rhs = rhs_idx ? rhs_idx[b] : cols[b] - 1;
        if (rows[b] <= 0 || cols[b] <= 1 || rhs < 1 || rhs >= cols[b]) return XPG_ERR_SHAPE;
        if (cols[b] > ecols) ecols = cols[b];
        if (rows[b] > erows) erows = rows[b];
        cells += (long long)rhs * cols[b];
        slots += rhs;
        steps += (long long)(rhs - 1) * (rhs + 2) / 2;
    }
    if (slots > INT_MAX) return XPG_ERR_UNSUPPORTED;
    if (const int rc = lineq_plan_rule(nb, erows, ecols, cap_rows, cap_out_rows, kind_bounds(true), p)) return rc;
    plan_slots(p, slots, cells, steps);
    return 0;
}
// Host arrays with a PACKED result in CELLS, as lineq_chain_ragged_packed gives them: out_cell_offsets [R + 1] and out_rows [R],
// R the sum of the rhs, variable j of system b at first[b] + j (first[b] the sum of the rhs before b). ONE upload (ragged_up:
// descriptors and systems, no list -- the descriptor's list_at / list_n carry first[b] / rhs), ONE launch, one synchronisation
// before the rows travel (ragged_rows_down). A system with out_ok <= 0 contributes no cells, the others are packed all the same.
// XPG_ERR_SHAPE where `outs` holds fewer than out_cell_offsets[R] cells (offsets, counts and verdicts are filled); neither
// outs nor view: a sizing call.
inline int lineq_bounds_ragged_packed(xpg_ctx * ctx, int nb, const R32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                      const int32_t * rhs_idx, int cap_rows, int cap_out_rows, R32 * outs, long long outs_cap_cells,
                                      const R32 ** view, long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok,
                                      int32_t * out_chain, int32_t * out_steps)
{
    if (view) *view = 0;
    route_clear(ROUTE_BOUNDS_RAGGED);
    if (nb < 0 || !out_cell_offsets) return XPG_ERR_SHAPE;
    if (nb == 0) { out_cell_offsets[0] = 0; return 0; }
    LineqPlan p;
    if (const int rc = bounds_ragged_plan(nb, rows, cols, rhs_idx, cap_rows, cap_out_rows, p)) return rc;
    if (!ctx || !mats || !offsets || !out_rows || !out_ok || !out_chain || !out_steps || (outs && outs_cap_cells < 0)) return XPG_ERR_SHAPE;
    for (int b = 0; b < nb; b++) if (offsets[b] < 0) return XPG_ERR_SHAPE;
    Scratch & seats = ctx->scratch[SCRATCH_LINEQ_BOUNDS];
    if (const int rc = scratch_reserve(ctx, seats, p.seat_bytes, p.seat_bytes, "hipMalloc(lineq_bounds_ragged seats)")) return rc;
    RaggedUp up;
    int first = 0;                                                   // (asked once per system, in order)
    const auto list = [&](int b, int & at, int & n, int & per) { at = first; n = per = rhs_idx ? rhs_idx[b] : cols[b] - 1; first += n; };
    if (const int rc = ragged_up(ctx, nb, mats, rows, cols, offsets, rhs_idx, (const int32_t *)0, 0, list, (int)p.slots, 3, p.cap_out, p.out_bytes,
                                 ragged_meta((int)p.slots, nb, 3), up)) return rc;
    if (const int rc = calc_bound_ragged_enqueue(ctx, p, up, seats.buf)) return rc;
    route_write(ROUTE_BOUNDS_RAGGED, p);
    int32_t * const verdicts[3] = {out_ok, out_chain, out_steps};
    return ragged_rows_down(ctx, nb, cols, ragged_down(up), true, outs, outs_cap_cells, view, out_cell_offsets, out_rows, verdicts);
}

// Matrix<Rational>::rank on device arrays, enqueue only: d_rank [nb].
inline int rat_rank_batch_dev(xpg_ctx * ctx, int nb, const R32 * d_mats, int rows, int cols, int32_t * d_rank)
{
    if (!ctx || nb < 0 || !d_mats || !d_rank || rows <= 0 || cols <= 0) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    size_t lds = ((size_t)rows * cols * 8 + 15) & ~(size_t)15;
    lds += ((size_t)rows * 13 + 15) & ~(size_t)15;           // row factors, rowpos, live flags
    if (lds > 160 * 1024) return XPG_ERR_UNSUPPORTED;
    const LineqGeom q = lineq_geom(nb, rows * cols > 256 ? 64 : cols, lds);
    XPG_TRY(lds_limit((const void *)k_gauss_batch, ctx->device, q.lds));
    hipLaunchKernelGGL(k_gauss_batch, dim3(q.grid), q.block, q.lds, ctx->stream, nb, d_mats, rows, cols, 0, 0,
                       (int *)d_rank, (R32 *)0, (R32 *)0, q.sys_lds);
    XPG_TRY(hipGetLastError());
    return 0;
}

// op 0: rank, 1: det, 2: inv, 3: rank with basis (flag = is_unitarize), 4: null space
inline int gauss_batch(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int op, int32_t * out_int,
                       R32 * out_val, R32 * out_mat, int flag = 0)
{
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols <= 0 || ((op == 1 || op == 2) && rows != cols)) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    size_t lds = ((size_t)rows * cols * 8 * (op == 2 ? 2 : 1) + 15) & ~(size_t)15;
    lds += ((size_t)rows * 13 + 15) & ~(size_t)15;           // row factors, rowpos, live flags
    if (lds > 160 * 1024) return XPG_ERR_UNSUPPORTED;
    const size_t bi = (size_t)nb * rows * cols * 8;
    const size_t bo = op == 2 || op == 3 ? bi : (op == 4 ? (size_t)nb * cols * cols * 8 : 8);
    DevBuf di, dint, dval, dmat;
    XPG_TRY(di.alloc(ctx, bi)); XPG_TRY(dint.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dval.alloc(ctx, (size_t)nb * 8));
    XPG_TRY(dmat.alloc(ctx, bo));
    XPG_TRY(hipMemcpyAsync(di.p, mats, bi, hipMemcpyHostToDevice, ctx->stream));
    if (op >= 2) XPG_TRY(hipMemsetAsync(dmat.p, 0, bo, ctx->stream));
    // small matrices share a wave (one lane per column); from a few hundred cells on the cell-parallel elimination
    // fills the wave by itself and sharing only serialises the groups' branches
    const LineqGeom q = lineq_geom(nb, rows * cols > 256 ? 64 : (op == 2 ? 2 * cols : cols), lds);
    XPG_TRY(lds_limit((const void *)k_gauss_batch, ctx->device, q.lds));
    hipLaunchKernelGGL(k_gauss_batch, dim3(q.grid), q.block, q.lds, ctx->stream, nb, (const R32 *)di.p, rows,
                       cols, op, flag, (int *)dint.p, (R32 *)dval.p, (R32 *)dmat.p, q.sys_lds);
    XPG_TRY(hipGetLastError());
    if (out_int) XPG_TRY(hipMemcpyAsync(out_int, dint.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (out_val) XPG_TRY(hipMemcpyAsync(out_val, dval.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (out_mat && op >= 2) XPG_TRY(hipMemcpyAsync(out_mat, dmat.p, bo, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// INTMat::hnf for nb matrices: h [nb][rows][cols], u [nb][cols][cols], status [nb].
inline int int_hnf_batch(xpg_ctx * ctx, int nb, const int32_t * mats, int rows, int cols, int32_t * h, int32_t * u,
                         int32_t * status)
{
    if (!ctx || nb < 0 || !mats || !h || !u || !status || rows <= 0 || cols <= 0) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const size_t lds = ((size_t)(rows + cols) * cols * 4 + 15) & ~(size_t)15;
    if (lds > 160 * 1024) return XPG_ERR_UNSUPPORTED;
    const size_t bi = (size_t)nb * rows * cols * 4, bu = (size_t)nb * cols * cols * 4;
    DevBuf di, dh, du, ds;
    XPG_TRY(di.alloc(ctx, bi)); XPG_TRY(dh.alloc(ctx, bi)); XPG_TRY(du.alloc(ctx, bu)); XPG_TRY(ds.alloc(ctx, (size_t)nb * 4));
    XPG_TRY(hipMemcpyAsync(di.p, mats, bi, hipMemcpyHostToDevice, ctx->stream));
    XPG_TRY(hipMemsetAsync(dh.p, 0, bi, ctx->stream));
    XPG_TRY(hipMemsetAsync(du.p, 0, bu, ctx->stream));
    XPG_TRY(lds_limit((const void *)k_hnf_batch, ctx->device, lds));
    hipLaunchKernelGGL(k_hnf_batch, dim3(lineq_grid(nb)), dim3(64), lds, ctx->stream, nb, (const int *)di.p, rows, cols,
                       (int *)dh.p, (int *)du.p, (int *)ds.p);
    XPG_TRY(hipGetLastError());
    XPG_TRY(hipMemcpyAsync(h, dh.p, bi, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(u, du.p, bu, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipMemcpyAsync(status, ds.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}

// INTMat::gcd for nb matrices, in place.
inline int int_gcd_batch(xpg_ctx * ctx, int nb, int32_t * mats, int rows, int cols)
{
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols <= 0) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const size_t bi = (size_t)nb * rows * cols * 4;
    const long long total = (long long)nb * rows;
    DevBuf di;
    XPG_TRY(di.alloc(ctx, bi));
    XPG_TRY(hipMemcpyAsync(di.p, mats, bi, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_int_gcd_batch, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ctx->stream, total,
                       (int *)di.p, cols);
    XPG_TRY(hipGetLastError());
    XPG_TRY(hipMemcpyAsync(mats, di.p, bi, hipMemcpyDeviceToHost, ctx->stream));
    XPG_TRY(hipStreamSynchronize(ctx->stream));
    return 0;
}



} // namespace xpg
