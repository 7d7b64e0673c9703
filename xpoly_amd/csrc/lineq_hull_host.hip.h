// Host half of the hull calls (k_group_reduce, lineq_kernels.hip.h): Lineq::ConvexHullUnionAndIntersect over many lists of
// polyhedra and the projected union of PolyTran::step_4, each as a producer launch, the group launch behind it on the same
// stream and one synchronisation. Included from api_lineq.hip only. No arithmetic here.
#pragma once
#include "lineq_host.hip.h"

namespace xpg {

// THE plan of a hull call (the launch and xpg_test_lineq_hull_plan both ask it), decided before anything is launched.
//   group_offsets [ng + 1] partitions the nb members: 0 first, monotone, nb last; the members of a group share cols and rhs_idx
//   (the reference's "homotype" assertion) -- else XPG_ERR_SHAPE. The members themselves are planned as the producer plans them:
//   bounds_ragged_plan (the hull) or ragged_chain_plan (the projected union: elim_offsets != NULL), with their error codes.
//   cap_hull   rows a group may gather, lead row included; <= 0: the largest lead + 2 x rhs x members of any group, at most 32767
//              (w_reduce indexes rows as short); > 32767: XPG_ERR_UNSUPPORTED
//   lds_rows   rows of the LDS matrix area at the envelope's width ecols: min(cap_hull, 32 KB / (ecols x 8)); the scratch beside it
//              is cap_hull's. XPG_ERR_UNSUPPORTED where the two exceed 160 KB.
//   home       of a group with members: its gathered capacity gcap = min(cap_hull, lead + slots x cap_out) rows of its OWN cols
//              in LDS where gcap x cols <= lds_rows x ecols cells, else in its workgroup's device slot (cap_hull x ecols cells;
//              allocated only where some group needs one, the grid lowered until the slots fit 1 GiB)
//   out        the producer's slots, cap_out x OWN cols cells per result, and ONE more slot behind every group that has a lead
//              row: the result of a group goes to the front of its own region and never has more rows than lead + the live rows
//              of its slots, so nothing grows with groups x cap_hull.
struct HullPlan {
    LineqPlan prod;                                                   // the producer's plan (all zero: no members, nothing is launched)
    int cap_hull, lds_rows, grid; size_t lds, slot_bytes, out_bytes; long long n_lds, n_dev;
};
enum { HULL_HOME_NONE = -1, HULL_HOME_LDS = 0, HULL_HOME_DEVICE = 1 };
inline int hull_plan(int ng, const int32_t * goff, int nb, const int32_t * rows, const int32_t * cols, const int32_t * rhs_idx,
                     const int32_t * elim, const int32_t * elim_offsets, int cap_rows, int cap_out_rows, int cap_hull_rows, HullPlan & p,
                     int32_t * homes, int32_t * gcaps)
{
    const bool is_union = elim_offsets != 0;
    if (ng <= 0 || nb < 0 || !goff || goff[0] != 0 || goff[ng] != nb) return XPG_ERR_SHAPE;
    for (int g = 0; g < ng; g++) if (goff[g + 1] < goff[g]) return XPG_ERR_SHAPE;
    p = HullPlan();
    if (nb > 0) {
        if (const int rc = is_union ? ragged_chain_plan(nb, rows, cols, rhs_idx, elim, elim_offsets, false, cap_rows, cap_out_rows, p.prod)
                                    : bounds_ragged_plan(nb, rows, cols, rhs_idx, cap_rows, cap_out_rows, p.prod)) return rc;
        p.out_bytes = p.prod.out_bytes;
    }
    const int lead = is_union ? 0 : 1;
    long long want = 1;
    for (int g = 0; g < ng; g++) {
        const int b0 = goff[g], n = goff[g + 1] - b0;
        if (n == 0) continue;
        const int rhs = rhs_idx ? rhs_idx[b0] : cols[b0] - 1;
        for (int b = b0 + 1; b < b0 + n; b++)
            if (cols[b] != cols[b0] || (rhs_idx ? rhs_idx[b] : cols[b] - 1) != rhs) return XPG_ERR_SHAPE;
        const long long w = lead + 2ll * rhs * n;
        if (w > want) want = w;
        if ((long long)n * (is_union ? 1 : rhs) * p.prod.cap_out + p.prod.cap_out > INT_MAX) return XPG_ERR_UNSUPPORTED;   // (a region's rows are ints)
        p.out_bytes += (size_t)lead * p.prod.cap_out * cols[b0] * 8;
    }
    if (cap_hull_rows > 32767) return XPG_ERR_UNSUPPORTED;
    p.cap_hull = cap_hull_rows > 0 ? cap_hull_rows : (int)(want < 32767 ? want : 32767);
    if (nb == 0) {                                                    // every group is empty: nothing is launched
        for (int g = 0; g < ng; g++) { if (homes) homes[g] = HULL_HOME_NONE; if (gcaps) gcaps[g] = 0; }
        return 0;
    }
    const int fit = 32 * 1024 / (p.prod.cols * 8) > 0 ? 32 * 1024 / (p.prod.cols * 8) : 1;
    p.lds_rows = p.cap_hull < fit ? p.cap_hull : fit;
    p.lds = (size_t)p.lds_rows * p.prod.cols * 8 + (lineq_lds_bytes(p.cap_hull, 1) - (size_t)p.cap_hull * 8) + 16;
    p.lds = (p.lds + 15) & ~(size_t)15;
    if (p.lds > 160 * 1024) return XPG_ERR_UNSUPPORTED;
    for (int g = 0; g < ng; g++) {
        const int b0 = goff[g], n = goff[g + 1] - b0;
        if (n == 0) { if (homes) homes[g] = HULL_HOME_NONE; if (gcaps) gcaps[g] = 0; continue; }
        const long long room = lead + (long long)n * (is_union ? 1 : (rhs_idx ? rhs_idx[b0] : cols[b0] - 1)) * p.prod.cap_out;
        const long long gcap = room < p.cap_hull ? room : p.cap_hull;
        const bool in_lds = gcap * cols[b0] <= (long long)p.lds_rows * p.prod.cols;
        if (in_lds) p.n_lds++; else p.n_dev++;
        if (homes) homes[g] = in_lds ? HULL_HOME_LDS : HULL_HOME_DEVICE;
        if (gcaps) gcaps[g] = (int32_t)gcap;
    }
    p.grid = lineq_grid(ng);
    const size_t one = (size_t)p.cap_hull * p.prod.cols * 8;
    if (p.n_dev) {
        const size_t most = ((size_t)1 << 30) / one;
        if ((size_t)p.grid > most) p.grid = most > 0 ? (int)most : 1;
        p.slot_bytes = (size_t)p.grid * one;
    }
    return 0;
}
// The figures of a hull plan (the HULL row of the table beside LineqRoute, lineq_host.hip.h): the route's ten -- the last,
// the rows gathered over all groups, is no plan figure: 0 here, counted by the call once the verdicts are down -- then what the
// plan view adds. The launch (route_write) and xpg_test_lineq_hull_plan (hull_plan_out) both call it.
enum { HULL_GATHERED = 9, HULL_FIGURES = 15 };
inline void hull_figures(const HullPlan & p, long long * f)
{
    const long long g[HULL_FIGURES] = { p.prod.launches, p.prod.launches, p.grid, (long long)p.lds, p.n_lds, p.n_dev, (long long)p.prod.seat_bytes,
                                        (long long)p.slot_bytes, (long long)p.out_bytes, 0, p.prod.cap, p.prod.cap_out, p.cap_hull, p.lds_rows,
                                        p.prod.cols };
    for (int k = 0; k < HULL_FIGURES; k++) f[k] = g[k];
}
inline int hull_plan_out(int rc, const HullPlan & p, long long * out, int n)   // (rc: hull_plan's answer for p; the view has no `gathered`)
{
    if (rc) return rc;
    long long f[HULL_FIGURES];
    hull_figures(p, f);
    figures_out(out, n, f, HULL_GATHERED);
    return n > HULL_GATHERED ? figures_out(out + HULL_GATHERED, n - HULL_GATHERED, f + HULL_GATHERED + 1, HULL_FIGURES - HULL_GATHERED - 1) : 0;
}

// Host arrays in, a PACKED result in CELLS out, one entry per GROUP: out_cell_offsets [ng + 1], out_rows [ng] and the verdicts
// [ng] as k_group_reduce writes them. ONE upload (ragged_up: the members' descriptors, the lists of a projected union with the
// groups' descriptors behind them in the block's list area, the systems), the producer launch, k_group_reduce behind it, one
// synchronisation before the rows travel (ragged_rows_down over the groups: a group's region begins with its result).
inline int lineq_hull_ragged_packed(xpg_ctx * ctx, int ng, const int32_t * goff, int nb, const R32 * mats, const int32_t * rows,
                                    const int32_t * cols, const long long * offsets, const int32_t * rhs_idx, const int32_t * elim,
                                    const int32_t * elim_offsets, int darkshadow, int is_intersect, int cap_rows, int cap_out_rows,
                                    int cap_hull_rows, R32 * outs, long long outs_cap_cells, const R32 ** view, long long * out_cell_offsets,
                                    int32_t * out_rows, int32_t * out_ok, int32_t * out_member, int32_t * out_chain, int32_t * out_steps)
{
    const bool is_union = elim_offsets != 0;
    if (view) *view = 0;
    route_clear(ROUTE_HULL);
    if (ng < 0 || nb < 0 || !out_cell_offsets) return XPG_ERR_SHAPE;
    if (ng == 0) { if (nb != 0) return XPG_ERR_SHAPE; out_cell_offsets[0] = 0; return 0; }
    HullPlan p;
    if (const int rc = hull_plan(ng, goff, nb, rows, cols, rhs_idx, elim, elim_offsets, cap_rows, cap_out_rows, cap_hull_rows, p, 0, 0)) return rc;
    if (!out_rows || !out_ok || !out_member || !out_chain || !out_steps || (outs && outs_cap_cells < 0)) return XPG_ERR_SHAPE;
    if (nb == 0) {                                                    // groups without members: 0 rows, verdict 1
        for (int g = 0; g < ng; g++) { out_cell_offsets[g] = 0; out_rows[g] = 0; out_ok[g] = 1; out_member[g] = -1; out_chain[g] = -1; out_steps[g] = 0; }
        out_cell_offsets[ng] = 0;
        return 0;
    }
    if (!ctx || !mats || !offsets) return XPG_ERR_SHAPE;
    for (int b = 0; b < nb; b++) if (offsets[b] < 0) return XPG_ERR_SHAPE;
    const int lead = is_union ? 0 : 1;
    // the groups' descriptors (k_group_reduce's reading of a RaggedSys) and the result slots every member owns: its own, and
    // the group's spare slot with the last member of a group that has a lead row
    std::vector<RaggedSys> gd((size_t)ng);
    std::vector<int32_t> per((size_t)nb), gcols((size_t)ng);
    {
        long long out_at = 0; int first = 0;
        for (int g = 0; g < ng; g++) {
            const int b0 = goff[g], n = goff[g + 1] - b0;
            const int gc = n ? cols[b0] : 2, rhs = n ? (rhs_idx ? rhs_idx[b0] : cols[b0] - 1) : 1, each = is_union ? 1 : rhs;
            gd[(size_t)g] = RaggedSys{b0, out_at, n, gc, rhs, first, each, lead};
            gcols[(size_t)g] = gc;
            for (int b = b0; b < b0 + n; b++) per[(size_t)b] = each + (lead && b == b0 + n - 1 ? 1 : 0);
            out_at += ((long long)n * each + (n ? lead : 0)) * p.prod.cap_out * gc;
            first += n * each;
        }
    }
    // the list area of the block: the lists (projected union), then the groups' descriptors on an 8-byte boundary
    const int n_elim = is_union ? elim_offsets[nb] : 0, desc_at = (n_elim + 1) & ~1, desc_ints = (int)(sizeof(RaggedSys) / 4);
    std::vector<int32_t> lists((size_t)desc_at + (size_t)ng * desc_ints, 0);
    if (n_elim) memcpy(lists.data(), elim, (size_t)n_elim * 4);
    memcpy(lists.data() + desc_at, gd.data(), (size_t)ng * sizeof(RaggedSys));
    Scratch & seats = ctx->scratch[is_union ? SCRATCH_LINEQ_PROJECT : SCRATCH_LINEQ_BOUNDS];
    if (const int rc = scratch_reserve(ctx, seats, p.prod.seat_bytes, p.prod.seat_bytes, "hipMalloc(lineq_hull seats)")) return rc;
    // everything the two launches need is allocated before the first, so that nothing stands between them
    RaggedUp up;
    DevBuf dslot, gints, gcells, goffs;                              // the workgroups' device slots; the groups' ints and scan scratch
    if (p.slot_bytes) XPG_TRY(dslot.alloc(ctx, p.slot_bytes));
    XPG_TRY(gints.alloc(ctx, (size_t)ng * 6 * 4)); XPG_TRY(gcells.alloc(ctx, (size_t)ng * 4)); XPG_TRY(goffs.alloc(ctx, (size_t)(ng + 1) * 8));
    int first = 0;                                                   // (asked once per member, in order)
    const auto list = [&](int b, int & at, int & n, int & pr) {
        if (is_union) { at = elim_offsets[b]; n = elim_offsets[b + 1] - at; }
        else { at = first; n = rhs_idx ? rhs_idx[b] : cols[b] - 1; first += n; }
        pr = per[(size_t)b];
    };
    // (what comes down first is the GROUPS': their offsets, counts and five verdict arrays; the members' ints stay on the device)
    if (const int rc = ragged_up(ctx, nb, mats, rows, cols, offsets, rhs_idx, lists.data(), (int)lists.size(), list, (int)p.prod.slots, is_union ? 2 : 3,
                                 p.prod.cap_out, p.out_bytes, ragged_meta(ng, ng, 5), up)) return rc;
    if (const int rc = is_union ? chain_ragged_enqueue<false>(ctx, p.prod, up, darkshadow, seats.buf) : calc_bound_ragged_enqueue(ctx, p.prod, up, seats.buf))
        return rc;
    // the members' verdicts as k_group_reduce reads them: ok, then (hull) chain and steps, or (projected union) steps alone
    const int * const d_chain = is_union ? (const int *)0 : up.d_verdict(1), * const d_steps = up.d_verdict(is_union ? 1 : 2);
    const RaggedSys * const d_grp = (const RaggedSys *)(up.d_lists + desc_at);
    int * const g_rows = (int *)gints.p;
    XPG_TRY(lds_limit((const void *)k_group_reduce, ctx->device, p.lds));
    hipLaunchKernelGGL(k_group_reduce, dim3(p.grid), dim3(64, 1), p.lds, ctx->stream, ng, d_grp, (R32 *)up.dout.p, p.prod.cap_out, (const int *)up.d_rows(),
                       (const int *)up.d_verdict(0), d_chain, d_steps, is_intersect, p.cap_hull, p.prod.cols, p.lds_rows * p.prod.cols,
                       (R32 *)dslot.p, g_rows, g_rows + ng, g_rows + 2 * (size_t)ng, g_rows + 3 * (size_t)ng, g_rows + 4 * (size_t)ng,
                       g_rows + 5 * (size_t)ng);
    XPG_TRY(hipGetLastError());
    long long f[HULL_FIGURES];
    hull_figures(p, f);
    route_write(ROUTE_HULL, f);
    // the way down is the ragged calls', over the GROUPS: the members' slots are the groups' regions
    RaggedDown down = ragged_down(up);
    down.hd = gd.data(); down.d_sys = d_grp; down.dints = &gints; down.dcells = &gcells; down.doff = &goffs; down.nres = ng; down.nv = 5;
    std::vector<int32_t> gath((size_t)ng, 0);
    int32_t * const verdicts[5] = {out_ok, out_member, out_chain, out_steps, gath.data()};
    const int rc = ragged_rows_down(ctx, ng, gcols.data(), down, false, outs, outs_cap_cells, view, out_cell_offsets, out_rows, verdicts);
    if (rc == 0 || rc == XPG_ERR_SHAPE) for (int g = 0; g < ng; g++) lineq_route(ROUTE_HULL).f[HULL_GATHERED] += gath[(size_t)g];
    return rc;
}

} // namespace xpg
