// The front ends on top of the MIP walk: Lineq::has_solution (src/com/linsys.cpp:830-906) and DepPoly::is_empty
// (src/eng/poly.cpp:530-573), with the two small kernels the latter runs between Lineq::reduce and the walks. A header of its
// own because the walk (mip_kernels.hip.h) and its host half (mip_host.hip.h) are included by more than one source of the
// library (api_mip.hip, api_mip_hbm.hip, api_has_solution.hip), and these -- non-template kernels and the instantiations has_solution pulls in -- belong to one.
#pragma once
#include "mip_host.hip.h"

namespace xpg {

// ---- DepPoly::is_empty (src/eng/poly.cpp:530-573) after the reduce, on the device ------------------------------
// Per polyhedron b with reduce's outputs kept[b] / ok[b]: the verdict reduce alone gives, else the feasibility
// objective of Lineq::has_solution (SIX::reviseTargetFunc on all ones, lpsol.h:2053-2074 / linsys.cpp:851-862: 1 for
// every variable that occurs in some inequality) and the "still open" mark for the MIP walks that follow.
__global__ void k_dep_prepare(int nb, const R32 * mats, int rows, int cols, const int * kept, const int * ok, R32 * tgtf,
                              int * active, int32_t * empty)
{
    const int b = blockIdx.x * blockDim.y + threadIdx.y;
    if (b >= nb) return;
    const int last = cols - 1, k = kept[b];
    const bool open = ok[b] != 0 && k > 0;
    if (threadIdx.x == 0) {
        active[b] = open ? 1 : 0;
        empty[b] = !ok[b] ? 1 : (k == 0 ? 0 : 1);       // inconsistent bounds: empty; only redundant constraints: not
    }
    const R32 * m = mats + (size_t)b * rows * cols;
    for (int j = threadIdx.x; j < cols; j += blockDim.x) {
        bool nz = false;
        if (open && j < last)
            for (int i = 0; i < k && !nz; i++) nz = ne(m[(size_t)i * cols + j], R32(0, 1));
        tgtf[(size_t)b * cols + j] = nz ? R32(1, 1) : R32(0, 1);
    }
}
// After a walk (maxm, then minm; linsys.cpp:864-876): success = a solution exists = not empty, decided; a negative
// status = the reference is undefined on this system, decided; anything else stays open for the next walk.
__global__ void k_dep_update(int nb, const int32_t * status, int * active, int32_t * empty)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb || active[b] != 1) return;
    const int st = status[b];
    if (st < 0) { empty[b] = st; active[b] = 0; }
    else if (st == XPG_IP_SUCC) { empty[b] = 0; active[b] = 0; }
}

// Lineq::has_solution (linsys.cpp:830-906): maxm then minm; success, or an unbounded answer
// when a unique solution is not demanded, means "has a solution".
inline int has_solution(xpg_ctx * ctx, const R32 * leq, int leq_rows, const R32 * eqs, int eq_rows, const R32 * vc,
                        int vc_rows, int cols, int rhs, bool is_int, bool is_unique)
{
    if (!ctx || !vc || cols < 2 || rhs != cols - 1 || vc_rows != rhs) return XPG_ERR_SHAPE;
    if (leq_rows == 0) return hs_no_inequality(eq_rows).has;
    const std::vector<R32> tgtf = feasibility_objective(leq, leq_rows, eqs, eq_rows, cols, rhs);
    R32 v; std::vector<R32> sol(cols);
    for (int pass = 0; pass < 2; pass++) {
        const int st = is_int
            ? mip_solve<R32>(ctx, 1, pass == 0, false, tgtf.data(), vc, vc_rows, eqs, eq_rows, leq, leq_rows, cols,
                             (const uint8_t *)0, &v, sol.data(), (long *)0)
            : six_solve<R32>(ctx, 1, pass == 0, tgtf.data(), vc, vc_rows, eqs, eq_rows, leq, leq_rows, cols,
                             0xFFFFFFFFu, &v, sol.data());
        if (const int has = hs_verdict(st, is_unique)) return has;
    }
    return 0;
}


// DepPoly::is_empty(keepit, vc) (src/eng/poly.cpp:530-573) for nb dependence polyhedra of one shape: the constant
// is column rhs_idx, columns after it are constant symbols. move2var (when there are symbols) -> Lineq::reduce at
// the last column -> inconsistent: empty; no row left: not empty; else Lineq::has_solution(int, unique) with the
// caller's variable constraints vc [rhs_idx][rhs_idx + 1] (NULL: -x_i <= 0, poly.cpp:563-567).
// With symbols that last step is undefined in the reference: has_solution is handed rhs_idx = the number of
// variables while the matrix has grown by the symbols, which SIX::verify (lpsol.h:1526-1552, "No yet support const
// term with multi-columns") only ASSERTs in debug builds -- those systems get XPG_ERR_REF_UNDEFINED, the ones
// reduce decides get their answer.
// symbols_as_vars (opt-in, NOT parity: XPG_DEP_SYMBOLS_AS_VARS): the evident intent of poly.cpp:530-573 for a parametrised
// polyhedron -- after move2var the constant symbols ARE variables (free ones: nothing is known of their sign), so has_solution
// is asked about the widened system, rhs_idx = the last column, vc widened by all-zero rows / columns for the symbols.
inline int dep_is_empty_batch(xpg_ctx * ctx, int nb, const R32 * mats, int rows, int cols, int rhs_idx, const R32 * vc_in,
                              int32_t * out_empty, long * out_nodes, int symbols_as_vars = 0)
{
    if (!ctx || nb < 0 || !mats || rows <= 0 || cols < 2 || !out_empty || rhs_idx < 1 || rhs_idx > cols - 1) return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    const int last = cols - 1, nsym = last - rhs_idx;
    // Variables that are x >= 0 or free (no vc, or a vc that is a sign pattern) and either no constant symbols or -- opt-in --
    // the symbols as free variables: the whole test stays on the device -- reduce, the feasibility objectives, the integer
    // maxm walk, the minm walk of what that left open -- and only the verdicts come back. With symbols, move2var runs on the
    // host in front of the upload; the walks' free list is the caller's free variables, then every symbol.
    const bool widen_dev = nsym > 0 && symbols_as_vars != 0;
    std::vector<int> fv;
    const bool pattern = !vc_in || vc_sign_pattern(vc_in, rhs_idx, rhs_idx + 1, fv);
    if (widen_dev) for (int j = rhs_idx; j < last; j++) fv.push_back(j);
    const int extra = (int)fv.size();
    if (mip_device_allowed() && (nsym == 0 || widen_dev) && pattern && mip_device_fits<R32>(rows, cols, false, 0, extra) &&
        lineq_lds_bytes(rows, cols) <= 160 * 1024 && rows <= 32767) {
        const int n = cols - 1, rmax = rows + n, depth = n + 2;
        const size_t bm = (size_t)nb * rows * cols * 8, bt = (size_t)nb * cols * 8;
        DevBuf dm, dt, dk, dok, dact, demp, dst, dv, dn, dws, dfv;
        std::vector<R32> moved;
        if (nsym > 0) {
            moved.resize((size_t)nb * rows * cols);
            for (int b = 0; b < nb; b++)
                move2var_one(mats + (size_t)b * rows * cols, moved.data() + (size_t)b * rows * cols, rows, cols, rhs_idx, rhs_idx + 1, last);
            mats = moved.data();
        }
        if (extra > 0) {
            XPG_TRY(dfv.alloc(ctx, (size_t)extra * 4));
            XPG_TRY(hipMemcpyAsync(dfv.p, fv.data(), (size_t)extra * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        XPG_TRY(dm.alloc(ctx, bm)); XPG_TRY(dt.alloc(ctx, bt)); XPG_TRY(dk.alloc(ctx, (size_t)nb * 4));
        XPG_TRY(dok.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dact.alloc(ctx, (size_t)nb * 4)); XPG_TRY(demp.alloc(ctx, (size_t)nb * 4));
        XPG_TRY(dst.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dv.alloc(ctx, (size_t)nb * 8)); XPG_TRY(dn.alloc(ctx, (size_t)nb * 4));
        XPG_TRY(hipMemcpyAsync(dm.p, mats, bm, hipMemcpyHostToDevice, ctx->stream));
        // Lineq::reduce on the device arrays (the C ABI entry: its kernels live in the row-elimination translation unit)
        int rc = xpg_lineq_reduce_batch_rat32_dev(ctx, nb, (xpg_rat32 *)dm.p, rows, cols, last, 1, (int32_t *)dk.p, (int32_t *)dok.p);
        if (rc) return rc;
        hipLaunchKernelGGL(k_dep_prepare, dim3((nb + 3) / 4), dim3(64, 4), 0, ctx->stream, nb, (const R32 *)dm.p, rows, cols,
                           (const int *)dk.p, (const int *)dok.p, (R32 *)dt.p, (int *)dact.p, (int32_t *)demp.p);
        XPG_TRY(hipMemsetAsync(dn.p, 0, (size_t)nb * 4, ctx->stream));
        std::vector<int32_t> nodes_a((size_t)nb, 0), nodes_b((size_t)nb, 0);
        for (int pass = 0; pass < 2; pass++) {
            const bool is_max = pass == 0;
            const MipGeom g = mip_geom<R32>(ctx, nb, rmax, n + extra, is_max);
            const size_t ws_words = mip_ws_words(rmax, cols, depth, extra);
            const int cus = ctx_cus(ctx);
            if (pass == 0) XPG_TRY(dws.alloc(ctx, (size_t)(cus * 32 < nb ? cus * 32 : nb) * ws_words * 8));   // the largest grid of either pass
            XPG_TRY(hipMemsetAsync(dn.p, 0, (size_t)nb * 4, ctx->stream));
            // ragged rows kept[b], the still-open marks, no solution wanted, no helpers
            rc = mip_tree_launch<R32>(ctx, g, 0, nb, dt.p, dm.p, rows, cols, is_max, false, rmax, depth, dws.p, ws_words, dst.p, dv.p, (void *)0, dn.p,
                                      dk.p, dact.p, (const void *)0, (const void *)0, 0, (void *)0, dfv.p, extra);
            if (rc) return rc;
            XPG_TRY(hipMemcpyAsync(pass == 0 ? nodes_a.data() : nodes_b.data(), dn.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
            hipLaunchKernelGGL(k_dep_update, dim3((nb + 255) / 256), dim3(256), 0, ctx->stream, nb, (const int32_t *)dst.p,
                               (int *)dact.p, (int32_t *)demp.p);
        }
        XPG_TRY(hipMemcpyAsync(out_empty, demp.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        if (out_nodes) { long t = 0; for (int b = 0; b < nb; b++) t += nodes_a[(size_t)b] + nodes_b[(size_t)b]; *out_nodes = t; }
        MipRoute & rt = mip_route();                     // a tree that was walked counted at least its root
        for (int b = 0; b < nb; b++) rt.device_trees += (nodes_a[(size_t)b] > 0) + (nodes_b[(size_t)b] > 0);
        if (extra > rt.free_vars) rt.free_vars = extra;
        return 0;
    }
    std::vector<R32> work((size_t)nb * rows * cols);
    if (nsym > 0) {
        for (int b = 0; b < nb; b++)
            move2var_one(mats + (size_t)b * rows * cols, work.data() + (size_t)b * rows * cols, rows, cols, rhs_idx, rhs_idx + 1, last);
    } else {
        work.assign(mats, mats + (size_t)nb * rows * cols);
    }
    std::vector<int32_t> kept(nb), ok(nb);
    int rc = xpg_lineq_reduce_batch_rat32(ctx, nb, (xpg_rat32 *)work.data(), rows, cols, last, 1, kept.data(), ok.data());
    if (rc) return rc;
    const bool widen = nsym > 0 && symbols_as_vars != 0;
    const int nv = widen ? last : rhs_idx;
    std::vector<R32> vc((size_t)nv * (nv + 1), R32(0, 1));
    if (vc_in && !widen) vc.assign(vc_in, vc_in + (size_t)nv * (nv + 1));
    else if (vc_in) {                                // the caller's [rhs_idx][rhs_idx + 1] block; the symbols' rows and columns stay zero (free)
        for (int i = 0; i < rhs_idx; i++) {
            for (int j = 0; j < rhs_idx; j++) vc[(size_t)i * (nv + 1) + j] = vc_in[(size_t)i * (rhs_idx + 1) + j];
            vc[(size_t)i * (nv + 1) + nv] = vc_in[(size_t)i * (rhs_idx + 1) + rhs_idx];
        }
    }
    else for (int i = 0; i < rhs_idx; i++) vc[(size_t)i * (nv + 1) + i] = R32(-1, 1);
    std::vector<int> open;                       // systems still undecided
    for (int b = 0; b < nb; b++) {
        if (!ok[b]) out_empty[b] = 1;            // inconsistent bounds: empty (poly.cpp:550-552)
        else if (kept[b] == 0) out_empty[b] = 0; // only redundant constraints: conservatively non-empty (:553-557)
        else if (nsym > 0 && !widen) out_empty[b] = XPG_ERR_REF_UNDEFINED;
        else { out_empty[b] = 1; open.push_back(b); }
    }
    long nodes = 0;
    for (int pass = 0; pass < 2 && !open.empty(); pass++) {          // maxm, then minm (linsys.cpp:864-876)
        std::vector<MipTask<R32> > tasks(open.size());
        for (size_t t = 0; t < open.size(); t++) {
            const int b = open[t];
            const R32 * leq = work.data() + (size_t)b * rows * cols;
            const std::vector<R32> tgtf = feasibility_objective(leq, kept[b], (const R32 *)0, 0, cols, last);
            tasks[t].start(make_problem<R32>(tgtf.data(), vc.data(), nv, (const R32 *)0, 0, leq, kept[b], cols),
                           pass == 0, false, (const uint8_t *)0);
        }
        rc = run_mip_tasks<R32>(ctx, 1, tasks);
        if (rc) return rc;
        std::vector<int> still;
        for (size_t t = 0; t < open.size(); t++) {
            nodes += tasks[t].nodes;
            const int st = tasks[t].final_status;
            if (st < 0) out_empty[open[t]] = st;             // reference undefined on this system
            else if (st == XPG_IP_SUCC) out_empty[open[t]] = 0;
            else still.push_back(open[t]);
        }
        open.swap(still);
    }
    if (out_nodes) *out_nodes = nodes;
    return 0;
}

} // namespace xpg
