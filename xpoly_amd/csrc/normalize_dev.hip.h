// SIX::normalize (src/com/lpsol.h:1290-1394) on the device, stated ONCE for its three callers: the HBM route's k_fold_eq /
// k_normal_form (six_host.hip.h), the batch kernel k_six_batch_vc (six_batch_vc.hip.h) and the MIP tree walk
// (mip_kernels.hip.h). Its steps: convertEq2Ineq (:1197-1278) substitutes, column by column, the one not yet used equality
// with a nonzero there into the inequalities; the equalities left over become pairs -e / e below them; every free variable
// gets a twin column; calcFinalSolution (:1851-1899) undoes the split. The host form the device cells are held against is
// fold_eq / normalize_cells_host / finish_host (six_host.hip.h, xpg_test_normalize). The reference's quirks live here only:
//   * the leading value of a substitution is read at the INEQUALITY's row index (:1232); once that index leaves the
//     equality's row the reference is undefined and the callers end XPG_ERR_REF_UNDEFINED
//   * the negation of a substituted row applies to the columns at and behind the constant column
//   * a left-over equality becomes -e first, then +e
//   * twins are the column times -1 with Matrix::mul's shortcuts (scaled()), which for fp64 decides the sign of zeros
// Two layers: CELL functions any thread may call, and WORKGROUP functions every thread of a block calls, barriers inside.
// The workgroup functions take the equalities through an accessor eqs(i, k) -- plain rows (EqRows) or the walk's list with
// its synthesised branch equalities -- and a pointer `sh` to four ints of LDS (NF_*). Arithmetic: the divide-free generic
// forms q_*(false, ...) of rat_ops.hip.h, equal to add / mul / div for every operand pair (tests/cxx/fma_canon_fuzz.cpp);
// substituted rows are not canonical, so nothing here may take the canonical forms.
#pragma once
#include "rat_ops.hip.h"

namespace xpg {

// ---- cell functions -------------------------------------------------------------------------------------------------

// What one substitution multiplies the equality's cells by in inequality q (lpsol.h:1232-1240): 1 / lead unless the lead
// is 1, then the inequality's coefficient, each with Matrix::mul's shortcuts. lead = the equality's cell at column q.
template <class S> struct FoldScale { S inv, coef; int mode1, mode2; };
template <class S> __device__ __forceinline__ FoldScale<S> nf_fold_scale(S lead, S coef)
{
    FoldScale<S> f;
    const bool rescale = ne(lead, one<S>());
    f.inv = rescale ? q_div(false, one<S>(), lead) : one<S>();
    f.coef = coef;
    f.mode1 = rescale ? scale_mode(f.inv) : (int)SCALE_KEEP;
    f.mode2 = scale_mode(coef);
    return f;
}
// Cell k of inequality q after the substitution for variable j (lpsol.h:1241-1250): the scaled cell e_k of the equality,
// negated from the constant column rhs on, plus the inequality's own cell cur -- which column j has given up.
template <class S> __device__ __forceinline__ S nf_fold_cell(S e_k, const FoldScale<S> & f, S cur, int k, int j, int rhs)
{
    S t = q_scaled(false, q_scaled(false, e_k, f.inv, f.mode1), f.coef, f.mode2);
    if (k >= rhs) t = neg(t);
    return q_add(false, t, k == j ? zero<S>() : cur);
}

// Column c of the widened form [n0 variables | one twin per free variable | constant] comes from this column of the
// caller's [n0 variables | constant] (n = n0 + the number of free variables).
__device__ __forceinline__ int nf_src_col(int c, int n0, int n, const int * free_var)
{
    return c < n0 ? c : (c == n ? n0 : free_var[c - n0]);
}
// A twin is its variable's cell times -1 (lpsol.h:1380-1386); the other columns pass.
template <class S> __device__ __forceinline__ S nf_twin_cell(S x, int c, int n0, int n)
{
    const S m1 = minus_one<S>();
    return c >= n0 && c < n ? q_scaled(false, x, m1, scale_mode(m1)) : x;
}
// Cell (i, c) of the normal form from its source cell x: rows from lrows on are the left-over equalities in pairs, the
// first of a pair times -1 (lpsol.h:1264-1277); then the twin.
template <class S> __device__ __forceinline__ S nf_form_cell(S x, int i, int lrows, int c, int n0, int n)
{
    const S m1 = minus_one<S>();
    if (i >= lrows && ((i - lrows) & 1) == 0) x = q_scaled(false, x, m1, scale_mode(m1));
    return nf_twin_cell(x, c, n0, n);
}

// ---- workgroup functions --------------------------------------------------------------------------------------------

enum { NF_COL = 0, NF_EQ = 1, NF_LEFT = 2, NF_UNDEF = 3 };      // sh[]: the step's column and equality, equalities left over, lpsol.h:1232 left a row

// Equalities that are rows of an array, in LDS or HBM.
template <class S> struct EqRows {
    const S * p; int cols;
    __device__ __forceinline__ S operator()(int i, int k) const { return p[(size_t)i * cols + k]; }
};

// convertEq2Ineq's next choice (lpsol.h:1209-1222) from column `from` on: the first column in which exactly one not yet
// used equality has a nonzero. Wave 0 looks, lane l holding equalities l, l + 64, ...; bit c of its `used`: equality
// 64 c + l is spent (so up to 4096 equalities). The step is in sh[NF_COL] / sh[NF_EQ] for everyone, column -1: none left.
template <class S, class E> __device__ __forceinline__ void nf_next_step(E eqs, int ne_rows, int n0, int from, unsigned long long & used, int * sh)
{
    if (threadIdx.x < 64) {
        const int lane = (int)threadIdx.x;
        int fj = -1, fat = -1;
        for (int j = from; j < n0 && fj < 0; j++) {
            int hits = 0, at = -1;
            for (int c = 0; c * 64 < ne_rows; c++) {
                const int i = c * 64 + lane;
                const bool hit = i < ne_rows && !((used >> c) & 1ull) && ne(eqs(i, j), zero<S>());
                const unsigned long long mask = __ballot(hit);
                hits += __popcll(mask);
                if (mask) at = c * 64 + __ffsll((long long)mask) - 1;
            }
            if (hits == 1) { fj = j; fat = at; }
        }
        if (fat >= 0 && (fat & 63) == lane) used |= 1ull << (fat >> 6);
        if (lane == 0) { sh[NF_COL] = fj; sh[NF_EQ] = fat; }
    }
    __syncthreads();
}

// One substitution (lpsol.h:1224-1250) on the inequalities L [lrows x cols]: it changes inequality q from its own cells
// and the equality's alone. A thread takes a cell; column j, which holds the coefficient the other cells of its row are
// folded with, goes last, a thread a row.
template <class S, class E> __device__ __forceinline__ void nf_fold_step(S * L, int lrows, int cols, E eqs, int j, int at, int * sh)
{
    for (int t = (int)threadIdx.x; t < lrows * cols; t += (int)blockDim.x) {
        const int q = t / cols, k = t - q * cols;
        const S coef = L[(size_t)q * cols + j];
        if (k == j || q >= cols || eq(coef, zero<S>())) continue;
        L[t] = nf_fold_cell(eqs(at, k), nf_fold_scale(eqs(at, q), coef), L[t], k, j, cols - 1);
    }
    __syncthreads();
    for (int q = (int)threadIdx.x; q < lrows; q += (int)blockDim.x) {
        const S coef = L[(size_t)q * cols + j];
        if (eq(coef, zero<S>())) continue;
        if (q >= cols) { sh[NF_UNDEF] = 1; continue; }
        L[(size_t)q * cols + j] = nf_fold_cell(eqs(at, j), nf_fold_scale(eqs(at, q), coef), zero<S>(), j, j, cols - 1);
    }
    __syncthreads();
}

// The equalities no step has used, ascending, into rest[]; their number is returned to every thread.
template <class I> __device__ __forceinline__ int nf_left_over(int ne_rows, unsigned long long used, I * rest, int * sh)
{
    if (threadIdx.x < 64) {
        const int lane = (int)threadIdx.x;
        int left = 0;
        for (int c = 0; c * 64 < ne_rows; c++) {
            const int i = c * 64 + lane;
            const bool keep = i < ne_rows && !((used >> c) & 1ull);
            const unsigned long long mask = __ballot(keep);
            if (keep) rest[left + __popcll(mask & ((1ull << lane) - 1ull))] = (I)i;
            left += __popcll(mask);
        }
        if (lane == 0) sh[NF_LEFT] = left;
    }
    __syncthreads();
    return sh[NF_LEFT];
}

// convertEq2Ineq on L [lrows x cols] in place: every substitution in the reference's order (with no inequality there is
// nothing to substitute into), then the list of the equalities left over. Returns their number, or -1 where a
// substitution read past an equality's row. The caller has a barrier between its last use of sh and this call.
template <class S, class E, class I> __device__ __forceinline__ int nf_convert_eq(S * L, int lrows, int cols, E eqs, int ne_rows, I * rest, int * sh)
{
    unsigned long long used = 0ull;
    if (threadIdx.x == 0) sh[NF_UNDEF] = 0;
    int from = 0;
    while (lrows > 0) {
        nf_next_step<S>(eqs, ne_rows, cols - 1, from, used, sh);
        const int j = sh[NF_COL], at = sh[NF_EQ];
        if (j < 0) break;
        nf_fold_step<S>(L, lrows, cols, eqs, j, at, sh);
        from = j + 1;
    }
    const int left = nf_left_over(ne_rows, used, rest, sh);
    return sh[NF_UNDEF] ? -1 : left;
}

// The normal form N [(lrows + 2 nrest) x (n + 1)] from the folded inequalities L [lrows x cols] and the equalities of
// rest[]. Without a free variable N may be L itself: its first lrows rows then map onto themselves.
template <class S, class E, class I>
__device__ __forceinline__ void nf_form(const S * L, int lrows, int cols, E eqs, const I * rest, int nrest, const int * free_var, int extra, S * N)
{
    const int n0 = cols - 1, n = n0 + extra;
    for (int t = (int)threadIdx.x; t < (lrows + 2 * nrest) * (n + 1); t += (int)blockDim.x) {
        const int i = t / (n + 1), c = t - i * (n + 1), sc = nf_src_col(c, n0, n, free_var);
        const S x = i < lrows ? L[(size_t)i * cols + sc] : eqs((int)rest[(i - lrows) >> 1], sc);
        N[t] = nf_form_cell(x, i, lrows, c, n0, n);
    }
    __syncthreads();
}
// The objective widened the same way (lpsol.h:1365-1392): obj [n + 1] from tgtf [cols].
template <class S> __device__ __forceinline__ void nf_objective(const S * tgtf, int cols, const int * free_var, int extra, S * obj)
{
    const int n0 = cols - 1, n = n0 + extra;
    for (int c = (int)threadIdx.x; c <= n; c += (int)blockDim.x) obj[c] = nf_twin_cell(tgtf[nf_src_col(c, n0, n, free_var)], c, n0, n);
    __syncthreads();
}

// calcFinalSolution (lpsol.h:1851-1899), first half: the raw values y [n] of the normal form's variables back to the
// caller's, y[v] = y[v'] - y[v''].
template <class S> __device__ __forceinline__ void nf_unsplit(S * y, int cols, const int * free_var, int extra)
{
    for (int k = (int)threadIdx.x; k < extra; k += (int)blockDim.x) y[free_var[k]] = q_sub(false, y[free_var[k]], y[cols - 1 + k]);
    __syncthreads();
}
// Second half: the solution (y, 1), its products with the ORIGINAL objective into prod [cols] (prod may be y) and its
// reduced entries into sol [cols]. The sum of the products keeps the reference's order: one thread of the caller adds them.
template <class S> __device__ __forceinline__ void nf_products(const S * y, const S * tgtf, int cols, S * prod, S * sol)
{
    for (int j = (int)threadIdx.x; j < cols; j += (int)blockDim.x) {
        S x = j < cols - 1 ? y[j] : one<S>();
        prod[j] = q_mul(false, x, tgtf[j]);
        reduce(x);
        sol[j] = x;
    }
    __syncthreads();
}

} // namespace xpg
