// C++ adapter: a class with the names and signatures of xpoly's Lineq (src/com/linsys.h:61-186) for the
// members that sit on the hot path -- reduce, fme, has_solution, calcBound, move2var, removeIdenRow -- on top of
// the C ABI in ../xpoly_amd.h, plus the small host-side members the engine's own Lineq objects call next to them
// (appendEquation, formatBound, initVarConstraint, is_consistent), so that call sites such as
//
//     Lineq lin(NULL);                                      // src/eng/poly.cpp:537
//     if (!lin.reduce(*coeff, coeff->get_col_size() - 1, true)) return true;
//     return !lin.has_solution(*coeff, eq, lvc, rhs_idx, true, true);   // src/eng/poly.cpp:571, linsys.cpp:830
//
// compile unchanged against `xpoly_amd::Lineq<RMat>` and run on the GPU. Each member is the batch entry point
// with a batch of one (the batch forms in xpoly_amd.h are what a caller with a SCoP's worth of polyhedra
// should use; the collectors below the class -- dep_is_empty_all, has_solution_all, fme_all, project_all,
// levels_all, project_each, levels_nests, calc_bound_all, calc_bound_each, hull_all, project_union_each -- take the caller's matrix objects and make those calls). Header only; relies on the Matrix<Rational> contract only: get_row_size(), get_col_size(),
// get_matrix() (row-major {int32 num; int32 den}, matt.h:152-156, rational.h:66-67), size(), reinit(r, c).
#ifndef XPOLY_AMD_LINEQ_HPP
#define XPOLY_AMD_LINEQ_HPP

#include <cstddef>
#include <cstring>
#include <type_traits>
#include <utility>
#include <vector>
#include "../xpoly_amd.h"
#include "six.hpp"

namespace xpoly_amd {

namespace detail {
// (defined below the collectors: the one call behind Lineq::ConvexHullUnionAndIntersect, hull_all and project_union_each)
template <class RMatT>
int hull_groups(const std::vector<std::vector<RMatT *> > & groups, const std::vector<int32_t> & rhs_idx,
                const std::vector<std::vector<std::vector<int32_t> > > * elims, bool darkshadow, bool is_intersect, std::vector<RMatT> & results,
                std::vector<int32_t> & ok, std::vector<int32_t> * member, xpg_ctx * c);
}

template <class RMatT> class Lineq {
    xpg_ctx * m_ctx;
    RMatT * m_coeff;                 // linsys.h:64-70
    int m_rhs_idx;
    xpg_ctx * ctx() { return m_ctx ? m_ctx : detail::shared_context(); }
    static void put(RMatT & m, const std::vector<xpg_rat32> & a, int rows, int cols)
    {
        m.reinit(rows, cols);
        if (rows > 0 && cols > 0) std::memcpy((void *)m.get_matrix(), (const void *)a.data(), sizeof(xpg_rat32) * (size_t)rows * cols);
    }
public:
    explicit Lineq(RMatT * m, int rhs_idx = -1, xpg_ctx * c = 0) : m_ctx(c), m_coeff(m), m_rhs_idx(rhs_idx)
    { if (m && rhs_idx == -1) m_rhs_idx = (int)m->get_col_size() - 1; }
    void init(RMatT * m, int rhs_idx = -1) { set_param(m, rhs_idx); }   // linsys.cpp:92-108
    void destroy() { m_coeff = 0; m_rhs_idx = -1; }
    void set_param(RMatT * m, int rhs_idx = -1)             // linsys.cpp:117-131
    { m_coeff = m; m_rhs_idx = (m && rhs_idx == -1) ? (int)m->get_col_size() - 1 : rhs_idx; }

    // ---- host-side members (no arithmetic worth a launch; they only reshape the caller's matrices with the
    //      Matrix type's own operations, exactly the ones the reference uses, so the cells are the reference's)
    // Lineq::appendEquation, linsys.cpp:922-935 (caller PolyTran::scan's bound computation, src/eng/poly.cpp:4804):
    // every equation a = b joins the system as a <= b and -a <= -b.
    void appendEquation(RMatT const & eq)
    {
        if (eq.size() == 0 || eq.get_row_size() == 0) return;
        RMatT both = eq;
        m_coeff->grow_row(both, 0, both.get_row_size() - 1);
        both.mul(-1);
        m_coeff->grow_row(both, 0, both.get_row_size() - 1);
    }
    // Lineq::initVarConstraint, linsys.cpp:803-819 (caller src/eng/poly.cpp:1603): -x_i <= 0 for every variable
    // whose sign entry is >= 0 (all of them without a sign vector), nothing for the others.
    template <class SignVec> void initVarConstraint(SignVec const * sign, RMatT & vc, unsigned rhs_idx)
    {
        typedef typename std::decay<decltype(std::declval<RMatT const &>().get(0u, 0u))>::type R;
        vc.reinit(rhs_idx, rhs_idx + 1);
        vc.set_col(rhs_idx, R(0));
        for (unsigned i = 0; i < rhs_idx; i++)
            if (!sign || sign->get(i) >= 0) vc.set(i, i, -1);
    }
    void initVarConstraint(std::nullptr_t, RMatT & vc, unsigned rhs_idx) { initVarConstraint((all_nonnegative const *)0, vc, rhs_idx); }
private:
    struct all_nonnegative { int get(unsigned) const { return 0; } };
public:
    // Lineq::is_consistent, linsys.cpp:779-800: eliminate the variables one after the other (each step an fme on the
    // device); the system is contradictory as soon as one elimination says so. The caller's matrix is left alone.
    bool is_consistent()
    {
        RMatT * const keep = m_coeff;
        const int keep_rhs = m_rhs_idx;
        RMatT work = *keep;
        set_param(&work, keep_rhs);
        bool consistent = true;
        for (unsigned v = 0; consistent && v < (unsigned)keep_rhs; v++) {
            RMatT next;
            if (!fme(v, next)) consistent = false; else work = next;
        }
        set_param(keep, keep_rhs);
        return consistent;
    }
    // Lineq::formatBound, linsys.cpp:948-1030 (caller src/eng/ldtran.cpp:1534): the rows that mention variable u, its
    // coefficient brought to +-1, the other variables moved to the right-hand side (negated, appended behind the
    // constant / symbol columns), every row then over one common denominator from column 1 on.
    void formatBound(unsigned u, RMatT & bound_of_u)
    {
        typedef typename std::decay<decltype(std::declval<RMatT const &>().get(0u, 0u))>::type R;
        bound_of_u.reinit(0, 0);
        for (unsigned i = 0; i < m_coeff->get_row_size(); i++)
            if (m_coeff->get(i, u) != 0) {
                RMatT row;
                m_coeff->innerRow(row, i, i);
                bound_of_u.grow_row(row);
            }
        const unsigned rows = bound_of_u.get_row_size();
        if (rows == 0) return;                               // nothing constrains u
        const unsigned nvar = (unsigned)m_rhs_idx;
        const unsigned moved_at = bound_of_u.get_col_size();
        if (nvar != 1) bound_of_u.grow_col(nvar - 1);
        for (unsigned i = 0; i < rows; i++) {
            for (unsigned j = moved_at; j < bound_of_u.get_col_size(); j++) bound_of_u.setr(i, j, 0, 1);
            R c = bound_of_u.get(i, u);
            if (c < 0) c = -c;
            if (c != 1) bound_of_u.mulOfRow(i, 1 / c);
            if (nvar == 1) continue;
            unsigned k = moved_at;
            for (unsigned j = 0; j < nvar; j++)
                if (j != u) bound_of_u.set(i, k++, -bound_of_u.get(i, j));
        }
        if (nvar != 1) {
            if (u + 1 != nvar) bound_of_u.del_col(u + 1, nvar - 1);
            if (u > 0) bound_of_u.del_col(0, u - 1);
        }
        for (unsigned i = 0; i < rows; i++) bound_of_u.comden(i, 1);
    }

    // Lineq::reduce, linsys.cpp:359-626: in place; false = the system is inconsistent.
    bool reduce(RMatT & m, unsigned rhs_idx, bool is_intersect)
    {
        const int rows = (int)m.get_row_size(), cols = (int)m.get_col_size();
        if (rows == 0) return true;
        std::vector<xpg_rat32> a((size_t)rows * cols);
        std::memcpy((void *)a.data(), (const void *)m.get_matrix(), sizeof(xpg_rat32) * a.size());
        int32_t kept = 0, ok = 0;
        if (xpg_lineq_reduce_batch_rat32(ctx(), 1, a.data(), rows, cols, (int)rhs_idx, is_intersect ? 1 : 0, &kept, &ok) != 0) return false;
        put(m, a, kept, cols);
        return ok != 0;
    }
    // Lineq::removeIdenRow, linsys.cpp:1209-1268
    void removeIdenRow(RMatT & m)
    {
        const int rows = (int)m.get_row_size(), cols = (int)m.get_col_size();
        if (rows == 0) return;
        std::vector<xpg_rat32> a((size_t)rows * cols);
        std::memcpy((void *)a.data(), (const void *)m.get_matrix(), sizeof(xpg_rat32) * a.size());
        int32_t kept = 0;
        if (xpg_lineq_remove_iden_batch_rat32(ctx(), 1, a.data(), rows, cols, &kept) == 0) put(m, a, kept, cols);
    }
    // Lineq::move2var, linsys.cpp:1177-1200
    void move2var(RMatT & ieq, unsigned rhs_idx, unsigned first_sym, unsigned last_sym, unsigned * first_var_idx, unsigned * last_var_idx)
    {
        xpg_lineq_move2var_batch_rat32(ctx(), 1, (xpg_rat32 *)ieq.get_matrix(), (int)ieq.get_row_size(), (int)ieq.get_col_size(),
                                       (int)rhs_idx, (int)first_sym, (int)last_sym);
        if (first_var_idx) *first_var_idx = rhs_idx;
        if (last_var_idx) *last_var_idx = rhs_idx + (last_sym - first_sym);
    }
    // Lineq::fme on the system given to the constructor / set_param, linsys.cpp:656-774
    bool fme(unsigned u, RMatT & res, bool darkshadow = false)
    {
        // the packed form: only the live rows travel, and they are read straight out of the handle's pinned buffer
        if (m_coeff->size() == 0) { res.clean(); return true; }       // an empty system stays empty (linsys.cpp:661-664)
        const int rows = (int)m_coeff->get_row_size(), cols = (int)m_coeff->get_col_size();
        const xpg_rat32 * view = 0;
        long long off[2] = {0, 0};
        int32_t ok = 0;
        if (xpg_lineq_fme_batch_packed_rat32(ctx(), 1, (const xpg_rat32 *)m_coeff->get_matrix(), rows, cols, m_rhs_idx, (int)u,
                                             darkshadow ? 1 : 0, 0, (xpg_rat32 *)0, 0, &view, off, &ok) != 0) return false;
        const int orows = (int)off[1];
        res.reinit(orows, cols);
        if (orows > 0 && cols > 0) std::memcpy((void *)res.get_matrix(), (const void *)view, sizeof(xpg_rat32) * (size_t)orows * cols);
        return ok != 0;
    }
    // Lineq::has_solution, linsys.cpp:830-906
    bool has_solution(RMatT const & leq, RMatT const & eq, RMatT & vc, unsigned rhs_idx, bool is_int_sol, bool is_unique_sol)
    {
        if (leq.size() == 0 && eq.size() == 0) return false;
        const int cols = leq.size() ? (int)leq.get_col_size() : (int)eq.get_col_size();
        const int r = xpg_has_solution_rat32(ctx(), (const xpg_rat32 *)detail::data_of(leq), leq.size() ? (int)leq.get_row_size() : 0,
                                             (const xpg_rat32 *)detail::data_of(eq), eq.size() ? (int)eq.get_row_size() : 0,
                                             (const xpg_rat32 *)detail::data_of(vc), (int)vc.get_row_size(), cols, (int)rhs_idx,
                                             is_int_sol ? 1 : 0, is_unique_sol ? 1 : 0);
        return r == 1;
    }
    // Lineq::calcBound, linsys.cpp:1047-1078: the bounds of variable j alone (every other variable eliminated, inner to
    // outer) for every j, all chains on the device in one call and one launch (xpg_lineq_bounds_batch_packed_rat32).
    //   bool calcBound(List<RMat*> & limits)   -- the reference's own signature (linsys.h:151): `limits` holds m_rhs_idx
    //                                             matrices the caller owns, *limits.get_head_nth(j) receives variable j's
    //                                             (linsys.cpp:1072-1074), so the call site at linsys.cpp:312 compiles unchanged
    //   bool calcBound(std::vector<RMat> &)    -- the same with value semantics (resized to m_rhs_idx)
private:
    template <class Sink> bool calc_bound_into(Sink sink)
    {
        // the packed form: only the live rows of the nv bound systems travel, read straight out of the handle's pinned buffer
        const int rows = (int)m_coeff->get_row_size(), cols = (int)m_coeff->get_col_size(), nv = m_rhs_idx;
        int cap = 4 * rows + 16;
        for (int attempt = 0; attempt < 2; attempt++) {
            std::vector<long long> off((size_t)nv + 1, 0);
            const xpg_rat32 * view = 0;
            int32_t ok = 0, chain = -1, step = 0;
            if (xpg_lineq_bounds_batch_packed_rat32(ctx(), 1, (const xpg_rat32 *)m_coeff->get_matrix(), rows, cols, nv, cap, 0, (xpg_rat32 *)0, 0,
                                                    &view, off.data(), &ok, &chain, &step) != 0) return false;
            if (ok < 0) { cap = -ok; continue; }
            if (ok == 0) return false;                       // "system inconsistency!" (linsys.cpp:1065-1068)
            for (int j = 0; j < nv; j++) {
                const int r = (int)(off[(size_t)j + 1] - off[(size_t)j]);
                std::vector<xpg_rat32> one;
                if (r) one.assign(view + (size_t)off[(size_t)j] * cols, view + (size_t)off[(size_t)j + 1] * cols);
                sink(j, one, r, cols);
            }
            return true;
        }
        return false;
    }
public:
    bool calcBound(std::vector<RMatT> & limits)
    {
        limits.resize((size_t)m_rhs_idx);
        return calc_bound_into([&](int j, const std::vector<xpg_rat32> & a, int r, int c) { put(limits[(size_t)j], a, r, c); });
    }
    template <class ListT, class = decltype(std::declval<ListT &>().get_head_nth(0u)), class = decltype(std::declval<ListT &>().get_elem_count())>
    bool calcBound(ListT & limits)
    {
        if ((int)limits.get_elem_count() != m_rhs_idx) return false;      // the reference ASSERTs (linsys.cpp:1050-1051)
        return calc_bound_into([&](int j, const std::vector<xpg_rat32> & a, int r, int c) { put(*limits.get_head_nth((unsigned)j), a, r, c); });
    }
    // Loop-bound generation, LoopTran::transformIterSpace (src/eng/ldtran.cpp:178-196 unimodular, :241-257 nonsingular):
    //     newb = aux_limits.get_tail();
    //     for (i = m_rhs_idx - 1; i > 0; i--) { *newb = *A; lineq.fme(i, res); *A = res; newb = aux_limits.get_prev(); }
    //     *newb = *A;
    // in ONE call and one launch (xpg_lineq_levels_batch_packed_rat32: every level of the projection is kept). `aux_limits`
    // holds m_rhs_idx matrices the caller owns (else false); walking from get_tail() by get_prev() the tail receives the
    // system unchanged, each further entry the next level -- variables m_rhs_idx-1 .. 1 eliminated one after the other --
    // and the head the outermost bound: what the loop leaves in the list. A (may be null; may be the system itself, as in
    // the reference) receives the last level, as the loop leaves *A. false where a step found the system inconsistent (the
    // reference ASSERTs there) or the call failed: the list is then left as it was. m_rhs_idx == 1 copies and makes no call.
    //   bool fmeLevels(ListT & aux_limits, RMat * A = 0)           -- a list with get_tail / get_prev / get_elem_count
    //   bool fmeLevels(std::vector<RMat> & aux_limits, RMat * A = 0) -- value semantics: resized to m_rhs_idx, [0] the
    //                                                                 outermost bound (the head), back() the system
private:
    static void put_rows(RMatT & m, const xpg_rat32 * a, int rows, int cols)
    {
        m.reinit((unsigned)rows, (unsigned)cols);
        if (rows > 0 && cols > 0) std::memcpy((void *)m.get_matrix(), (const void *)a, sizeof(xpg_rat32) * (size_t)rows * cols);
    }
    // sink(pos, cells, rows, cols): pos 0 is the system itself (the tail), pos k + 1 level k; called only once every level
    // is there, read straight out of the handle's pinned buffer. A capacity found short is raised to the need reported --
    // need > cap: a step's unreduced rows, else a level's slot -- and the call made again, at most four times.
    template <class Sink> bool levels_into(Sink sink)
    {
        const int nv = m_rhs_idx, n = nv - 1;
        if (nv < 1) return false;
        const int rows = m_coeff->size() == 0 ? 0 : (int)m_coeff->get_row_size(), cols = (int)m_coeff->get_col_size();
        const xpg_rat32 * in = rows ? (const xpg_rat32 *)m_coeff->get_matrix() : (const xpg_rat32 *)0;
        if (n == 0 || rows == 0) {                               // nothing to eliminate, or an empty system: it stays empty
            sink(0, in, rows, cols);
            for (int k = 0; k < n; k++) sink(k + 1, (const xpg_rat32 *)0, 0, cols);
            return true;
        }
        std::vector<int32_t> elim((size_t)n);
        for (int k = 0; k < n; k++) elim[(size_t)k] = nv - 1 - k;
        int cap = rows * rows / 4 + rows + 1, cap_out = cap < 4 * rows + 16 ? cap : 4 * rows + 16;
        for (int attempt = 0; attempt < 4; attempt++) {
            std::vector<long long> off((size_t)n + 1, 0);
            const xpg_rat32 * view = 0;
            int32_t ok = 0, step = 0;
            if (xpg_lineq_levels_batch_packed_rat32(ctx(), 1, in, rows, cols, nv, elim.data(), n, 0, cap, cap_out, (xpg_rat32 *)0, 0, &view,
                                                    off.data(), &ok, &step) != 0) return false;
            if (ok < 0) { if (-ok > cap) cap = -ok; else cap_out = -ok; continue; }
            if (ok == 0) return false;                           // "system inconsistency!" (ldtran.cpp:186-188)
            sink(0, in, rows, cols);
            for (int k = 0; k < n; k++)
                sink(k + 1, off[(size_t)k + 1] > off[(size_t)k] ? view + (size_t)off[(size_t)k] * cols : (const xpg_rat32 *)0,
                     (int)(off[(size_t)k + 1] - off[(size_t)k]), cols);
            return true;
        }
        return false;
    }
public:
    bool fmeLevels(std::vector<RMatT> & aux_limits, RMatT * A = 0)
    {
        if (m_rhs_idx < 1) return false;
        const size_t nv = (size_t)m_rhs_idx;
        std::vector<RMatT> got(nv);
        if (!levels_into([&](int pos, const xpg_rat32 * a, int r, int c) { put_rows(got[nv - 1 - (size_t)pos], a, r, c); })) return false;
        aux_limits.swap(got);
        if (A) *A = aux_limits[0];
        return true;
    }
    template <class ListT, class = decltype(std::declval<ListT &>().get_tail()), class = decltype(std::declval<ListT &>().get_prev()),
              class = decltype(std::declval<ListT &>().get_elem_count())>
    bool fmeLevels(ListT & aux_limits, RMatT * A = 0)
    {
        if (m_rhs_idx < 1 || (int)aux_limits.get_elem_count() != m_rhs_idx) return false;   // the reference ASSERTs (ldtran.cpp:191-192)
        std::vector<RMatT *> dst;                                // the tail first; none of them is the system itself
        for (RMatT * newb = aux_limits.get_tail(); (int)dst.size() < m_rhs_idx; newb = aux_limits.get_prev()) {
            if (!newb || newb == m_coeff) return false;
            dst.push_back(newb);
            if ((int)dst.size() == m_rhs_idx) break;
        }
        if (!levels_into([&](int pos, const xpg_rat32 * a, int r, int c) { put_rows(*dst[(size_t)pos], a, r, c); })) return false;
        if (A) *A = *dst.back();
        return true;
    }
    // Lineq::ConvexHullUnionAndIntersect, linsys.cpp:283-336, with the reference's signature: calcBound on every polyhedron of
    // `chlst` (all of one dimension), every variable's bounds appended behind one zero row, and reduce(res, rhs_idx,
    // is_intersect) over the lot -- the widest bounds (the union's bounding hull) or the tightest; an inconsistent intersection
    // and an empty list clean `res`. ONE library call (xpg_lineq_hull_batch_ragged_rat32 with one group: two launches, one
    // synchronisation); many lists at once: hull_all, below. STATED DEVIATION: where calcBound fails on a member the reference's
    // release build goes on with the bounds of the member before; here `res` is cleaned (a violated precondition, not a result).
    //   void ConvexHullUnionAndIntersect(RMat & res, ListT & chlst, unsigned rhs_idx, bool is_intersect)   -- a list with
    //                                             get_head / get_next / get_elem_count (the reference's List<RMat*>)
    //   void ConvexHullUnionAndIntersect(RMat & res, std::vector<RMat *> & chlst, unsigned rhs_idx, bool is_intersect)
    void ConvexHullUnionAndIntersect(RMatT & res, std::vector<RMatT *> & chlst, unsigned rhs_idx, bool is_intersect)
    {
        if (chlst.empty()) { res.clean(); return; }                 // linsys.cpp:289-292
        std::vector<std::vector<RMatT *> > groups(1, chlst);
        std::vector<RMatT> out;
        std::vector<int32_t> ok, member;
        if (detail::hull_groups(groups, std::vector<int32_t>(1, (int32_t)rhs_idx), (const std::vector<std::vector<std::vector<int32_t> > > *)0, false,
                                is_intersect, out, ok, &member, ctx()) != 0 || member[0] >= 0 || ok[0] < 0 || out[0].size() == 0) { res.clean(); return; }
        res = out[0];
    }
    template <class ListT, class = decltype(std::declval<ListT &>().get_head()), class = decltype(std::declval<ListT &>().get_next()),
              class = decltype(std::declval<ListT &>().get_elem_count())>
    void ConvexHullUnionAndIntersect(RMatT & res, ListT & chlst, unsigned rhs_idx, bool is_intersect)
    {
        std::vector<RMatT *> v;
        for (RMatT * p = chlst.get_head(); p != 0; p = chlst.get_next()) v.push_back(p);
        ConvexHullUnionAndIntersect(res, v, rhs_idx, is_intersect);
    }
};

// One SCoP's worth of dependence tests in ONE call: DepPoly::is_empty (src/eng/poly.cpp:530-573, called per polyhedron by
// DepGraph::rebuild, poly.cpp:268-314) on polyhedra of whatever shapes DepPolyMgr::build produced (poly.cpp:1120-1224).
// empty[k] = 1 / 0 as is_empty would return for *polys[k], XPG_ERR_REF_UNDEFINED where the reference is undefined.
template <class RMatT>
inline int dep_is_empty_all(const std::vector<RMatT *> & polys, std::vector<int32_t> & empty, xpg_ctx * c = 0)
{
    const int nb = (int)polys.size();
    std::vector<int32_t> rows((size_t)nb), cols((size_t)nb);
    std::vector<long long> off((size_t)nb + 1, 0);
    for (int b = 0; b < nb; b++) {
        rows[(size_t)b] = (int32_t)polys[(size_t)b]->get_row_size(); cols[(size_t)b] = (int32_t)polys[(size_t)b]->get_col_size();
        off[(size_t)b + 1] = off[(size_t)b] + (long long)rows[(size_t)b] * cols[(size_t)b];
    }
    std::vector<xpg_rat32> flat((size_t)off[(size_t)nb]);
    for (int b = 0; b < nb; b++)
        if (rows[(size_t)b] * cols[(size_t)b])
            std::memcpy((void *)(flat.data() + off[(size_t)b]), (const void *)polys[(size_t)b]->get_matrix(),
                        sizeof(xpg_rat32) * (size_t)rows[(size_t)b] * cols[(size_t)b]);
    empty.assign((size_t)nb, 0);
    return xpg_dep_is_empty_batch_ragged_rat32(c ? c : detail::shared_context(), nb, flat.data(), rows.data(), cols.data(), off.data(),
                                               empty.data(), (long long *)0);
}

// Many feasibility questions in few calls: Lineq::has_solution(*leqs[k], *eqs[k], vc, rhs_idx, is_int_sol, is_unique_sol)
// (linsys.cpp:830-906) under one vc. leqs[k] / eqs[k] may be null or without rows; all non-empty matrices have rhs_idx + 1
// columns. The systems are packed once, in the order given, and go up in ONE xpg_has_solution_batch_ragged_rat32 call
// whatever their shapes (leq rows, eq rows): the library sends each system the way a batch of its shape goes -- one launch
// per kernel, each system answered by one workgroup that normalises once and asks maxm, then minm. With is_int_sol the call is
// xpg_has_solution_int_batch_ragged_rat32: the library forms the shape classes itself and answers each on the device --
// objective, both integer walks and the verdict, one synchronisation per class. out[k] = 1 / 0 as has_solution would return, or a negative XPG_ERR_* where the reference is
// undefined on system k. Returns 0 or a negative XPG_ERR_* code.
template <class RMatT>
inline int has_solution_all(const std::vector<RMatT *> & leqs, const std::vector<RMatT *> & eqs, const RMatT & vc, int rhs_idx,
                            bool is_int_sol, bool is_unique_sol, std::vector<int32_t> & out, xpg_ctx * c = 0)
{
    const int nb = (int)leqs.size(), cols = rhs_idx + 1;
    if ((int)eqs.size() != nb || rhs_idx < 1 || (int)vc.get_row_size() != rhs_idx || (int)vc.get_col_size() != cols) return XPG_ERR_SHAPE;
    out.assign((size_t)nb, 0);
    if (nb == 0) return 0;
    const auto rows_of = [&](const RMatT * m) { return m && m->get_col_size() ? (int)m->get_row_size() : 0; };
    std::vector<int32_t> lrows((size_t)nb), erows((size_t)nb);
    std::vector<long long> loff((size_t)nb + 1, 0), eoff((size_t)nb + 1, 0);
    for (int b = 0; b < nb; b++) {
        for (const RMatT * m : { (const RMatT *)leqs[(size_t)b], (const RMatT *)eqs[(size_t)b] })
            if (rows_of(m) > 0 && (int)m->get_col_size() != cols) return XPG_ERR_SHAPE;
        lrows[(size_t)b] = rows_of(leqs[(size_t)b]); erows[(size_t)b] = rows_of(eqs[(size_t)b]);
        loff[(size_t)b + 1] = loff[(size_t)b] + (long long)lrows[(size_t)b] * cols;
        eoff[(size_t)b + 1] = eoff[(size_t)b] + (long long)erows[(size_t)b] * cols;
    }
    std::vector<xpg_rat32> L((size_t)loff[(size_t)nb]), E((size_t)eoff[(size_t)nb]);
    for (int b = 0; b < nb; b++) {
        if (lrows[(size_t)b])
            std::memcpy((void *)(L.data() + loff[(size_t)b]), (const void *)leqs[(size_t)b]->get_matrix(), sizeof(xpg_rat32) * (size_t)lrows[(size_t)b] * cols);
        if (erows[(size_t)b])
            std::memcpy((void *)(E.data() + eoff[(size_t)b]), (const void *)eqs[(size_t)b]->get_matrix(), sizeof(xpg_rat32) * (size_t)erows[(size_t)b] * cols);
    }
    if (is_int_sol)      // the integer form on the device: objective, both walks and the verdict, one synchronisation per shape class
        return xpg_has_solution_int_batch_ragged_rat32(c ? c : detail::shared_context(), nb, L.empty() ? (const xpg_rat32 *)0 : L.data(),
                                                       lrows.data(), loff.data(), E.empty() ? (const xpg_rat32 *)0 : E.data(), erows.data(),
                                                       eoff.data(), (const xpg_rat32 *)vc.get_matrix(), rhs_idx, cols, rhs_idx,
                                                       is_unique_sol ? 1 : 0, out.data(), (int32_t *)0);
    return xpg_has_solution_batch_ragged_rat32(c ? c : detail::shared_context(), nb, L.empty() ? (const xpg_rat32 *)0 : L.data(), lrows.data(),
                                               loff.data(), E.empty() ? (const xpg_rat32 *)0 : E.data(), erows.data(), eoff.data(),
                                               (const xpg_rat32 *)vc.get_matrix(), rhs_idx, cols, rhs_idx, is_int_sol ? 1 : 0,
                                               is_unique_sol ? 1 : 0, 0xFFFFFFFFu, out.data(), (int32_t *)0);
}

// Many eliminations in ONE call: Lineq::fme(u[k], results[k]) (linsys.cpp:656-774) on systems of whatever shapes, the constant
// in column rhs_idx[k] (empty vector: the last column of each). The reference's hot callers eliminate level by level --
// loop-bound generation (src/eng/ldtran.cpp:178-193: for i = rhs_idx - 1 .. 1: fme(i)) and scanning (src/eng/poly.cpp:4803-4821) --
// one small system per call; collected over the statements of a SCoP a level becomes one launch. ok[k] is fme's bool.
// Returns 0 or a negative XPG_ERR_* code.
template <class RMatT>
inline int fme_all(const std::vector<RMatT *> & systems, const std::vector<int32_t> & u, const std::vector<int32_t> & rhs_idx,
                   std::vector<RMatT> & results, std::vector<int32_t> & ok, bool darkshadow = false, xpg_ctx * c = 0)
{
    const int nb = (int)systems.size();
    if ((int)u.size() != nb || (!rhs_idx.empty() && (int)rhs_idx.size() != nb)) return XPG_ERR_SHAPE;
    results.resize((size_t)nb); ok.assign((size_t)nb, 0);
    // empty systems stay empty (linsys.cpp:661-664) and do not travel
    std::vector<int> live;
    for (int b = 0; b < nb; b++) { if (systems[(size_t)b]->size() == 0) { results[(size_t)b].clean(); ok[(size_t)b] = 1; } else live.push_back(b); }
    const int nl = (int)live.size();
    if (nl == 0) return 0;
    std::vector<int32_t> rows((size_t)nl), cols((size_t)nl), uu((size_t)nl), rr((size_t)nl), orows((size_t)nl), ook((size_t)nl);
    std::vector<long long> off((size_t)nl + 1, 0), ooff((size_t)nl + 1, 0);
    for (int k = 0; k < nl; k++) {
        const RMatT & m = *systems[(size_t)live[(size_t)k]];
        rows[(size_t)k] = (int32_t)m.get_row_size(); cols[(size_t)k] = (int32_t)m.get_col_size();
        uu[(size_t)k] = u[(size_t)live[(size_t)k]];
        rr[(size_t)k] = rhs_idx.empty() ? cols[(size_t)k] - 1 : rhs_idx[(size_t)live[(size_t)k]];
        off[(size_t)k + 1] = off[(size_t)k] + (long long)rows[(size_t)k] * cols[(size_t)k];
    }
    std::vector<xpg_rat32> flat((size_t)off[(size_t)nl]);
    for (int k = 0; k < nl; k++)
        std::memcpy((void *)(flat.data() + off[(size_t)k]), (const void *)systems[(size_t)live[(size_t)k]]->get_matrix(),
                    sizeof(xpg_rat32) * (size_t)rows[(size_t)k] * cols[(size_t)k]);
    xpg_ctx * h = c ? c : detail::shared_context();
    // a buffer for the worst case of every result while that is small (one call), else a sizing call first
    long long capc = 0;
    for (int k = 0; k < nl; k++) capc += ((long long)rows[(size_t)k] * rows[(size_t)k] / 4 + rows[(size_t)k]) * cols[(size_t)k];
    std::vector<xpg_rat32> outs;
    int rc;
    if (capc * (long long)sizeof(xpg_rat32) <= (64ll << 20)) {
        outs.resize((size_t)(capc > 0 ? capc : 1));
        rc = xpg_lineq_fme_batch_ragged_rat32(h, nl, flat.data(), rows.data(), cols.data(), off.data(), rr.data(), uu.data(), darkshadow ? 1 : 0,
                                              outs.data(), capc, ooff.data(), orows.data(), ook.data());
    } else {
        rc = xpg_lineq_fme_batch_ragged_rat32(h, nl, flat.data(), rows.data(), cols.data(), off.data(), rr.data(), uu.data(), darkshadow ? 1 : 0,
                                              (xpg_rat32 *)0, 0, ooff.data(), orows.data(), ook.data());
        if (rc == XPG_ERR_SHAPE && ooff[(size_t)nl] > 0) {
            outs.resize((size_t)ooff[(size_t)nl]);
            rc = xpg_lineq_fme_batch_ragged_rat32(h, nl, flat.data(), rows.data(), cols.data(), off.data(), rr.data(), uu.data(), darkshadow ? 1 : 0,
                                                  outs.data(), ooff[(size_t)nl], ooff.data(), orows.data(), ook.data());
        }
    }
    if (rc != 0) return rc;
    for (int k = 0; k < nl; k++) {
        RMatT & res = results[(size_t)live[(size_t)k]];
        res.reinit(orows[(size_t)k], cols[(size_t)k]);
        if (orows[(size_t)k] * cols[(size_t)k])
            std::memcpy((void *)res.get_matrix(), (const void *)(outs.data() + ooff[(size_t)k]), sizeof(xpg_rat32) * (size_t)orows[(size_t)k] * cols[(size_t)k]);
        ok[(size_t)live[(size_t)k]] = ook[(size_t)k];
    }
    return 0;
}

// Many projections in few calls: the variables elim[0], elim[1], ... eliminated out of every *systems[k], each Lineq::fme's
// result the next one's input -- DepPoly::eliminateAuxVar's loop (src/eng/poly.cpp:643-651: for u = rhs - 1 .. l) and the
// scanning bounds (src/eng/poly.cpp:4807-4813) -- the constant in column rhs_idx of every system. Systems of one shape go up
// together, one xpg_lineq_project_batch_packed_rat32 call per shape class: every step of a system in one launch, only the
// final rows come back. ok[k] = 1 and results[k] the projection, or 0 (a step found the system inconsistent, as the loop's
// fme would return false) with results[k] empty. A class one of whose systems needs more rows than the capacity tried is
// called again with the need the library reports, at most three times; still short: XPG_ERR_UNSUPPORTED, never a silent
// empty result. Returns 0 or a negative XPG_ERR_* code.
template <class RMatT>
inline int project_all(const std::vector<RMatT *> & systems, const std::vector<int32_t> & elim, int rhs_idx,
                       std::vector<RMatT> & results, std::vector<int32_t> & ok, xpg_ctx * c = 0, bool darkshadow = false)
{
    const int nb = (int)systems.size();
    results.resize((size_t)nb); ok.assign((size_t)nb, 0);
    if (elim.empty() || rhs_idx < 1) return XPG_ERR_SHAPE;
    xpg_ctx * h = c ? c : detail::shared_context();
    std::vector<char> done((size_t)nb, 0);
    for (int b0 = 0; b0 < nb; b0++) {
        if (done[(size_t)b0]) continue;
        if (systems[(size_t)b0]->size() == 0) {                     // an empty system stays empty (linsys.cpp:661-664), no call
            results[(size_t)b0].clean(); ok[(size_t)b0] = 1; done[(size_t)b0] = 1;
            continue;
        }
        const int rows = (int)systems[(size_t)b0]->get_row_size(), cols = (int)systems[(size_t)b0]->get_col_size();
        std::vector<int> cls;
        for (int b = b0; b < nb; b++)
            if (!done[(size_t)b] && systems[(size_t)b]->size() != 0 && (int)systems[(size_t)b]->get_row_size() == rows &&
                (int)systems[(size_t)b]->get_col_size() == cols) {
                cls.push_back(b); done[(size_t)b] = 1;
            }
        const int nc = (int)cls.size();
        std::vector<xpg_rat32> flat((size_t)nc * rows * cols);
        for (int k = 0; k < nc; k++)
            std::memcpy((void *)(flat.data() + (size_t)k * rows * cols), (const void *)systems[(size_t)cls[(size_t)k]]->get_matrix(), sizeof(xpg_rat32) * (size_t)rows * cols);
        int cap = 0;                                                // the library's default first; the final slots take cap too
        bool answered = false;
        for (int attempt = 0; attempt < 3 && !answered; attempt++) {
            std::vector<long long> off((size_t)nc + 1, 0);
            std::vector<int32_t> kok((size_t)nc, 0), steps((size_t)nc, 0);
            const xpg_rat32 * view = 0;
            const int rc = xpg_lineq_project_batch_packed_rat32(h, nc, flat.data(), rows, cols, rhs_idx, elim.data(), (int)elim.size(),
                                                                darkshadow ? 1 : 0, cap, 0, (xpg_rat32 *)0, 0, &view, off.data(),
                                                                kok.data(), steps.data());
            if (rc != 0) return rc;
            int need = 0;
            for (int k = 0; k < nc; k++) if (kok[(size_t)k] < 0 && -kok[(size_t)k] > need) need = -kok[(size_t)k];
            if (need) { cap = need; continue; }                     // a step needed more rows than cap: once more with that many
            for (int k = 0; k < nc; k++) {
                const int b = cls[(size_t)k];
                const long long lo = off[(size_t)k], hi = off[(size_t)k + 1];
                ok[(size_t)b] = kok[(size_t)k];
                results[(size_t)b].reinit((unsigned)(hi - lo), (unsigned)cols);
                if (hi > lo) std::memcpy((void *)results[(size_t)b].get_matrix(), (const void *)(view + (size_t)lo * cols), sizeof(xpg_rat32) * (size_t)(hi - lo) * cols);
            }
            answered = true;
        }
        if (!answered) return XPG_ERR_UNSUPPORTED;
    }
    return 0;
}

// Loop-nest limits for many statements in few calls: the variables elim[0], elim[1], ... eliminated out of every *systems[k]
// as project_all does, but EVERY level is kept -- levels[k][step] is *systems[k] with elim[0 .. step] eliminated, the system
// that bounds one loop of the nest (LoopTran::transformIterSpace, src/eng/ldtran.cpp:178-196, :241-257, with elim =
// rhs_idx-1 .. 1; Lineq::fmeLevels above is the same for one system). Systems of one shape go up together, one
// xpg_lineq_levels_batch_packed_rat32 call per shape class: one launch instead of one fme_all call per level, no
// intermediate crosses the link twice. ok[k] = 1 with levels[k] filled, or 0 (a step found the system inconsistent) with
// every level of k empty. A class found short of rows is called again with the need the library reports -- above the
// capacity tried: a step's unreduced rows, cap_rows; else a level's slot, cap_out_rows -- at most four times; still short:
// XPG_ERR_UNSUPPORTED, never a silent empty level. Returns 0 or a negative XPG_ERR_* code.
template <class RMatT>
inline int levels_all(const std::vector<RMatT *> & systems, const std::vector<int32_t> & elim, int rhs_idx,
                      std::vector<std::vector<RMatT> > & levels, std::vector<int32_t> & ok, xpg_ctx * c = 0, bool darkshadow = false)
{
    const int nb = (int)systems.size(), n = (int)elim.size();
    levels.assign((size_t)nb, std::vector<RMatT>());
    ok.assign((size_t)nb, 0);
    if (elim.empty() || rhs_idx < 1) return XPG_ERR_SHAPE;
    xpg_ctx * h = c ? c : detail::shared_context();
    std::vector<char> done((size_t)nb, 0);
    for (int b0 = 0; b0 < nb; b0++) {
        if (done[(size_t)b0]) continue;
        if (systems[(size_t)b0]->size() == 0) {                     // an empty system stays empty (linsys.cpp:661-664), no call
            levels[(size_t)b0].resize((size_t)n);
            for (int k = 0; k < n; k++) levels[(size_t)b0][(size_t)k].clean();
            ok[(size_t)b0] = 1; done[(size_t)b0] = 1;
            continue;
        }
        const int rows = (int)systems[(size_t)b0]->get_row_size(), cols = (int)systems[(size_t)b0]->get_col_size();
        std::vector<int> cls;
        for (int b = b0; b < nb; b++)
            if (!done[(size_t)b] && systems[(size_t)b]->size() != 0 && (int)systems[(size_t)b]->get_row_size() == rows &&
                (int)systems[(size_t)b]->get_col_size() == cols) {
                cls.push_back(b); done[(size_t)b] = 1;
            }
        const int nc = (int)cls.size();
        std::vector<xpg_rat32> flat((size_t)nc * rows * cols);
        for (int k = 0; k < nc; k++)
            std::memcpy((void *)(flat.data() + (size_t)k * rows * cols), (const void *)systems[(size_t)cls[(size_t)k]]->get_matrix(), sizeof(xpg_rat32) * (size_t)rows * cols);
        int cap = rows * rows / 4 + rows + 1, cap_out = cap < 4 * rows + 16 ? cap : 4 * rows + 16;   // the library's defaults, spelled out
        bool answered = false;
        for (int attempt = 0; attempt < 4 && !answered; attempt++) {
            std::vector<long long> off((size_t)nc * n + 1, 0);
            std::vector<int32_t> kok((size_t)nc, 0), steps((size_t)nc, 0);
            const xpg_rat32 * view = 0;
            const int rc = xpg_lineq_levels_batch_packed_rat32(h, nc, flat.data(), rows, cols, rhs_idx, elim.data(), n, darkshadow ? 1 : 0,
                                                               cap, cap_out, (xpg_rat32 *)0, 0, &view, off.data(), kok.data(), steps.data());
            if (rc != 0) return rc;
            int need_cap = 0, need_out = 0;
            for (int k = 0; k < nc; k++) {
                const int need = -kok[(size_t)k];
                if (need > cap) { if (need > need_cap) need_cap = need; }
                else if (need > need_out) need_out = need;          // (need <= 0: the system was answered)
            }
            if (need_cap) cap = need_cap;
            if (need_out) cap_out = need_out;
            if (need_cap || need_out) continue;
            for (int k = 0; k < nc; k++) {
                const int b = cls[(size_t)k];
                ok[(size_t)b] = kok[(size_t)k];
                levels[(size_t)b].resize((size_t)n);
                for (int j = 0; j < n; j++) {
                    const long long lo = off[(size_t)k * n + j], hi = off[(size_t)k * n + j + 1];
                    RMatT & m = levels[(size_t)b][(size_t)j];
                    m.reinit((unsigned)(hi - lo), (unsigned)cols);
                    if (hi > lo) std::memcpy((void *)m.get_matrix(), (const void *)(view + (size_t)lo * cols), sizeof(xpg_rat32) * (size_t)(hi - lo) * cols);
                }
            }
            answered = true;
        }
        if (!answered) return XPG_ERR_UNSUPPORTED;
    }
    return 0;
}

namespace detail {
// What project_each and levels_nests share: the systems that travel (`live`: indices into `systems`, each with its list in
// `lists`) go up in ONE xpg_lineq_{project,levels}_batch_ragged_rat32 call whatever their shapes and lists; a call found
// short of rows is made again with the largest need reported -- above the capacity tried: a step's unreduced rows, cap_rows;
// else an output slot, cap_out_rows -- at most four times, then XPG_ERR_UNSUPPORTED. sink(i, k, cells, rows, cols) receives
// result k of live system i (k == 0 alone for a projection) out of the handle's pinned buffer, once every answer is there;
// ok[live[i]] the verdict (1, or 0: a step found the system inconsistent, every result of it empty).
template <class RMatT, class Sink>
inline int chain_ragged(bool levels, const std::vector<RMatT *> & systems, const std::vector<int> & live, const std::vector<std::vector<int32_t> > & lists,
                        const std::vector<int32_t> & rhs_idx, std::vector<int32_t> & ok, xpg_ctx * h, bool darkshadow, Sink sink)
{
    const int nl = (int)live.size();
    if (nl == 0) return 0;
    std::vector<int32_t> rows((size_t)nl), cols((size_t)nl), rr((size_t)nl), eoff((size_t)nl + 1, 0), flat_el;
    std::vector<long long> off((size_t)nl + 1, 0);
    for (int i = 0; i < nl; i++) {
        const RMatT & m = *systems[(size_t)live[(size_t)i]];
        rows[(size_t)i] = (int32_t)m.get_row_size(); cols[(size_t)i] = (int32_t)m.get_col_size();
        rr[(size_t)i] = rhs_idx[(size_t)live[(size_t)i]];
        off[(size_t)i + 1] = off[(size_t)i] + (long long)rows[(size_t)i] * cols[(size_t)i];
        flat_el.insert(flat_el.end(), lists[(size_t)i].begin(), lists[(size_t)i].end());
        eoff[(size_t)i + 1] = (int32_t)flat_el.size();
    }
    std::vector<xpg_rat32> flat((size_t)off[(size_t)nl]);
    for (int i = 0; i < nl; i++)
        std::memcpy((void *)(flat.data() + off[(size_t)i]), (const void *)systems[(size_t)live[(size_t)i]]->get_matrix(),
                    sizeof(xpg_rat32) * (size_t)rows[(size_t)i] * cols[(size_t)i]);
    const int nres = levels ? (int)flat_el.size() : nl;
    int cap = 0, cap_out = 0;                                       // the library's defaults first
    for (int attempt = 0; attempt < 4; attempt++) {
        std::vector<long long> ooff((size_t)nres + 1, 0);
        std::vector<int32_t> orows((size_t)nres, 0), kok((size_t)nl, 0), steps((size_t)nl, 0);
        const xpg_rat32 * view = 0;
        const int rc = (levels ? xpg_lineq_levels_batch_ragged_rat32 : xpg_lineq_project_batch_ragged_rat32)(
            h, nl, flat.data(), rows.data(), cols.data(), off.data(), rr.data(), flat_el.data(), eoff.data(), darkshadow ? 1 : 0, cap, cap_out,
            (xpg_rat32 *)0, 0, &view, ooff.data(), orows.data(), kok.data(), steps.data());
        if (rc != 0) return rc;
        if (cap == 0) {                                             // the capacities that call settled on (xpoly_amd.h), spelled out
            int most = 0;
            for (int i = 0; i < nl; i++) if (rows[(size_t)i] > most) most = rows[(size_t)i];
            cap = most * most / 4 + most + 1;
            cap_out = levels && 4 * most + 16 < cap ? 4 * most + 16 : cap;
        }
        int need_cap = 0, need_out = 0;
        for (int i = 0; i < nl; i++) {
            const int need = -kok[(size_t)i];
            if (need > cap) { if (need > need_cap) need_cap = need; }
            else if (need > need_out) need_out = need;              // (need <= 0: the system was answered)
        }
        if (need_cap) cap = need_cap;
        if (need_out) cap_out = need_out;
        if (!levels) cap_out = cap;                                 // (a projection's final slot takes cap)
        if (need_cap || need_out) continue;
        for (int i = 0; i < nl; i++) {
            ok[(size_t)live[(size_t)i]] = kok[(size_t)i];
            const int first = levels ? eoff[(size_t)i] : i, n = levels ? eoff[(size_t)i + 1] - eoff[(size_t)i] : 1;
            for (int k = 0; k < n; k++)
                sink(i, k, view ? view + ooff[(size_t)(first + k)] : view, (int)orows[(size_t)(first + k)], (int)cols[(size_t)i]);
        }
        return 0;
    }
    return XPG_ERR_UNSUPPORTED;
}
template <class RMatT> inline void put_cells(RMatT & m, const xpg_rat32 * a, int rows, int cols)
{
    m.reinit((unsigned)rows, (unsigned)cols);
    if (rows > 0 && cols > 0) std::memcpy((void *)m.get_matrix(), (const void *)a, sizeof(xpg_rat32) * (size_t)rows * cols);
}
} // namespace detail

// Many projections in ONE call whatever the shapes: project_all with a list and a constant column PER SYSTEM -- the variables
// elims[k][0], elims[k][1], ... eliminated out of *systems[k], the constant in column rhs_idx[k]. Statements of different depth
// (other rows, columns, rhs_idx and lists) go up together in one xpg_lineq_project_batch_ragged_rat32 call: one upload, one
// launch. ok[k] = 1 and results[k] the projection, or 0 (a step found the system inconsistent) with results[k] empty. Empty
// systems stay empty (linsys.cpp:661-664) and do not travel. A call found short of rows is made again with the largest need
// the library reports, at most four times; still short: XPG_ERR_UNSUPPORTED, never a silent empty result. Returns 0 or a
// negative XPG_ERR_* code (XPG_ERR_SHAPE: a missing or empty list).
template <class RMatT>
inline int project_each(const std::vector<RMatT *> & systems, const std::vector<std::vector<int32_t> > & elims, const std::vector<int32_t> & rhs_idx,
                        std::vector<RMatT> & results, std::vector<int32_t> & ok, xpg_ctx * c = 0, bool darkshadow = false)
{
    const int nb = (int)systems.size();
    results.resize((size_t)nb); ok.assign((size_t)nb, 0);
    if ((int)elims.size() != nb || (int)rhs_idx.size() != nb) return XPG_ERR_SHAPE;
    std::vector<int> live;
    std::vector<std::vector<int32_t> > lists;
    for (int b = 0; b < nb; b++) {
        if (elims[(size_t)b].empty() || rhs_idx[(size_t)b] < 1) return XPG_ERR_SHAPE;
        if (systems[(size_t)b]->size() == 0) { results[(size_t)b].clean(); ok[(size_t)b] = 1; }
        else { live.push_back(b); lists.push_back(elims[(size_t)b]); }
    }
    return detail::chain_ragged(false, systems, live, lists, rhs_idx, ok, c ? c : detail::shared_context(), darkshadow,
                                [&](int i, int, const xpg_rat32 * a, int r, int cc) { detail::put_cells(results[(size_t)live[(size_t)i]], a, r, cc); });
}

// Loop-nest limits for the statements of a SCoP in ONE call: levels_all for nests of DIFFERENT depths. System k has rhs_idx[k]
// variables and is walked as LoopTran::transformIterSpace walks it (src/eng/ldtran.cpp:178-196, :241-257): rhs_idx[k]-1 .. 1
// eliminated one after the other, levels[k][step] the system after step `step` (rhs_idx[k] - 1 of them; Lineq::fmeLevels is
// the same for one system). All nests that have something to eliminate go up in one xpg_lineq_levels_batch_ragged_rat32 call:
// one upload, one launch, no intermediate crosses the link twice. Empty systems and nests of depth 1 are answered here, as
// fmeLevels answers them: ok 1, every level (none at depth 1) empty. ok[k] = 0: a step found the system inconsistent, every
// level of k empty. Retries and return codes as project_each.
template <class RMatT>
inline int levels_nests(const std::vector<RMatT *> & systems, const std::vector<int32_t> & rhs_idx, std::vector<std::vector<RMatT> > & levels,
                        std::vector<int32_t> & ok, xpg_ctx * c = 0, bool darkshadow = false)
{
    const int nb = (int)systems.size();
    levels.assign((size_t)nb, std::vector<RMatT>());
    ok.assign((size_t)nb, 0);
    if ((int)rhs_idx.size() != nb) return XPG_ERR_SHAPE;
    std::vector<int> live;
    std::vector<std::vector<int32_t> > lists;
    for (int b = 0; b < nb; b++) {
        const int nv = rhs_idx[(size_t)b];
        if (nv < 1) return XPG_ERR_SHAPE;
        levels[(size_t)b].resize((size_t)(nv - 1));
        if (nv == 1 || systems[(size_t)b]->size() == 0) {          // nothing to eliminate, or an empty system: it stays empty
            for (int k = 0; k + 1 < nv; k++) levels[(size_t)b][(size_t)k].clean();
            ok[(size_t)b] = 1;
            continue;
        }
        std::vector<int32_t> el;
        for (int u = nv - 1; u > 0; u--) el.push_back(u);
        live.push_back(b); lists.push_back(el);
    }
    return detail::chain_ragged(true, systems, live, lists, rhs_idx, ok, c ? c : detail::shared_context(), darkshadow,
                                [&](int i, int k, const xpg_rat32 * a, int r, int cc) { detail::put_cells(levels[(size_t)live[(size_t)i]][(size_t)k], a, r, cc); });
}

// Lineq::calcBound (linsys.cpp:1047-1078) for many systems: limits[k][j] receives the bounds of variable j of *systems[k]
// alone (the constant in column rhs_idx[k]); ok[k] is calcBound's bool. Systems of one shape go up together -- one call per
// shape class (SCoPs have a handful), xpg_lineq_bounds_batch_packed_rat32: every elimination chain of a class in one launch.
// A class one of whose systems needs more rows than the capacity tried is called again with the largest need the library
// reports, at most three times; still short: XPG_ERR_UNSUPPORTED, never a silent ok = 0. Returns 0 or XPG_ERR_*.
// (Systems of MIXED shapes in one call and one launch: calc_bound_each, below.)
template <class RMatT>
inline int calc_bound_all(const std::vector<RMatT *> & systems, const std::vector<int32_t> & rhs_idx,
                          std::vector<std::vector<RMatT> > & limits, std::vector<int32_t> & ok, xpg_ctx * c = 0)
{
    const int nb = (int)systems.size();
    if ((int)rhs_idx.size() != nb) return XPG_ERR_SHAPE;
    limits.assign((size_t)nb, std::vector<RMatT>());
    ok.assign((size_t)nb, 0);
    xpg_ctx * h = c ? c : detail::shared_context();
    std::vector<char> done((size_t)nb, 0);
    for (int b0 = 0; b0 < nb; b0++) {
        if (done[(size_t)b0]) continue;
        const int rows = (int)systems[(size_t)b0]->get_row_size(), cols = (int)systems[(size_t)b0]->get_col_size(), nv = rhs_idx[(size_t)b0];
        std::vector<int> cls;
        for (int b = b0; b < nb; b++)
            if (!done[(size_t)b] && (int)systems[(size_t)b]->get_row_size() == rows && (int)systems[(size_t)b]->get_col_size() == cols && rhs_idx[(size_t)b] == nv) {
                cls.push_back(b); done[(size_t)b] = 1;
            }
        if (rows == 0 || cols == 0 || nv < 1 || nv >= cols) return XPG_ERR_SHAPE;
        const int nc = (int)cls.size();
        std::vector<xpg_rat32> flat((size_t)nc * rows * cols);
        for (int k = 0; k < nc; k++)
            std::memcpy((void *)(flat.data() + (size_t)k * rows * cols), (const void *)systems[(size_t)cls[(size_t)k]]->get_matrix(), sizeof(xpg_rat32) * (size_t)rows * cols);
        int cap = 4 * rows + 16;
        bool answered = false;
        for (int attempt = 0; attempt < 3 && !answered; attempt++) {
            std::vector<long long> off((size_t)nc * nv + 1, 0);
            std::vector<int32_t> kok((size_t)nc, 0), kchain((size_t)nc, 0), ksteps((size_t)nc, 0);
            const xpg_rat32 * view = 0;
            const int rc = xpg_lineq_bounds_batch_packed_rat32(h, nc, flat.data(), rows, cols, nv, cap, 0, (xpg_rat32 *)0, 0, &view, off.data(),
                                                               kok.data(), kchain.data(), ksteps.data());
            if (rc != 0) return rc;
            int need = 0;
            for (int k = 0; k < nc; k++) if (kok[(size_t)k] < 0 && -kok[(size_t)k] > need) need = -kok[(size_t)k];
            if (need) { cap = need; continue; }                     // a step needed more rows than cap: once more with that many
            for (int k = 0; k < nc; k++) {
                const int b = cls[(size_t)k];
                ok[(size_t)b] = kok[(size_t)k];
                limits[(size_t)b].resize((size_t)nv);
                for (int j = 0; j < nv; j++) {
                    const long long lo = off[(size_t)k * nv + j], hi = off[(size_t)k * nv + j + 1];
                    RMatT & m = limits[(size_t)b][(size_t)j];
                    m.reinit((unsigned)(hi - lo), (unsigned)cols);
                    if (hi > lo) std::memcpy((void *)m.get_matrix(), (const void *)(view + (size_t)lo * cols), sizeof(xpg_rat32) * (size_t)(hi - lo) * cols);
                }
            }
            answered = true;
        }
        if (!answered) return XPG_ERR_UNSUPPORTED;
    }
    return 0;
}

// calc_bound_all for systems of MIXED shapes in ONE call: the same arguments, limits and ok, but every system -- whatever its
// rows, columns and rhs_idx -- is packed once and goes up in one xpg_lineq_bounds_batch_ragged_rat32 call: one upload, one
// launch, one synchronisation instead of one of each per shape class. The capacities are the call's (the library's default,
// 4 * most rows + 16, first). Where a system reports -need the call is made again with the largest need reported -- above the
// capacity tried: a step's unreduced rows, cap_rows; else an output slot, cap_out_rows -- at most three times; still short:
// XPG_ERR_UNSUPPORTED, never a silent ok = 0. Returns 0 or XPG_ERR_*.
template <class RMatT>
inline int calc_bound_each(const std::vector<RMatT *> & systems, const std::vector<int32_t> & rhs_idx,
                           std::vector<std::vector<RMatT> > & limits, std::vector<int32_t> & ok, xpg_ctx * c = 0)
{
    const int nb = (int)systems.size();
    if ((int)rhs_idx.size() != nb) return XPG_ERR_SHAPE;
    limits.assign((size_t)nb, std::vector<RMatT>());
    ok.assign((size_t)nb, 0);
    if (nb == 0) return 0;
    xpg_ctx * h = c ? c : detail::shared_context();
    std::vector<int32_t> rows((size_t)nb), cols((size_t)nb);
    std::vector<long long> off((size_t)nb + 1, 0);
    std::vector<int> first((size_t)nb + 1, 0);
    int most = 0;
    for (int b = 0; b < nb; b++) {
        rows[(size_t)b] = (int32_t)systems[(size_t)b]->get_row_size(); cols[(size_t)b] = (int32_t)systems[(size_t)b]->get_col_size();
        const int nv = rhs_idx[(size_t)b];
        if (rows[(size_t)b] == 0 || cols[(size_t)b] == 0 || nv < 1 || nv >= cols[(size_t)b]) return XPG_ERR_SHAPE;
        off[(size_t)b + 1] = off[(size_t)b] + (long long)rows[(size_t)b] * cols[(size_t)b];
        first[(size_t)b + 1] = first[(size_t)b] + nv;
        if (rows[(size_t)b] > most) most = rows[(size_t)b];
    }
    std::vector<xpg_rat32> flat((size_t)off[(size_t)nb]);
    for (int b = 0; b < nb; b++)
        std::memcpy((void *)(flat.data() + off[(size_t)b]), (const void *)systems[(size_t)b]->get_matrix(),
                    sizeof(xpg_rat32) * (size_t)rows[(size_t)b] * cols[(size_t)b]);
    const int nres = first[(size_t)nb];
    int cap = 4 * most + 16, cap_out = cap;                         // the library's defaults, spelled out
    for (int attempt = 0; attempt < 3; attempt++) {
        std::vector<long long> ooff((size_t)nres + 1, 0);
        std::vector<int32_t> orows((size_t)nres, 0), kok((size_t)nb, 0), kchain((size_t)nb, 0), ksteps((size_t)nb, 0);
        const xpg_rat32 * view = 0;
        const int rc = xpg_lineq_bounds_batch_ragged_rat32(h, nb, flat.data(), rows.data(), cols.data(), off.data(), rhs_idx.data(), cap, cap_out,
                                                           (xpg_rat32 *)0, 0, &view, ooff.data(), orows.data(), kok.data(), kchain.data(),
                                                           ksteps.data());
        if (rc != 0) return rc;
        int need_cap = 0, need_out = 0;
        for (int b = 0; b < nb; b++) {
            const int need = -kok[(size_t)b];
            if (need > cap) { if (need > need_cap) need_cap = need; }
            else if (need > need_out) need_out = need;              // (need <= 0: the system was answered)
        }
        if (need_cap) { cap = need_cap; cap_out = cap; }            // (a result's slot takes cap, as in calc_bound_all)
        else if (need_out) cap_out = need_out;
        if (need_cap || need_out) continue;
        for (int b = 0; b < nb; b++) {
            const int nv = rhs_idx[(size_t)b];
            ok[(size_t)b] = kok[(size_t)b];
            limits[(size_t)b].resize((size_t)nv);
            for (int j = 0; j < nv; j++) {
                const int r = first[(size_t)b] + j;
                detail::put_cells(limits[(size_t)b][(size_t)j], view ? view + ooff[(size_t)r] : view, (int)orows[(size_t)r], (int)cols[(size_t)b]);
            }
        }
        return 0;
    }
    return XPG_ERR_UNSUPPORTED;
}

namespace detail {
// The one call behind the hull collectors: the members of every group packed once, xpg_lineq_hull_batch_ragged_rat32 (elims
// NULL) or xpg_lineq_project_union_batch_ragged_rat32. Where a group reports -need the call is made again with the largest need
// reported -- of a member (above the cap_rows tried: a step's unreduced rows; else a result's slot, cap_out_rows) or of a group
// (member -1: cap_hull_rows) -- at most three times; still short: XPG_ERR_UNSUPPORTED.
template <class RMatT>
inline int hull_groups(const std::vector<std::vector<RMatT *> > & groups, const std::vector<int32_t> & rhs_idx,
                       const std::vector<std::vector<std::vector<int32_t> > > * elims, bool darkshadow, bool is_intersect, std::vector<RMatT> & results,
                       std::vector<int32_t> & ok, std::vector<int32_t> * member, xpg_ctx * c)
{
    const int ng = (int)groups.size();
    if ((int)rhs_idx.size() != ng || (elims && (int)elims->size() != ng)) return XPG_ERR_SHAPE;
    results.assign((size_t)ng, RMatT());
    ok.assign((size_t)ng, 0);
    if (member) member->assign((size_t)ng, -1);
    if (ng == 0) return 0;
    xpg_ctx * h = c ? c : shared_context();
    std::vector<int32_t> goff((size_t)ng + 1, 0), rows, cols, rhs, elim, eoff(1, 0);
    std::vector<long long> off(1, 0);
    int most = 0;
    for (int g = 0; g < ng; g++) {
        const std::vector<RMatT *> & grp = groups[(size_t)g];
        if (elims && (*elims)[(size_t)g].size() != grp.size()) return XPG_ERR_SHAPE;
        for (size_t i = 0; i < grp.size(); i++) {
            const int r = grp[i]->size() == 0 ? 0 : (int)grp[i]->get_row_size(), cc = (int)grp[i]->get_col_size();
            if (r == 0 || cc == 0) return XPG_ERR_SHAPE;
            rows.push_back(r); cols.push_back(cc); rhs.push_back(rhs_idx[(size_t)g]);
            off.push_back(off.back() + (long long)r * cc);
            if (r > most) most = r;
            if (elims) {
                const std::vector<int32_t> & e = (*elims)[(size_t)g][i];
                elim.insert(elim.end(), e.begin(), e.end());
                eoff.push_back((int32_t)elim.size());
            }
        }
        goff[(size_t)g + 1] = goff[(size_t)g] + (int32_t)grp.size();
    }
    const int nb = goff[(size_t)ng];
    std::vector<xpg_rat32> flat((size_t)off.back() + 1);
    for (int g = 0, b = 0; g < ng; g++)
        for (size_t i = 0; i < groups[(size_t)g].size(); i++, b++)
            std::memcpy((void *)(flat.data() + off[(size_t)b]), (const void *)groups[(size_t)g][i]->get_matrix(),
                        sizeof(xpg_rat32) * (size_t)rows[(size_t)b] * cols[(size_t)b]);
    if (elim.empty()) elim.push_back(0);
    int cap = elims ? most * most / 4 + most + 1 : 4 * most + 16, cap_out = cap, cap_hull = 0;   // the library's defaults, spelled out
    for (int attempt = 0; attempt < 3; attempt++) {
        std::vector<long long> ooff((size_t)ng + 1, 0);
        std::vector<int32_t> orows((size_t)ng, 0), kok((size_t)ng, 0), kmem((size_t)ng, 0), kchain((size_t)ng, 0), ksteps((size_t)ng, 0);
        const xpg_rat32 * view = 0;
        const int rc = elims
            ? xpg_lineq_project_union_batch_ragged_rat32(h, ng, goff.data(), nb, flat.data(), rows.data(), cols.data(), off.data(), rhs.data(),
                                                         elim.data(), eoff.data(), darkshadow ? 1 : 0, is_intersect ? 1 : 0, cap, cap_out, cap_hull,
                                                         (xpg_rat32 *)0, 0, &view, ooff.data(), orows.data(), kok.data(), kmem.data(), kchain.data(),
                                                         ksteps.data())
            : xpg_lineq_hull_batch_ragged_rat32(h, ng, goff.data(), nb, flat.data(), rows.data(), cols.data(), off.data(), rhs.data(),
                                                is_intersect ? 1 : 0, cap, cap_out, cap_hull, (xpg_rat32 *)0, 0, &view, ooff.data(), orows.data(),
                                                kok.data(), kmem.data(), kchain.data(), ksteps.data());
        if (rc != 0) return rc;
        int need_cap = 0, need_out = 0, need_hull = 0;
        for (int g = 0; g < ng; g++) {
            const int need = -kok[(size_t)g];
            if (need <= 0) continue;                                // the group was answered
            if (kmem[(size_t)g] < 0) { if (need > need_hull) need_hull = need; }
            else if (need > cap) { if (need > need_cap) need_cap = need; }
            else if (need > need_out) need_out = need;
        }
        if (need_cap) { cap = need_cap; cap_out = cap; }
        else if (need_out) cap_out = need_out;
        if (need_hull) cap_hull = need_hull;
        if (need_cap || need_out || need_hull) continue;
        for (int g = 0; g < ng; g++) {
            ok[(size_t)g] = kok[(size_t)g];
            if (member) (*member)[(size_t)g] = kmem[(size_t)g];
            if (orows[(size_t)g] > 0) put_cells(results[(size_t)g], view + ooff[(size_t)g], (int)orows[(size_t)g], (int)cols[(size_t)goff[(size_t)g]]);
            else results[(size_t)g].clean();
        }
        return 0;
    }
    return XPG_ERR_UNSUPPORTED;
}
} // namespace detail

// Lineq::ConvexHullUnionAndIntersect (linsys.cpp:283-336) for MANY lists of polyhedra in ONE call -- the hull of the statements
// that share a loop, of the access regions per array: groups[g] is a list of polyhedra that share their columns, rhs_idx[g] its
// constant column. calcBound on every member of every group in one launch, ONE reduce per group in a second, one upload and one
// synchronisation (xpg_lineq_hull_batch_ragged_rat32). results[g] receives the hull (cleaned where it has no rows), ok[g] 1; 0
// where reduce found the group inconsistent (is_intersect: results[g] cleaned) or calcBound found a member inconsistent -- then
// (*member)[g] (may be NULL) is that member's index, else -1, and results[g] is cleaned: the stated deviation from the reference,
// which goes on with stale bounds. A call found short of rows is made again with the largest need reported, at most three
// times; still short: XPG_ERR_UNSUPPORTED. Returns 0 or XPG_ERR_*.
template <class RMatT>
inline int hull_all(const std::vector<std::vector<RMatT *> > & groups, const std::vector<int32_t> & rhs_idx, bool is_intersect,
                    std::vector<RMatT> & results, std::vector<int32_t> & ok, xpg_ctx * c = 0, std::vector<int32_t> * member = 0)
{
    return detail::hull_groups(groups, rhs_idx, (const std::vector<std::vector<std::vector<int32_t> > > *)0, false, is_intersect, results, ok, member, c);
}

// The projected union of PolyTran::step_4 (src/eng/poly.cpp:4802-4823) for many groups in ONE call: member i of group g is
// projected by its own list elims[g][i] (one launch of the ragged chain kernel), the results of a group are concatenated in list
// order and ONE reduce(ub, rhs_idx[g], is_intersect) runs per group (step_4 passes false). Arguments, verdicts and retries as
// hull_all (xpg_lineq_project_union_batch_ragged_rat32).
template <class RMatT>
inline int project_union_each(const std::vector<std::vector<RMatT *> > & groups, const std::vector<std::vector<std::vector<int32_t> > > & elims,
                              const std::vector<int32_t> & rhs_idx, bool is_intersect, std::vector<RMatT> & results, std::vector<int32_t> & ok,
                              xpg_ctx * c = 0, bool darkshadow = false, std::vector<int32_t> * member = 0)
{
    return detail::hull_groups(groups, rhs_idx, &elims, darkshadow, is_intersect, results, ok, member, c);
}

} // namespace xpoly_amd
#endif
