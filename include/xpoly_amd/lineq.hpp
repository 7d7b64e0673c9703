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
// levels_all, project_each, levels_nests, calc_bound_all, calc_bound_each, hull_all, project_union_each, transform_levels_all
// (and LoopTran<RMat>, the reference's LoopTran::transformIterSpace on top of it) -- take the caller's
// matrix objects and make those calls). Header only; relies on the Matrix<Rational> contract only: get_row_size(), get_col_size(),
// get_matrix() (row-major {int32 num; int32 den}, matt.h:152-156, rational.h:66-67), size(), reinit(r, c).
#ifndef XPOLY_AMD_LINEQ_HPP
#define XPOLY_AMD_LINEQ_HPP

#include <cstddef>
#include <cstring>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>
#include "../xpoly_amd.h"
#include "six.hpp"

namespace xpoly_amd {

namespace detail {
// ---- what every collector below is made of, stated once (tests/cxx/collectors_trace.cpp pins what they do)
inline xpg_ctx * ctx_or_shared(xpg_ctx * c) { return c ? c : shared_context(); }

template <class RMatT> inline void put_cells(RMatT & m, const xpg_rat32 * a, int rows, int cols)
{
    m.reinit((unsigned)rows, (unsigned)cols);
    if (rows > 0 && cols > 0) std::memcpy((void *)m.get_matrix(), (const void *)a, sizeof(xpg_rat32) * (size_t)rows * cols);
}

// One packed view of a list of matrices: rows, cols and cell offsets of each, their cells back to back in list order, the
// largest row count. at(i) is matrix i (a pointer), shape_of(m) the rows and columns it travels with: the rule for what counts
// as having none is the caller's. A class of equal shapes is the same pack -- [n][rows][cols], what the _packed_ entry points
// take -- under the rule that knows its shape and does not ask each member again.
struct packed {
    std::vector<int32_t> rows, cols;
    std::vector<long long> off;
    std::vector<xpg_rat32> flat;                                    // (never without a cell: data() is no null pointer)
    int most;
    long long cells() const { return off.back(); }
};
struct shape_as_is { template <class M> std::pair<int, int> operator()(const M * m) const { return std::make_pair((int)m->get_row_size(), (int)m->get_col_size()); } };
struct shape_known { int rows, cols; template <class M> std::pair<int, int> operator()(const M *) const { return std::make_pair(rows, cols); } };
template <class At, class Shape> inline packed pack(int n, At at, Shape shape_of)
{
    packed p;
    p.rows.resize((size_t)n); p.cols.resize((size_t)n); p.off.assign((size_t)n + 1, 0); p.most = 0;
    for (int i = 0; i < n; i++) {
        const std::pair<int, int> shape = shape_of(at(i));
        p.rows[(size_t)i] = (int32_t)shape.first; p.cols[(size_t)i] = (int32_t)shape.second;
        p.off[(size_t)i + 1] = p.off[(size_t)i] + (long long)p.rows[(size_t)i] * p.cols[(size_t)i];
        if (p.rows[(size_t)i] > p.most) p.most = p.rows[(size_t)i];
    }
    p.flat.resize((size_t)(p.cells() ? p.cells() : 1));
    for (int i = 0; i < n; i++)
        if (p.off[(size_t)i + 1] > p.off[(size_t)i])
            std::memcpy((void *)(p.flat.data() + p.off[(size_t)i]), (const void *)at(i)->get_matrix(),
                        sizeof(xpg_rat32) * (size_t)(p.off[(size_t)i + 1] - p.off[(size_t)i]));
    return p;
}
template <class RMatT, class Shape> inline packed pack(const std::vector<RMatT *> & systems, const std::vector<int> & which, Shape shape_of)
{ return pack((int)which.size(), [&](int i) { return (const RMatT *)systems[(size_t)which[(size_t)i]]; }, shape_of); }

// The systems that travel: empty ones stay empty (linsys.cpp:661-664) and are answered by the caller's answer_empty(b).
template <class RMatT, class Answer> inline std::vector<int> live_systems(const std::vector<RMatT *> & systems, Answer answer_empty)
{
    std::vector<int> live;
    for (int b = 0; b < (int)systems.size(); b++) { if (systems[(size_t)b]->size() == 0) answer_empty(b); else live.push_back(b); }
    return live;
}
// One class walk: fn(cls) receives the members of `which` whose key_of(b) equals that of the first one not yet handed out, in
// the caller's order; classes come in order of first appearance. A non-zero return of fn ends the walk and is returned.
struct class_key {
    int rows, cols, more;                                           // more: what else the caller tells classes apart by
    bool operator==(const class_key & o) const { return rows == o.rows && cols == o.cols && more == o.more; }
};
template <class RMatT> inline class_key shape_of(const std::vector<RMatT *> & systems, int b, int more = 0)
{ const class_key k = { (int)systems[(size_t)b]->get_row_size(), (int)systems[(size_t)b]->get_col_size(), more }; return k; }
template <class Key, class Fn> inline int for_each_class(const std::vector<int> & which, Key key_of, Fn fn)
{
    std::vector<class_key> keys;                                    // (SCoPs have a handful of classes: a linear search)
    std::vector<std::vector<int> > classes;
    for (size_t i = 0; i < which.size(); i++) {
        const class_key k = key_of(which[i]);
        size_t j = 0;
        while (j < keys.size() && !(keys[j] == k)) j++;
        if (j == keys.size()) { keys.push_back(k); classes.push_back(std::vector<int>()); }
        classes[j].push_back(which[i]);
    }
    for (size_t j = 0; j < classes.size(); j++) {
        const int rc = fn(classes[j]);
        if (rc != 0) return rc;
    }
    return 0;
}

// One retry rule. A system (group) that reports -need was short of rows; the call is made again with the capacity it was short
// of raised to the largest need reported: of a group itself (member -1) cap_hull_rows; above the cap_rows tried a step's
// unreduced rows, cap_rows; else an output slot, cap_out_rows. What differs between the collectors is data:
struct caps { int cap, out, hull; };                                // cap_rows, cap_out_rows, cap_hull_rows; 0: the library's default
enum slot_rule {
    one_capacity,                                                   // cap_out_rows stays 0 (the slots take cap_rows): EVERY need sets cap_rows
    own_slot,                                                       // a slot's need raises cap_out_rows alone
    slot_follows,                                                   // the same, and a raised cap_rows is the slots' as well
    slot_is_cap                                                     // the slots take cap_rows whatever was short
};
struct retry_rule {
    caps first;                                                     // what the first call passes
    caps spelled;                                                   // cap != 0: the defaults that call settled on, spelled out after it
    slot_rule slot;
    bool groups;                                                    // the verdicts are groups': member -1 is the group's own need
    int attempts;                                                   // calls at the most; still short: XPG_ERR_UNSUPPORTED
};
// What a call answers with: the view into the handle's pinned buffer, an offset (and, the ragged forms, a row count) per result,
// a verdict, member, chain and step count per system or group -- each entry point fills the ones it has. Plain pointers into one
// block the driver owns: a sink receives a copy.
struct answer {
    const xpg_rat32 * view;
    long long * off;
    int32_t * rows, * ok, * member, * chain, * steps;
    // result r where the offsets count ROWS of `cols` columns (the packed forms) ...
    const xpg_rat32 * packed_at(size_t r, int cols) const { return view ? view + (size_t)off[r] * cols : view; }
    int packed_rows(size_t r) const { return (int)(off[r + 1] - off[r]); }
    template <class RMatT> void put_packed(RMatT & m, size_t r, int cols) const { put_cells(m, packed_at(r, cols), packed_rows(r), cols); }
    // ... and where they count cells and every result has a row count of its own (the ragged forms)
    const xpg_rat32 * ragged_at(size_t r) const { return view ? view + off[r] : view; }
    template <class RMatT> void put_ragged(RMatT & m, size_t r, int cols) const { put_cells(m, ragged_at(r), (int)rows[r], cols); }
};
// reads the verdicts of a call: true = all answered, else the right capacity is raised
inline bool answered(const retry_rule & how, caps & c, const answer & a, size_t systems)
{
    int need_cap = 0, need_out = 0, need_hull = 0;
    for (size_t i = 0; i < systems; i++) {
        const int need = -a.ok[i];
        if (need <= 0) continue;                                    // answered
        if (how.groups && a.member[i] < 0) { if (need > need_hull) need_hull = need; }
        else if (how.slot == one_capacity || need > c.cap) { if (need > need_cap) need_cap = need; }
        else if (need > need_out) need_out = need;
    }
    if (need_cap) c.cap = need_cap;
    if (how.slot == slot_follows && need_cap) c.out = c.cap;
    else if (need_out) c.out = need_out;
    if (how.slot == slot_is_cap) c.out = c.cap;
    if (need_hull) c.hull = need_hull;
    return !(need_cap || need_out || need_hull);
}
// call(capacities, answer) makes the library call for `systems` systems (groups) with `results` results in all; sink(answer)
// takes the results once every answer is there. Returns the call's code as soon as it is not 0, else 0, or XPG_ERR_UNSUPPORTED:
// never a silent empty result.
template <class Call, class Sink>
inline int call_until_answered(const retry_rule & how, size_t systems, size_t results, Call call, Sink sink)
{
    caps c = how.first;
    const size_t room = results + 1 + (results + 4 * systems + 1) / 2;   // in long long: the offsets, then the five int32 arrays
    long long few[64];                                              // (a batch of one, a small class: no allocation)
    const std::unique_ptr<long long[]> many(room > 64 ? new long long[room] : (long long *)0);
    answer a;
    a.off = room > 64 ? many.get() : few; a.rows = (int32_t *)(void *)(a.off + results + 1); a.ok = a.rows + results;
    a.member = a.ok + systems; a.chain = a.member + systems; a.steps = a.chain + systems;
    for (int attempt = 0; attempt < how.attempts; attempt++) {
        std::memset((void *)a.off, 0, sizeof(long long) * room);
        a.view = 0;
        const int rc = call(c, a);
        if (rc != 0) return rc;
        if (attempt == 0 && how.spelled.cap) c = how.spelled;
        if (answered(how, c, a, systems)) { const answer got = a; sink(got); return 0; }
    }
    return XPG_ERR_UNSUPPORTED;
}
inline int chain_default(int rows) { return rows * rows / 4 + rows + 1; }     // the library's default cap_rows of an fme chain
inline int bound_default(int rows) { return 4 * rows + 16; }                  // of a calcBound walk, and a level's slot at the most

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
    xpg_ctx * ctx() { return detail::ctx_or_shared(m_ctx); }
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
        detail::put_cells(m, a.data(), kept, cols);
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
        if (xpg_lineq_remove_iden_batch_rat32(ctx(), 1, a.data(), rows, cols, &kept) == 0) detail::put_cells(m, a.data(), kept, cols);
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
        detail::put_cells(res, view, (int)off[1], cols);
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
    // sink(j, cells, rows, cols): variable j's bounds, read straight out of the handle's pinned buffer once they are all there.
    // A capacity found short is set to the need reported and the call made once more.
    template <class Sink> bool calc_bound_into(Sink sink)
    {
        // the packed form: only the live rows of the nv bound systems travel
        const int rows = (int)m_coeff->get_row_size(), cols = (int)m_coeff->get_col_size(), nv = m_rhs_idx;
        const detail::retry_rule how = { { detail::bound_default(rows), 0, 0 }, { 0, 0, 0 }, detail::one_capacity, false, 2 };
        bool consistent = false;
        return detail::call_until_answered(how, 1, (size_t)nv,
            [&](const detail::caps & c, detail::answer & a) {
                return xpg_lineq_bounds_batch_packed_rat32(ctx(), 1, (const xpg_rat32 *)m_coeff->get_matrix(), rows, cols, nv, c.cap, c.out,
                                                           (xpg_rat32 *)0, 0, &a.view, a.off, a.ok, a.chain, a.steps);
            },
            [&](const detail::answer & a) {
                if (a.ok[0] == 0) return;                        // "system inconsistency!" (linsys.cpp:1065-1068)
                consistent = true;
                for (int j = 0; j < nv; j++) sink(j, a.packed_at((size_t)j, cols), a.packed_rows((size_t)j), cols);
            }) == 0 && consistent;
    }
public:
    bool calcBound(std::vector<RMatT> & limits)
    {
        limits.resize((size_t)m_rhs_idx);
        return calc_bound_into([&](int j, const xpg_rat32 * a, int r, int c) { detail::put_cells(limits[(size_t)j], a, r, c); });
    }
    template <class ListT, class = decltype(std::declval<ListT &>().get_head_nth(0u)), class = decltype(std::declval<ListT &>().get_elem_count())>
    bool calcBound(ListT & limits)
    {
        if ((int)limits.get_elem_count() != m_rhs_idx) return false;      // the reference ASSERTs (linsys.cpp:1050-1051)
        return calc_bound_into([&](int j, const xpg_rat32 * a, int r, int c) { detail::put_cells(*limits.get_head_nth((unsigned)j), a, r, c); });
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
        const int cap = detail::chain_default(rows);
        const detail::retry_rule how = { { cap, cap < detail::bound_default(rows) ? cap : detail::bound_default(rows), 0 }, { 0, 0, 0 }, detail::own_slot, false, 4 };
        bool consistent = false;
        return detail::call_until_answered(how, 1, (size_t)n,
            [&](const detail::caps & c, detail::answer & a) {
                return xpg_lineq_levels_batch_packed_rat32(ctx(), 1, in, rows, cols, nv, elim.data(), n, 0, c.cap, c.out, (xpg_rat32 *)0, 0, &a.view,
                                                           a.off, a.ok, a.steps);
            },
            [&](const detail::answer & a) {
                if (a.ok[0] == 0) return;                        // "system inconsistency!" (ldtran.cpp:186-188)
                consistent = true;
                sink(0, in, rows, cols);
                for (int k = 0; k < n; k++) sink(k + 1, a.packed_at((size_t)k, cols), a.packed_rows((size_t)k), cols);
            }) == 0 && consistent;
    }
public:
    bool fmeLevels(std::vector<RMatT> & aux_limits, RMatT * A = 0)
    {
        if (m_rhs_idx < 1) return false;
        const size_t nv = (size_t)m_rhs_idx;
        std::vector<RMatT> got(nv);
        if (!levels_into([&](int pos, const xpg_rat32 * a, int r, int c) { detail::put_cells(got[nv - 1 - (size_t)pos], a, r, c); })) return false;
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
        if (!levels_into([&](int pos, const xpg_rat32 * a, int r, int c) { detail::put_cells(*dst[(size_t)pos], a, r, c); })) return false;
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
    const detail::packed p = detail::pack((int)polys.size(), [&](int b) { return (const RMatT *)polys[(size_t)b]; }, detail::shape_as_is());
    empty.assign(polys.size(), 0);
    return xpg_dep_is_empty_batch_ragged_rat32(detail::ctx_or_shared(c), (int)polys.size(), p.flat.data(), p.rows.data(), p.cols.data(), p.off.data(),
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
    const auto rows_of = [](const RMatT * m) { return m && m->get_col_size() ? (int)m->get_row_size() : 0; };
    const auto shape_of = [&](const RMatT * m) { return std::make_pair(rows_of(m), m ? (int)m->get_col_size() : 0); };
    for (int b = 0; b < nb; b++)
        for (const RMatT * m : { (const RMatT *)leqs[(size_t)b], (const RMatT *)eqs[(size_t)b] })
            if (rows_of(m) > 0 && (int)m->get_col_size() != cols) return XPG_ERR_SHAPE;
    const detail::packed L = detail::pack(nb, [&](int b) { return (const RMatT *)leqs[(size_t)b]; }, shape_of),
                         E = detail::pack(nb, [&](int b) { return (const RMatT *)eqs[(size_t)b]; }, shape_of);
    const xpg_rat32 * const l = L.cells() ? L.flat.data() : (const xpg_rat32 *)0, * const e = E.cells() ? E.flat.data() : (const xpg_rat32 *)0;
    if (is_int_sol)      // the integer form on the device: objective, both walks and the verdict, one synchronisation per shape class
        return xpg_has_solution_int_batch_ragged_rat32(detail::ctx_or_shared(c), nb, l, L.rows.data(), L.off.data(), e, E.rows.data(), E.off.data(),
                                                       (const xpg_rat32 *)vc.get_matrix(), rhs_idx, cols, rhs_idx, is_unique_sol ? 1 : 0, out.data(),
                                                       (int32_t *)0);
    return xpg_has_solution_batch_ragged_rat32(detail::ctx_or_shared(c), nb, l, L.rows.data(), L.off.data(), e, E.rows.data(), E.off.data(),
                                               (const xpg_rat32 *)vc.get_matrix(), rhs_idx, cols, rhs_idx, 0, is_unique_sol ? 1 : 0, 0xFFFFFFFFu,
                                               out.data(), (int32_t *)0);
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
    const std::vector<int> live = detail::live_systems(systems, [&](int b) { results[(size_t)b].clean(); ok[(size_t)b] = 1; });
    const int nl = (int)live.size();
    if (nl == 0) return 0;
    const detail::packed p = detail::pack(systems, live, detail::shape_as_is());
    std::vector<int32_t> uu((size_t)nl), rr((size_t)nl), orows((size_t)nl), ook((size_t)nl);
    std::vector<long long> ooff((size_t)nl + 1, 0);
    long long capc = 0;                                             // the worst case of every result, in cells
    for (int k = 0; k < nl; k++) {
        uu[(size_t)k] = u[(size_t)live[(size_t)k]];
        rr[(size_t)k] = rhs_idx.empty() ? p.cols[(size_t)k] - 1 : rhs_idx[(size_t)live[(size_t)k]];
        capc += ((long long)p.rows[(size_t)k] * p.rows[(size_t)k] / 4 + p.rows[(size_t)k]) * p.cols[(size_t)k];
    }
    xpg_ctx * h = detail::ctx_or_shared(c);
    std::vector<xpg_rat32> outs;
    const auto call = [&](long long room) {
        outs.resize((size_t)(room > 0 ? room : 1));
        return xpg_lineq_fme_batch_ragged_rat32(h, nl, p.flat.data(), p.rows.data(), p.cols.data(), p.off.data(), rr.data(), uu.data(), darkshadow ? 1 : 0,
                                                room < 0 ? (xpg_rat32 *)0 : outs.data(), room < 0 ? 0 : room, ooff.data(), orows.data(), ook.data());
    };
    // a buffer for the worst case of every result while that is small (one call), else a sizing call (no buffer) first
    int rc;
    if (capc * (long long)sizeof(xpg_rat32) <= (64ll << 20)) rc = call(capc);
    else {
        rc = call(-1);
        if (rc == XPG_ERR_SHAPE && ooff[(size_t)nl] > 0) rc = call(ooff[(size_t)nl]);
    }
    if (rc != 0) return rc;
    for (int k = 0; k < nl; k++) {
        detail::put_cells(results[(size_t)live[(size_t)k]], outs.data() + ooff[(size_t)k], orows[(size_t)k], p.cols[(size_t)k]);
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
    xpg_ctx * h = detail::ctx_or_shared(c);
    // an empty system stays empty (linsys.cpp:661-664), no call
    const std::vector<int> live = detail::live_systems(systems, [&](int b) { results[(size_t)b].clean(); ok[(size_t)b] = 1; });
    return detail::for_each_class(live, [&](int b) { return detail::shape_of(systems, b); }, [&](const std::vector<int> & cls) {
        const int nc = (int)cls.size();
        const int rows = (int)systems[(size_t)cls[0]]->get_row_size(), cols = (int)systems[(size_t)cls[0]]->get_col_size();
        const detail::shape_known shape = { rows, cols };
        const detail::packed p = detail::pack(systems, cls, shape);
        const detail::retry_rule how = { { 0, 0, 0 }, { 0, 0, 0 }, detail::one_capacity, false, 3 };   // the library's default first; the final slots take cap too
        return detail::call_until_answered(how, (size_t)nc, (size_t)nc,
            [&](const detail::caps & cp, detail::answer & a) {
                return xpg_lineq_project_batch_packed_rat32(h, nc, p.flat.data(), rows, cols, rhs_idx, elim.data(), (int)elim.size(), darkshadow ? 1 : 0,
                                                            cp.cap, cp.out, (xpg_rat32 *)0, 0, &a.view, a.off, a.ok, a.steps);
            },
            [&](const detail::answer & a) {
                for (int k = 0; k < nc; k++) {
                    ok[(size_t)cls[(size_t)k]] = a.ok[(size_t)k];
                    a.put_packed(results[(size_t)cls[(size_t)k]], (size_t)k, cols);
                }
            });
    });
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
    xpg_ctx * h = detail::ctx_or_shared(c);
    // an empty system stays empty (linsys.cpp:661-664), no call
    const std::vector<int> live = detail::live_systems(systems, [&](int b) {
        levels[(size_t)b].resize((size_t)n);
        for (int k = 0; k < n; k++) levels[(size_t)b][(size_t)k].clean();
        ok[(size_t)b] = 1;
    });
    return detail::for_each_class(live, [&](int b) { return detail::shape_of(systems, b); }, [&](const std::vector<int> & cls) {
        const int nc = (int)cls.size();
        const int rows = (int)systems[(size_t)cls[0]]->get_row_size(), cols = (int)systems[(size_t)cls[0]]->get_col_size(), cap = detail::chain_default(rows);
        const detail::shape_known shape = { rows, cols };
        const detail::packed p = detail::pack(systems, cls, shape);
        const detail::retry_rule how = { { cap, cap < detail::bound_default(rows) ? cap : detail::bound_default(rows), 0 }, { 0, 0, 0 },   // the library's defaults, spelled out
                                         detail::own_slot, false, 4 };
        return detail::call_until_answered(how, (size_t)nc, (size_t)nc * n,
            [&](const detail::caps & cp, detail::answer & a) {
                return xpg_lineq_levels_batch_packed_rat32(h, nc, p.flat.data(), rows, cols, rhs_idx, elim.data(), n, darkshadow ? 1 : 0, cp.cap, cp.out,
                                                           (xpg_rat32 *)0, 0, &a.view, a.off, a.ok, a.steps);
            },
            [&](const detail::answer & a) {
                for (int k = 0; k < nc; k++) {
                    std::vector<RMatT> & lev = levels[(size_t)cls[(size_t)k]];
                    ok[(size_t)cls[(size_t)k]] = a.ok[(size_t)k];
                    lev.resize((size_t)n);
                    for (int j = 0; j < n; j++) a.put_packed(lev[(size_t)j], (size_t)k * n + j, cols);
                }
            });
    });
}

namespace detail {
// What project_each and levels_nests share: the systems that travel (`live`: indices into `systems`, each with its list in
// `lists`) go up in ONE xpg_lineq_{project,levels}_batch_ragged_rat32 call whatever their shapes and lists; a call found
// short of rows is made again with the largest need reported -- above the capacity tried: a step's unreduced rows, cap_rows;
// else an output slot, cap_out_rows -- at most four times, then XPG_ERR_UNSUPPORTED. sink(i, k, answer, r, cols) receives
// result k of live system i (k == 0 alone for a projection), result r of the answer, once every answer is there;
// ok[live[i]] the verdict (1, or 0: a step found the system inconsistent, every result of it empty).
template <class RMatT, class Sink>
inline int chain_ragged(bool levels, const std::vector<RMatT *> & systems, const std::vector<int> & live, const std::vector<std::vector<int32_t> > & lists,
                        const std::vector<int32_t> & rhs_idx, std::vector<int32_t> & ok, xpg_ctx * h, bool darkshadow, Sink sink)
{
    const int nl = (int)live.size();
    if (nl == 0) return 0;
    const packed p = pack(systems, live, shape_as_is());
    std::vector<int32_t> rr((size_t)nl), eoff((size_t)nl + 1, 0), flat_el;
    for (int i = 0; i < nl; i++) {
        rr[(size_t)i] = rhs_idx[(size_t)live[(size_t)i]];
        flat_el.insert(flat_el.end(), lists[(size_t)i].begin(), lists[(size_t)i].end());
        eoff[(size_t)i + 1] = (int32_t)flat_el.size();
    }
    const int nres = levels ? (int)flat_el.size() : nl, cap = chain_default(p.most);
    // the library's defaults first, then the capacities that call settled on (xpoly_amd.h); a projection's final slot takes cap
    const retry_rule how = { { 0, 0, 0 }, { cap, levels && bound_default(p.most) < cap ? bound_default(p.most) : cap, 0 }, levels ? own_slot : slot_is_cap, false, 4 };
    return call_until_answered(how, (size_t)nl, (size_t)nres,
        [&](const caps & cp, answer & a) {
            return (levels ? xpg_lineq_levels_batch_ragged_rat32 : xpg_lineq_project_batch_ragged_rat32)(
                h, nl, p.flat.data(), p.rows.data(), p.cols.data(), p.off.data(), rr.data(), flat_el.data(), eoff.data(), darkshadow ? 1 : 0, cp.cap, cp.out,
                (xpg_rat32 *)0, 0, &a.view, a.off, a.rows, a.ok, a.steps);
        },
        [&](const answer & a) {
            for (int i = 0; i < nl; i++) {
                ok[(size_t)live[(size_t)i]] = a.ok[(size_t)i];
                const int first = levels ? eoff[(size_t)i] : i, n = levels ? eoff[(size_t)i + 1] - eoff[(size_t)i] : 1;
                for (int k = 0; k < n; k++) sink(i, k, a, (size_t)(first + k), (int)p.cols[(size_t)i]);
            }
        });
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
    return detail::chain_ragged(false, systems, live, lists, rhs_idx, ok, detail::ctx_or_shared(c), darkshadow,
                                [&](int i, int, const detail::answer & a, size_t r, int cc) { a.put_ragged(results[(size_t)live[(size_t)i]], r, cc); });
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
    return detail::chain_ragged(true, systems, live, lists, rhs_idx, ok, detail::ctx_or_shared(c), darkshadow,
                                [&](int i, int k, const detail::answer & a, size_t r, int cc) { a.put_ragged(levels[(size_t)live[(size_t)i]][(size_t)k], r, cc); });
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
    xpg_ctx * h = detail::ctx_or_shared(c);
    std::vector<int> all((size_t)nb);
    for (int b = 0; b < nb; b++) all[(size_t)b] = b;
    return detail::for_each_class(all, [&](int b) { return detail::shape_of(systems, b, rhs_idx[(size_t)b]); }, [&](const std::vector<int> & cls) {
        const int nc = (int)cls.size(), nv = rhs_idx[(size_t)cls[0]];
        const int rows = (int)systems[(size_t)cls[0]]->get_row_size(), cols = (int)systems[(size_t)cls[0]]->get_col_size();
        if (rows == 0 || cols == 0 || nv < 1 || nv >= cols) return (int)XPG_ERR_SHAPE;
        const detail::shape_known shape = { rows, cols };
        const detail::packed p = detail::pack(systems, cls, shape);
        const detail::retry_rule how = { { detail::bound_default(rows), 0, 0 }, { 0, 0, 0 }, detail::one_capacity, false, 3 };
        return detail::call_until_answered(how, (size_t)nc, (size_t)nc * nv,
            [&](const detail::caps & cp, detail::answer & a) {
                return xpg_lineq_bounds_batch_packed_rat32(h, nc, p.flat.data(), rows, cols, nv, cp.cap, cp.out, (xpg_rat32 *)0, 0, &a.view, a.off,
                                                           a.ok, a.chain, a.steps);
            },
            [&](const detail::answer & a) {
                for (int k = 0; k < nc; k++) {
                    std::vector<RMatT> & lim = limits[(size_t)cls[(size_t)k]];
                    ok[(size_t)cls[(size_t)k]] = a.ok[(size_t)k];
                    lim.resize((size_t)nv);
                    for (int j = 0; j < nv; j++) a.put_packed(lim[(size_t)j], (size_t)k * nv + j, cols);
                }
            });
    });
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
    xpg_ctx * h = detail::ctx_or_shared(c);
    const detail::packed p = detail::pack(nb, [&](int b) { return (const RMatT *)systems[(size_t)b]; }, detail::shape_as_is());
    std::vector<int> first((size_t)nb + 1, 0);
    for (int b = 0; b < nb; b++) {
        const int nv = rhs_idx[(size_t)b];
        if (p.rows[(size_t)b] == 0 || p.cols[(size_t)b] == 0 || nv < 1 || nv >= p.cols[(size_t)b]) return XPG_ERR_SHAPE;
        first[(size_t)b + 1] = first[(size_t)b] + nv;
    }
    const int nres = first[(size_t)nb], cap = detail::bound_default(p.most);
    const detail::retry_rule how = { { cap, cap, 0 }, { 0, 0, 0 }, detail::slot_follows, false, 3 };   // the library's defaults, spelled out; a result's slot takes cap, as in calc_bound_all
    return detail::call_until_answered(how, (size_t)nb, (size_t)nres,
        [&](const detail::caps & cp, detail::answer & a) {
            return xpg_lineq_bounds_batch_ragged_rat32(h, nb, p.flat.data(), p.rows.data(), p.cols.data(), p.off.data(), rhs_idx.data(), cp.cap, cp.out,
                                                       (xpg_rat32 *)0, 0, &a.view, a.off, a.rows, a.ok, a.chain, a.steps);
        },
        [&](const detail::answer & a) {
            for (int b = 0; b < nb; b++) {
                const int nv = rhs_idx[(size_t)b];
                ok[(size_t)b] = a.ok[(size_t)b];
                limits[(size_t)b].resize((size_t)nv);
                for (int j = 0; j < nv; j++) a.put_ragged(limits[(size_t)b][(size_t)j], (size_t)(first[(size_t)b] + j), (int)p.cols[(size_t)b]);
            }
        });
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
    xpg_ctx * h = ctx_or_shared(c);
    std::vector<const RMatT *> all;                                 // the members of every group, in group order
    std::vector<int32_t> goff((size_t)ng + 1, 0), rhs, elim, eoff(1, 0);
    for (int g = 0; g < ng; g++) {
        const std::vector<RMatT *> & grp = groups[(size_t)g];
        if (elims && (*elims)[(size_t)g].size() != grp.size()) return XPG_ERR_SHAPE;
        for (size_t i = 0; i < grp.size(); i++) {
            if (grp[i]->get_row_size() == 0 || grp[i]->get_col_size() == 0) return XPG_ERR_SHAPE;
            all.push_back(grp[i]); rhs.push_back(rhs_idx[(size_t)g]);
            if (elims) {
                const std::vector<int32_t> & e = (*elims)[(size_t)g][i];
                elim.insert(elim.end(), e.begin(), e.end());
                eoff.push_back((int32_t)elim.size());
            }
        }
        goff[(size_t)g + 1] = goff[(size_t)g] + (int32_t)grp.size();
    }
    const int nb = goff[(size_t)ng];
    const packed p = pack(nb, [&](int b) { return all[(size_t)b]; }, shape_as_is());
    if (elim.empty()) elim.push_back(0);
    const int cap = elims ? chain_default(p.most) : bound_default(p.most);
    const retry_rule how = { { cap, cap, 0 }, { 0, 0, 0 }, slot_follows, true, 3 };   // the library's defaults, spelled out
    return call_until_answered(how, (size_t)ng, (size_t)ng,
        [&](const caps & cp, answer & a) {
            return elims
                ? xpg_lineq_project_union_batch_ragged_rat32(h, ng, goff.data(), nb, p.flat.data(), p.rows.data(), p.cols.data(), p.off.data(), rhs.data(),
                                                             elim.data(), eoff.data(), darkshadow ? 1 : 0, is_intersect ? 1 : 0, cp.cap, cp.out, cp.hull,
                                                             (xpg_rat32 *)0, 0, &a.view, a.off, a.rows, a.ok, a.member,
                                                             a.chain, a.steps)
                : xpg_lineq_hull_batch_ragged_rat32(h, ng, goff.data(), nb, p.flat.data(), p.rows.data(), p.cols.data(), p.off.data(), rhs.data(),
                                                    is_intersect ? 1 : 0, cp.cap, cp.out, cp.hull, (xpg_rat32 *)0, 0, &a.view, a.off, a.rows,
                                                    a.ok, a.member, a.chain, a.steps);
        },
        [&](const answer & a) {
            for (int g = 0; g < ng; g++) {
                ok[(size_t)g] = a.ok[(size_t)g];
                if (member) (*member)[(size_t)g] = a.member[(size_t)g];
                if (a.rows[(size_t)g] > 0) a.put_ragged(results[(size_t)g], (size_t)g, (int)p.cols[(size_t)goff[(size_t)g]]);
                else results[(size_t)g].clean();
            }
        });
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

// ---- limits of TRANSFORMED loop nests: LoopTran::transformIterSpace (src/eng/ldtran.cpp:131-300) ---------------------------------
// What one transformation of a nest comes back as: the verdicts of xpg_lineq_transform_levels_batch_packed_rat32, the
// determinant (mode 0), invt (the multiplier; empty for kind 1 and 2) and the levels -- levels[0] the transformed nest (A * invt
// | C), levels[k] that system with rhs_idx-1 .. rhs_idx-k eliminated; all empty for kind 1 / 2 or ok <= 0.
template <class RMatT> struct transformed_nest {
    int32_t ok, steps, kind; xpg_rat32 det; RMatT invt; std::vector<RMatT> levels;
};
namespace detail {
// The one call behind LoopTran and transform_levels_all: nb transformations tm [nb][nv][nv] against nests [nb][rows][cols] or
// (shared) ONE nest, retried on -need as levels_all retries. sink(answer, kind, det, mult) once every answer is there.
template <class Sink>
inline int transform_call(xpg_ctx * h, int nb, const xpg_rat32 * nests, bool shared, const xpg_rat32 * tm, int rows, int cols, int nv, int mode,
                          Sink sink)
{
    const int cap = chain_default(rows);
    const retry_rule how = { { cap, cap < bound_default(rows) ? cap : bound_default(rows), 0 }, { 0, 0, 0 }, own_slot, false, 4 };
    std::vector<int32_t> kind((size_t)nb);
    std::vector<xpg_rat32> det((size_t)nb), mult((size_t)nb * nv * nv);
    return call_until_answered(how, (size_t)nb, (size_t)nb * nv,
        [&](const caps & cp, answer & a) {
            return xpg_lineq_transform_levels_batch_packed_rat32(h, nb, nests, shared ? 1 : 0, tm, rows, cols, nv, mode, cp.cap, cp.out, (xpg_rat32 *)0, 0,
                                                                 &a.view, a.off, a.ok, a.steps, kind.data(), det.data(), mult.data());
        },
        [&](const answer & a) { sink(a, kind.data(), det.data(), mult.data()); });
}
template <class RMatT>
inline int transform_levels_some(const std::vector<const RMatT *> & nests, bool shared, const std::vector<RMatT *> & ts, int rhs_idx, int mode,
                                 std::vector<transformed_nest<RMatT> > & out, xpg_ctx * c)
{
    const int nb = (int)ts.size(), nv = rhs_idx;
    out.clear();
    if (nb == 0) return 0;
    if (nests.empty() || (!shared && (int)nests.size() != nb) || nests[0]->size() == 0 || nv < 1) return XPG_ERR_SHAPE;
    const int rows = (int)nests[0]->get_row_size(), cols = (int)nests[0]->get_col_size();
    for (size_t k = 0; k < nests.size(); k++)
        if (nests[k]->size() == 0 || (int)nests[k]->get_row_size() != rows || (int)nests[k]->get_col_size() != cols) return XPG_ERR_SHAPE;
    for (int b = 0; b < nb; b++)
        if ((int)ts[(size_t)b]->get_row_size() != nv || (int)ts[(size_t)b]->get_col_size() != nv) return XPG_ERR_SHAPE;
    const shape_known nshape = { rows, cols }, tshape = { nv, nv };
    const packed pn = pack((int)nests.size(), [&](int i) { return nests[(size_t)i]; }, nshape);
    const packed pt = pack(nb, [&](int i) { return (const RMatT *)ts[(size_t)i]; }, tshape);
    out.resize((size_t)nb);
    return transform_call(ctx_or_shared(c), nb, pn.flat.data(), shared, pt.flat.data(), rows, cols, nv, mode,
        [&](const answer & a, const int32_t * kind, const xpg_rat32 * det, const xpg_rat32 * mult) {
            for (int b = 0; b < nb; b++) {
                transformed_nest<RMatT> & o = out[(size_t)b];
                o.ok = a.ok[(size_t)b]; o.steps = a.steps[(size_t)b]; o.kind = kind[(size_t)b]; o.det = det[(size_t)b];
                if (o.kind == 0) put_cells(o.invt, mult + (size_t)b * nv * nv, nv, nv);
                o.levels.resize((size_t)nv);
                for (int k = 0; k < nv; k++) a.put_packed(o.levels[(size_t)k], (size_t)b * nv + k, cols);
            }
        });
}
}
// The search over transformations: ONE nest against many T in one shared-nest call -- per T the kind, the determinant, invt
// and the levels (transformed_nest). mode 1: the ts are the right multipliers themselves. Returns 0 or a negative XPG_ERR_* code.
template <class RMatT>
inline int transform_levels_all(const RMatT & nest, const std::vector<RMatT *> & ts, int rhs_idx, std::vector<transformed_nest<RMatT> > & out,
                                xpg_ctx * c = 0, int mode = 0)
{
    return detail::transform_levels_some(std::vector<const RMatT *>(1, &nest), true, ts, rhs_idx, mode, out, c);
}
// The same with one nest per T, all of one shape.
template <class RMatT>
inline int transform_levels_all(const std::vector<RMatT *> & nests, const std::vector<RMatT *> & ts, int rhs_idx,
                                std::vector<transformed_nest<RMatT> > & out, xpg_ctx * c = 0, int mode = 0)
{
    return detail::transform_levels_some(std::vector<const RMatT *>(nests.begin(), nests.end()), false, ts, rhs_idx, mode, out, c);
}

// A class with the reference's LoopTran constructor and transformIterSpace signature (src/eng/ldtran.h:50-103), so that
//     LoopTran lt(&A, rhs_idx);  bool uni = lt.transformIterSpace(t, stride, idx_map, aux_limits, ofst, mul, &trA);
// compiles against xpoly_amd::LoopTran<RMat>. Beyond lineq.hpp's matrix contract it relies on RMat's own operator* and
// assignment (matt.h:60-79), as the reference does for idx_map * invt and Ui * Hi.
//   t unimodular: ONE mode 0 call -- det, T^-1, A * T^-1 and every level on the device. stride is a row of ones, ofst and mul
//     are emptied, aux_limits is filled tail to head (the tail the transformed nest), trA receives the tail. Returns true.
//   t nonsingular, not unimodular (that call answers kind 2): the reference's second branch (:203-291) -- hnf through
//     xpg_int_hnf_batch, H^-1 through xpg_rat_inv_batch, ONE mode 1 call with Ui; stride = mul = diag(H), invt = Ui * Hi, and
//     ofst = (the strictly lower part of H) * Hi, whose row i is the reference's sum of H(i,j) * Hi[j] over j < i (:271-289; the
//     product also adds the zero terms, which leaves a canonical cell as it is). Returns false, status() == 0.
//   t singular, an inconsistent nest (the reference ASSERTs at both) or a failed call: returns false with every argument left
//     as it was and status() != 0 -- 1: t is singular, 2: "system inconsistency!", 3: H of the hnf has no inverse, else the
//     negative XPG_ERR_* code (XPG_ERR_REF_UNDEFINED where INTMat::hnf itself is undefined for t, xpg_int_hnf_batch).
//   idx_map = idx_map * invt, or invt where idx_map is empty (:293-298).
template <class RMatT> class LoopTran {
    xpg_ctx * m_ctx;
    RMatT * m_a;
    int m_rhs_idx, m_status;
    static void put_ints(RMatT & m, const int32_t * v, int rows, int cols, bool lower_only = false)
    {
        std::vector<xpg_rat32> cells((size_t)rows * cols);
        for (int i = 0; i < rows; i++)
            for (int j = 0; j < cols; j++) { cells[(size_t)i * cols + j].num = lower_only && j >= i ? 0 : v[(size_t)i * cols + j]; cells[(size_t)i * cols + j].den = 1; }
        detail::put_cells(m, cells.data(), rows, cols);
    }
public:
    explicit LoopTran(RMatT * m, int rhs_idx = -1, xpg_ctx * c = 0) : m_ctx(c), m_a(0), m_rhs_idx(-1), m_status(0) { if (m) set_param(m, rhs_idx); }
    void set_param(RMatT * m, int rhs_idx = -1) { m_a = m; m_rhs_idx = rhs_idx == -1 ? (int)m->get_col_size() - 1 : rhs_idx; }   // ldtran.cpp:51-62
    int status() const { return m_status; }
    template <class ListT, class = decltype(std::declval<ListT &>().get_tail()), class = decltype(std::declval<ListT &>().get_prev()),
              class = decltype(std::declval<ListT &>().get_elem_count())>
    bool transformIterSpace(RMatT & t, RMatT & stride, RMatT & idx_map, ListT & aux_limits, RMatT & ofst, RMatT & mul, RMatT * trA = 0)
    {
        const int nv = m_rhs_idx;
        m_status = XPG_ERR_SHAPE;
        if (!m_a || m_a->size() == 0 || nv < 1 || nv >= (int)m_a->get_col_size() || (int)aux_limits.get_elem_count() != nv ||
            (int)t.get_row_size() != nv || (int)t.get_col_size() != nv)
            return false;                                               // the reference ASSERTs (:139-140, :151)
        std::vector<RMatT *> dst;                                       // the tail first; none of them is the nest itself
        for (RMatT * newb = aux_limits.get_tail(); (int)dst.size() < nv; newb = aux_limits.get_prev()) {
            if (!newb || newb == m_a) return false;
            dst.push_back(newb);
        }
        xpg_ctx * h = detail::ctx_or_shared(m_ctx);
        const int rows = (int)m_a->get_row_size(), cols = (int)m_a->get_col_size();
        const xpg_rat32 * in = (const xpg_rat32 *)m_a->get_matrix();
        int kind = 0, ok = 0;
        std::vector<RMatT> got((size_t)nv);
        RMatT invt;
        const auto keep = [&](const detail::answer & a, const int32_t * k, const xpg_rat32 *, const xpg_rat32 * mult) {
            kind = k[0]; ok = a.ok[0];
            if (kind != 0 || ok != 1) return;
            detail::put_cells(invt, mult, nv, nv);
            for (int j = 0; j < nv; j++) a.put_packed(got[(size_t)j], (size_t)j, cols);
        };
        int rc = detail::transform_call(h, 1, in, true, (const xpg_rat32 *)t.get_matrix(), rows, cols, nv, 0, keep);
        if (rc != 0) { m_status = rc; return false; }
        if (kind == 1) { m_status = 1; return false; }                  // "T is singular!!" (:149)
        const bool is_uni = kind == 0;
        std::vector<int32_t> hm((size_t)nv * nv), um((size_t)nv * nv);
        RMatT Hi;
        if (!is_uni) {
            std::vector<int32_t> it((size_t)nv * nv);
            const xpg_rat32 * tc = (const xpg_rat32 *)t.get_matrix();
            for (size_t x = 0; x < it.size(); x++) it[x] = tc[x].den ? tc[x].num / tc[x].den : 0;    // it.copy(t) (:207)
            int32_t st = 0, inv_ok = 0;
            rc = xpg_int_hnf_batch(h, 1, it.data(), nv, nv, hm.data(), um.data(), &st);               // tmph = it * tmpu (:208)
            if (rc != 0 || st != 0) { m_status = rc ? rc : st; return false; }
            RMatT H, Ui;
            put_ints(H, hm.data(), nv, nv); put_ints(Ui, um.data(), nv, nv);
            std::vector<xpg_rat32> hi((size_t)nv * nv);
            rc = xpg_rat_inv_batch(h, 1, (const xpg_rat32 *)H.get_matrix(), nv, hi.data(), &inv_ok);  // H.inv(Hi) (:223)
            if (rc != 0 || !inv_ok) { m_status = rc ? rc : 3; return false; }
            detail::put_cells(Hi, hi.data(), nv, nv);
            rc = detail::transform_call(h, 1, in, true, (const xpg_rat32 *)Ui.get_matrix(), rows, cols, nv, 1, keep);   // A * Ui (:233-235)
            if (rc != 0) { m_status = rc; return false; }
            invt = Ui * Hi;                                             // (:224)
        }
        if (ok != 1) { m_status = ok == 0 ? 2 : XPG_ERR_UNSUPPORTED; return false; }      // "system inconsistency!" (:186-188, :249-251)
        m_status = 0;
        for (int j = 0; j < nv; j++) *dst[(size_t)j] = got[(size_t)j];
        if (trA) *trA = got[0];                                         // (:197-200, :258-261)
        if (is_uni) {
            std::vector<int32_t> ones((size_t)nv, 1);
            put_ints(stride, ones.data(), 1, nv);                       // (:167-170)
            ofst.reinit(0, 0); mul.reinit(0, 0);                        // (:154-155)
        } else {
            std::vector<int32_t> diag((size_t)nv);
            for (int i = 0; i < nv; i++) diag[(size_t)i] = hm[(size_t)i * nv + i];
            put_ints(stride, diag.data(), 1, nv); put_ints(mul, diag.data(), 1, nv);     // H.getdiag(stride); mul.copy(stride) (:221-222)
            RMatT lower;
            put_ints(lower, hm.data(), nv, nv, true);
            ofst = lower * Hi;                                          // (:271-289)
        }
        if (idx_map.size() > 0) idx_map = idx_map * invt; else idx_map = invt;           // (:293-298)
        return is_uni;
    }
};

} // namespace xpoly_amd
#endif
