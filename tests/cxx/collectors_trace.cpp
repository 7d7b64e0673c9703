// What the collectors of include/xpoly_amd/lineq.hpp do, seen from BELOW: this program defines xpg_create and every xpg_* entry
// point the header calls itself and is linked WITHOUT the library, so no device is needed. Each stand-in
//   - prints one line per call: its name, the handle (shared / own), nb, every shape, offset, rhs_idx, list and capacity argument,
//     whether outs / out_view were given, and a checksum of the packed cells;
//   - fills its outputs with cells that name their origin: num = ((call * 100 + system) * 100 + result) * 100 + row, den = column + 1,
//     result k of system b with (b + 2 k + 1) % 4 rows (none where the verdict is not 1, none for the system named by g_zero);
//   - answers from the script the scenario set: per call a return code and, per system (group), a verdict -- 1, 0 or -need -- and a
//     member; a call beyond the script is answered 1 throughout.
// After each collector returns the program prints its return code, ok[] and member[], and rows x cols and a checksum of every
// result matrix (0x4 and 0x0 are different states). Every scenario ends with "calls <n>". tests/test_lineq_collectors_host.py
// compiles it under the sanitizers, runs it and compares the output with tests/golden/g15_collectors_trace.txt line for line.
//   collectors_trace          the trace
//   collectors_trace --time [NAME]   median microseconds per collector call on a SCoP-sized batch -- 692 systems over the 20 shape classes
//                             of the mixed SCoP (triangular nests of depth 2 .. 6 with 0 .. 3 further bounds, system b of class
//                             (7 b) % 20) -- with printing and stamping off: the host time spent inside the header
#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "xpoly_amd/lineq.hpp"

struct StubMat {
    unsigned rows, cols;
    std::vector<xpg_rat32> cells;
    StubMat() : rows(0), cols(0) {}
    StubMat(unsigned r, unsigned c, int seed) : rows(0), cols(0)
    {
        reinit(r, c);
        for (unsigned i = 0; i < r; i++) for (unsigned j = 0; j < c; j++) { cells[(size_t)i * c + j].num = seed * 100 + (int)i * 10 + (int)j; cells[(size_t)i * c + j].den = 1; }
    }
    unsigned get_row_size() const { return rows; }
    unsigned get_col_size() const { return cols; }
    unsigned size() const { return rows * cols; }
    const xpg_rat32 * get_matrix() const { return cells.data(); }
    void reinit(unsigned r, unsigned c) { rows = r; cols = c; xpg_rat32 z; z.num = 0; z.den = 1; cells.assign((size_t)r * c, z); }
    void clean() { rows = 0; cols = 0; cells.clear(); }
};
// what the reference's List<RMat*> offers the members
struct StubList {
    std::vector<StubMat *> v; size_t at;
    StubList() : at(0) {}
    StubMat * get_head() { at = 0; return v.empty() ? 0 : v[0]; }
    StubMat * get_next() { return ++at < v.size() ? v[at] : 0; }
    StubMat * get_tail() { at = v.size() - 1; return v.empty() ? 0 : v[at]; }
    StubMat * get_prev() { return at > 0 ? v[--at] : 0; }
    StubMat * get_head_nth(unsigned n) { return n < v.size() ? v[n] : 0; }
    unsigned get_elem_count() const { return (unsigned)v.size(); }
};
typedef xpoly_amd::Lineq<StubMat> Lin;
typedef std::vector<int32_t> I32;

// ---------------------------------------------------------------- the script and the stand-ins' shared parts
struct Step { int rc; std::map<int, int> ok, mem; };
static std::vector<Step> g_script;
static int g_call = 0, g_zero = -1;
static bool g_quiet = false;
static std::vector<xpg_rat32> g_view;
static int g_own_ctx, g_shared_ctx;

static Step S(int rc, std::map<int, int> ok = std::map<int, int>(), std::map<int, int> mem = std::map<int, int>())
{ Step s; s.rc = rc; s.ok = ok; s.mem = mem; return s; }
static const Step * step_of(int call) { return call < (int)g_script.size() ? &g_script[(size_t)call] : (const Step *)0; }
static int rc_of(int call) { const Step * s = step_of(call); return s ? s->rc : 0; }
static int verdict(int call, int sys)
{
    const Step * s = step_of(call);
    if (!s) return 1;
    std::map<int, int>::const_iterator it = s->ok.find(sys);
    return it == s->ok.end() ? 1 : it->second;
}
static int member_of(int call, int sys)
{
    const Step * s = step_of(call);
    if (!s) return -1;
    std::map<int, int>::const_iterator it = s->mem.find(sys);
    return it == s->mem.end() ? -1 : it->second;
}
static void say(const char * fmt, ...)
{
    if (g_quiet) return;
    va_list ap; va_start(ap, fmt); vprintf(fmt, ap); va_end(ap);
}
template <class T> static void arr(const char * key, const T * a, long long n)
{
    if (g_quiet) return;
    if (!a) { printf(" %s=null", key); return; }
    printf(" %s=[", key);
    for (long long i = 0; i < n; i++) printf(i ? ",%lld" : "%lld", (long long)a[i]);
    printf("]");
}
static unsigned sum(const xpg_rat32 * a, long long n)
{
    unsigned h = 2166136261u;
    for (long long i = 0; a && i < n; i++) { h = (h ^ (unsigned)a[i].num) * 16777619u; h = (h ^ (unsigned)a[i].den) * 16777619u; }
    return h;
}
static void cells(const char * key, const xpg_rat32 * a, long long n)
{
    if (g_quiet) return;
    if (!a || n == 0) printf(" %s=none", key); else printf(" %s=%lld:%08x", key, n, sum(a, n));
}
static int begin(const char * name, xpg_ctx * ctx)
{
    const int call = g_call++;
    say("  call %d %s ctx=%s", call, name, ctx == (xpg_ctx *)&g_shared_ctx ? "shared" : ctx == (xpg_ctx *)&g_own_ctx ? "own" : ctx ? "other" : "null");
    return call;
}
static int end(int rc) { say(" -> %d\n", rc); return rc; }
static int rows_of_result(int sys, int res, int ok) { return ok != 1 || sys == g_zero ? 0 : (sys + 2 * res + 1) % 4; }
static void stamp(xpg_rat32 * at, int call, int sys, int res, int rows, int cols)
{
    for (int i = 0; i < rows; i++)
        for (int j = 0; j < cols; j++) { at[(size_t)i * cols + j].num = ((call * 100 + sys) * 100 + res) * 100 + i; at[(size_t)i * cols + j].den = j + 1; }
}
// lays the results of a call out back to back: nres(b) results of cols(b) columns for system b; cell_off[total + 1], rows[total]
// (may be null). Into `into` where given (room asserted by the caller), else into the stand-in's own buffer. Returns the base.
template <class NRes, class Cols>
static xpg_rat32 * lay(int call, int nb, NRes nres, Cols cols, const int32_t * ok, long long * cell_off, int32_t * rows, xpg_rat32 * into = 0)
{
    long long total = 0;
    for (int b = 0; b < nb; b++) for (int k = 0; k < nres(b); k++) total += (long long)rows_of_result(b, k, ok[b]) * cols(b);   // (no columns: no rows)
    if (!into) { if ((long long)g_view.size() < total + 1) g_view.resize((size_t)total + 1); into = g_view.data(); }
    long long at = 0;
    int r = 0;
    for (int b = 0; b < nb; b++)
        for (int k = 0; k < nres(b); k++, r++) {
            const int n = cols(b) ? rows_of_result(b, k, ok[b]) : 0;
            cell_off[r] = at;
            if (rows) rows[r] = n;
            if (!g_quiet) stamp(into + at, call, b, k, n, cols(b));
            at += (long long)n * cols(b);
        }
    cell_off[r] = at;
    return into;
}
struct Const { int v; int operator()(int) const { return v; } };
struct From { const int32_t * a; int operator()(int b) const { return a[b]; } };
struct Span { const int32_t * off; int operator()(int b) const { return off[b + 1] - off[b]; } };

// the packed chain forms: nb systems of one shape, nres results each, offsets in ROWS
static int packed_chain(int call, int nb, int cols, int nres, const xpg_rat32 ** out_view, long long * row_offsets, int32_t * out_ok)
{
    const int rc = rc_of(call);
    if (rc != 0) return rc;
    for (int b = 0; b < nb; b++) out_ok[b] = verdict(call, b);
    Const n = { nres }, c = { cols };
    const xpg_rat32 * v = lay(call, nb, n, c, out_ok, row_offsets, (int32_t *)0);
    for (long long r = 0; r <= (long long)nb * nres; r++) row_offsets[r] /= cols;
    if (out_view) *out_view = v;
    return 0;
}

extern "C" {
int xpg_create(xpg_ctx ** out, int) { *out = (xpg_ctx *)&g_shared_ctx; return 0; }

int xpg_lineq_reduce_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols, int rhs_idx, int is_intersect, int32_t * out_rows, int32_t * out_ok)
{
    const int call = begin("reduce_batch", ctx);
    say(" nb=%d rows=%d cols=%d rhs=%d intersect=%d", nb, rows, cols, rhs_idx, is_intersect);
    cells("cells", mats, (long long)nb * rows * cols);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) { out_ok[b] = verdict(call, b); out_rows[b] = rows - 1; stamp(mats + (size_t)b * rows * cols, call, b, 0, rows - 1, cols); }
    return end(0);
}
int xpg_lineq_remove_iden_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols, int32_t * out_rows)
{
    const int call = begin("remove_iden_batch", ctx);
    say(" nb=%d rows=%d cols=%d", nb, rows, cols);
    cells("cells", mats, (long long)nb * rows * cols);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) { out_rows[b] = rows - 1; stamp(mats + (size_t)b * rows * cols, call, b, 0, rows - 1, cols); }
    return end(0);
}
int xpg_lineq_move2var_batch_rat32(xpg_ctx * ctx, int nb, xpg_rat32 * mats, int rows, int cols, int rhs_idx, int first_sym, int last_sym)
{
    const int call = begin("move2var_batch", ctx);
    say(" nb=%d rows=%d cols=%d rhs=%d sym=%d..%d", nb, rows, cols, rhs_idx, first_sym, last_sym);
    cells("cells", mats, (long long)nb * rows * cols);
    for (int b = 0; b < nb; b++) stamp(mats + (size_t)b * rows * cols, call, b, 0, rows, cols);
    return end(rc_of(call));
}
int xpg_lineq_fme_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, int u, int darkshadow, int cap_rows,
                                     xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view, long long * row_offsets, int32_t * out_ok)
{
    const int call = begin("fme_batch_packed", ctx);
    say(" nb=%d rows=%d cols=%d rhs=%d u=%d dark=%d caps=%d outs=%d/%lld view=%d", nb, rows, cols, rhs_idx, u, darkshadow, cap_rows, outs ? 1 : 0, outs_cap_rows,
        out_view ? 1 : 0);
    cells("cells", mats, (long long)nb * rows * cols);
    return end(packed_chain(call, nb, cols, 1, out_view, row_offsets, out_ok));
}
int xpg_has_solution_rat32(xpg_ctx * ctx, const xpg_rat32 * leq, int leq_rows, const xpg_rat32 * eq, int eq_rows, const xpg_rat32 * vc, int vc_rows, int cols,
                           int rhs_idx, int is_int_sol, int is_unique_sol)
{
    const int call = begin("has_solution", ctx);
    say(" leq_rows=%d eq_rows=%d vc_rows=%d cols=%d rhs=%d int=%d unique=%d", leq_rows, eq_rows, vc_rows, cols, rhs_idx, is_int_sol, is_unique_sol);
    cells("leq", leq, (long long)leq_rows * cols); cells("eq", eq, (long long)eq_rows * cols); cells("vc", vc, (long long)vc_rows * cols);
    return end(rc_of(call) != 0 ? rc_of(call) : verdict(call, 0));
}
int xpg_lineq_bounds_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, int cap_rows, int cap_out_rows,
                                        xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view, long long * row_offsets, int32_t * out_ok,
                                        int32_t * out_chain, int32_t * out_steps)
{
    const int call = begin("bounds_batch_packed", ctx);
    say(" nb=%d rows=%d cols=%d rhs=%d caps=%d/%d outs=%d/%lld view=%d", nb, rows, cols, rhs_idx, cap_rows, cap_out_rows, outs ? 1 : 0, outs_cap_rows, out_view ? 1 : 0);
    cells("cells", mats, (long long)nb * rows * cols);
    for (int b = 0; b < nb; b++) { out_chain[b] = -1; out_steps[b] = 0; }
    return end(packed_chain(call, nb, cols, rhs_idx, out_view, row_offsets, out_ok));
}
static int packed_list(const char * name, xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, const int32_t * elim, int n_elim, int darkshadow,
                       int cap_rows, int cap_out_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view, long long * row_offsets,
                       int32_t * out_ok, int32_t * out_steps, int nres)
{
    const int call = begin(name, ctx);
    say(" nb=%d rows=%d cols=%d rhs=%d", nb, rows, cols, rhs_idx);
    arr("elim", elim, n_elim);
    say(" dark=%d caps=%d/%d outs=%d/%lld view=%d", darkshadow, cap_rows, cap_out_rows, outs ? 1 : 0, outs_cap_rows, out_view ? 1 : 0);
    cells("cells", mats, (long long)nb * rows * cols);
    for (int b = 0; b < nb; b++) out_steps[b] = 0;
    return end(packed_chain(call, nb, cols, nres, out_view, row_offsets, out_ok));
}
int xpg_lineq_project_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, const int32_t * elim, int n_elim,
                                         int darkshadow, int cap_rows, int cap_out_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                         long long * row_offsets, int32_t * out_ok, int32_t * out_steps)
{
    return packed_list("project_batch_packed", ctx, nb, mats, rows, cols, rhs_idx, elim, n_elim, darkshadow, cap_rows, cap_out_rows, outs, outs_cap_rows, out_view,
                       row_offsets, out_ok, out_steps, 1);
}
int xpg_lineq_levels_batch_packed_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, int rows, int cols, int rhs_idx, const int32_t * elim, int n_elim,
                                        int darkshadow, int cap_rows, int cap_out_rows, xpg_rat32 * outs, long long outs_cap_rows, const xpg_rat32 ** out_view,
                                        long long * row_offsets, int32_t * out_ok, int32_t * out_steps)
{
    return packed_list("levels_batch_packed", ctx, nb, mats, rows, cols, rhs_idx, elim, n_elim, darkshadow, cap_rows, cap_out_rows, outs, outs_cap_rows, out_view,
                       row_offsets, out_ok, out_steps, n_elim);
}
// what every ragged call prints of its systems
static void ragged_head(int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets, const int32_t * rhs_idx)
{
    say(" nb=%d", nb);
    arr("rows", rows, nb); arr("cols", cols, nb); arr("off", offsets, nb + 1); arr("rhs", rhs_idx, nb);
    cells("cells", mats, offsets ? offsets[nb] : 0);
}
int xpg_dep_is_empty_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                        int32_t * out_empty, long long * out_nodes)
{
    const int call = begin("dep_is_empty_batch_ragged", ctx);
    ragged_head(nb, mats, rows, cols, offsets, (const int32_t *)0);
    say(" nodes=%d", out_nodes ? 1 : 0);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) out_empty[b] = verdict(call, b);
    return end(0);
}
static int has_solution_ragged(const char * name, xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets,
                               const xpg_rat32 * eq, const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx,
                               int is_int_sol, int is_unique_sol, long long max_iter, int32_t * out_has, int32_t * out_status)
{
    const int call = begin(name, ctx);
    say(" nb=%d", nb);
    arr("leq_rows", leq_rows, nb); arr("leq_off", leq_offsets, nb + 1); cells("leq", leq, leq_offsets[nb]);
    arr("eq_rows", eq_rows, nb); arr("eq_off", eq_offsets, nb + 1); cells("eq", eq, eq_offsets[nb]);
    cells("vc", vc, (long long)vc_rows * cols);
    say(" vc_rows=%d cols=%d rhs=%d int=%d unique=%d max_iter=%lld status=%d", vc_rows, cols, rhs_idx, is_int_sol, is_unique_sol, max_iter, out_status ? 1 : 0);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) out_has[b] = verdict(call, b);
    return end(0);
}
int xpg_has_solution_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets, const xpg_rat32 * eq,
                                        const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx, int is_int_sol,
                                        int is_unique_sol, unsigned max_iter, int32_t * out_has, int32_t * out_status)
{
    return has_solution_ragged("has_solution_batch_ragged", ctx, nb, leq, leq_rows, leq_offsets, eq, eq_rows, eq_offsets, vc, vc_rows, cols, rhs_idx, is_int_sol,
                               is_unique_sol, (long long)max_iter, out_has, out_status);
}
int xpg_has_solution_int_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * leq, const int32_t * leq_rows, const long long * leq_offsets, const xpg_rat32 * eq,
                                            const int32_t * eq_rows, const long long * eq_offsets, const xpg_rat32 * vc, int vc_rows, int cols, int rhs_idx,
                                            int is_unique_sol, int32_t * out_has, int32_t * out_status)
{
    return has_solution_ragged("has_solution_int_batch_ragged", ctx, nb, leq, leq_rows, leq_offsets, eq, eq_rows, eq_offsets, vc, vc_rows, cols, rhs_idx, -1,
                               is_unique_sol, -1, out_has, out_status);
}
// the sizing protocol of the library: without room for every result XPG_ERR_SHAPE and the total in out_cell_offsets[nb]
int xpg_lineq_fme_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                     const int32_t * rhs_idx, const int32_t * u, int darkshadow, xpg_rat32 * outs, long long outs_cap_cells,
                                     long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok)
{
    const int call = begin("fme_batch_ragged", ctx);
    ragged_head(nb, mats, rows, cols, offsets, rhs_idx);
    arr("u", u, nb);
    say(" dark=%d outs=%d/%lld", darkshadow, outs ? 1 : 0, outs_cap_cells);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) out_ok[b] = verdict(call, b);
    Const one = { 1 };
    From c = { cols };
    long long total = 0;
    for (int b = 0; b < nb; b++) total += (long long)rows_of_result(b, 0, out_ok[b]) * cols[b];
    if (!outs || outs_cap_cells < total) { out_cell_offsets[nb] = total; say(" total=%lld", total); return end(XPG_ERR_SHAPE); }
    lay(call, nb, one, c, out_ok, out_cell_offsets, out_rows, outs);
    return end(0);
}
static int ragged_chain(const char * name, bool levels, xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols,
                        const long long * offsets, const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, int darkshadow, int cap_rows,
                        int cap_out_rows, xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                        int32_t * out_ok, int32_t * out_steps)
{
    const int call = begin(name, ctx);
    ragged_head(nb, mats, rows, cols, offsets, rhs_idx);
    arr("eoff", elim_offsets, nb + 1); arr("elim", elim, elim_offsets[nb]);
    say(" dark=%d caps=%d/%d outs=%d/%lld view=%d", darkshadow, cap_rows, cap_out_rows, outs ? 1 : 0, outs_cap_cells, out_view ? 1 : 0);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) { out_ok[b] = verdict(call, b); out_steps[b] = 0; }
    From c = { cols };
    const xpg_rat32 * v;
    if (levels) { Span n = { elim_offsets }; v = lay(call, nb, n, c, out_ok, out_cell_offsets, out_rows); }
    else { Const n = { 1 }; v = lay(call, nb, n, c, out_ok, out_cell_offsets, out_rows); }
    if (out_view) *out_view = v;
    return end(0);
}
int xpg_lineq_project_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                         const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, int darkshadow, int cap_rows, int cap_out_rows,
                                         xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                                         int32_t * out_ok, int32_t * out_steps)
{
    return ragged_chain("project_batch_ragged", false, ctx, nb, mats, rows, cols, offsets, rhs_idx, elim, elim_offsets, darkshadow, cap_rows, cap_out_rows, outs,
                        outs_cap_cells, out_view, out_cell_offsets, out_rows, out_ok, out_steps);
}
int xpg_lineq_levels_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                        const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, int darkshadow, int cap_rows, int cap_out_rows,
                                        xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                                        int32_t * out_ok, int32_t * out_steps)
{
    return ragged_chain("levels_batch_ragged", true, ctx, nb, mats, rows, cols, offsets, rhs_idx, elim, elim_offsets, darkshadow, cap_rows, cap_out_rows, outs,
                        outs_cap_cells, out_view, out_cell_offsets, out_rows, out_ok, out_steps);
}
int xpg_lineq_bounds_batch_ragged_rat32(xpg_ctx * ctx, int nb, const xpg_rat32 * mats, const int32_t * rows, const int32_t * cols, const long long * offsets,
                                        const int32_t * rhs_idx, int cap_rows, int cap_out_rows, xpg_rat32 * outs, long long outs_cap_cells,
                                        const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok, int32_t * out_chain,
                                        int32_t * out_steps)
{
    const int call = begin("bounds_batch_ragged", ctx);
    ragged_head(nb, mats, rows, cols, offsets, rhs_idx);
    say(" caps=%d/%d outs=%d/%lld view=%d", cap_rows, cap_out_rows, outs ? 1 : 0, outs_cap_cells, out_view ? 1 : 0);
    if (rc_of(call) != 0) return end(rc_of(call));
    for (int b = 0; b < nb; b++) { out_ok[b] = verdict(call, b); out_chain[b] = -1; out_steps[b] = 0; }
    From n = { rhs_idx }, c = { cols };
    const xpg_rat32 * v = lay(call, nb, n, c, out_ok, out_cell_offsets, out_rows);
    if (out_view) *out_view = v;
    return end(0);
}
static int groups_call(const char * name, xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats, const int32_t * rows,
                       const int32_t * cols, const long long * offsets, const int32_t * rhs_idx, const int32_t * elim, const int32_t * elim_offsets, int darkshadow,
                       int is_intersect, int cap_rows, int cap_out_rows, int cap_hull_rows, xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view,
                       long long * out_cell_offsets, int32_t * out_rows, int32_t * out_ok, int32_t * out_member, int32_t * out_chain, int32_t * out_steps)
{
    const int call = begin(name, ctx);
    say(" ng=%d", n_groups);
    arr("goff", group_offsets, n_groups + 1);
    ragged_head(n_members, mats, rows, cols, offsets, rhs_idx);
    if (elim_offsets) { arr("eoff", elim_offsets, n_members + 1); arr("elim", elim, elim_offsets[n_members]); }
    say(" dark=%d intersect=%d caps=%d/%d/%d outs=%d/%lld view=%d", darkshadow, is_intersect, cap_rows, cap_out_rows, cap_hull_rows, outs ? 1 : 0, outs_cap_cells,
        out_view ? 1 : 0);
    if (rc_of(call) != 0) return end(rc_of(call));
    std::vector<int32_t> gcols((size_t)n_groups);
    for (int g = 0; g < n_groups; g++) {
        out_ok[g] = verdict(call, g); out_member[g] = member_of(call, g); out_chain[g] = -1; out_steps[g] = 0;
        gcols[(size_t)g] = group_offsets[g + 1] > group_offsets[g] ? cols[group_offsets[g]] : 0;     // (a group without members has no result)
    }
    Const one = { 1 };
    From c = { gcols.data() };
    const xpg_rat32 * v = lay(call, n_groups, one, c, out_ok, out_cell_offsets, out_rows);
    if (out_view) *out_view = v;
    return end(0);
}
int xpg_lineq_hull_batch_ragged_rat32(xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats, const int32_t * rows,
                                      const int32_t * cols, const long long * offsets, const int32_t * rhs_idx, int is_intersect, int cap_rows, int cap_out_rows,
                                      int cap_hull_rows, xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets,
                                      int32_t * out_rows, int32_t * out_ok, int32_t * out_member, int32_t * out_chain, int32_t * out_steps)
{
    return groups_call("hull_batch_ragged", ctx, n_groups, group_offsets, n_members, mats, rows, cols, offsets, rhs_idx, (const int32_t *)0, (const int32_t *)0, -1,
                       is_intersect, cap_rows, cap_out_rows, cap_hull_rows, outs, outs_cap_cells, out_view, out_cell_offsets, out_rows, out_ok, out_member, out_chain,
                       out_steps);
}
int xpg_lineq_project_union_batch_ragged_rat32(xpg_ctx * ctx, int n_groups, const int32_t * group_offsets, int n_members, const xpg_rat32 * mats, const int32_t * rows,
                                               const int32_t * cols, const long long * offsets, const int32_t * rhs_idx, const int32_t * elim,
                                               const int32_t * elim_offsets, int darkshadow, int is_intersect, int cap_rows, int cap_out_rows, int cap_hull_rows,
                                               xpg_rat32 * outs, long long outs_cap_cells, const xpg_rat32 ** out_view, long long * out_cell_offsets, int32_t * out_rows,
                                               int32_t * out_ok, int32_t * out_member, int32_t * out_chain, int32_t * out_steps)
{
    return groups_call("project_union_batch_ragged", ctx, n_groups, group_offsets, n_members, mats, rows, cols, offsets, rhs_idx, elim, elim_offsets, darkshadow,
                       is_intersect, cap_rows, cap_out_rows, cap_hull_rows, outs, outs_cap_cells, out_view, out_cell_offsets, out_rows, out_ok, out_member, out_chain,
                       out_steps);
}
} // extern "C"

// ---------------------------------------------------------------- what a collector left
static void scenario(const std::string & name, const std::vector<Step> & script = std::vector<Step>(), int zero = -1)
{
    printf("== %s\n", name.c_str());
    g_script = script; g_call = 0; g_zero = zero;
}
static void done() { printf("calls %d\n", g_call); }
static void show(const char * key, int i, int j, const StubMat & m)
{
    if (j < 0) printf("  %s[%d] %ux%u %08x\n", key, i, m.rows, m.cols, sum(m.cells.data(), (long long)m.cells.size()));
    else printf("  %s[%d][%d] %ux%u %08x\n", key, i, j, m.rows, m.cols, sum(m.cells.data(), (long long)m.cells.size()));
}
static void show(const char * key, const std::vector<StubMat> & v) { for (size_t i = 0; i < v.size(); i++) show(key, (int)i, -1, v[i]); }
static void show(const char * key, const std::vector<std::vector<StubMat> > & v)
{
    for (size_t i = 0; i < v.size(); i++) {
        if (v[i].empty()) printf("  %s[%d] none\n", key, (int)i);
        for (size_t j = 0; j < v[i].size(); j++) show(key, (int)i, (int)j, v[i][j]);
    }
}
static void show(const char * key, const I32 & v)
{
    printf("  %s=[", key);
    for (size_t i = 0; i < v.size(); i++) printf(i ? ",%d" : "%d", (int)v[i]);
    printf("]\n");
}
static void rc_line(int rc) { printf("  rc %d%s\n", rc, rc == XPG_ERR_UNSUPPORTED ? " XPG_ERR_UNSUPPORTED" : rc == XPG_ERR_SHAPE ? " XPG_ERR_SHAPE" : ""); }
static void bool_line(bool b) { printf("  returns %s\n", b ? "true" : "false"); }

// ---------------------------------------------------------------- the eight retry loops, each on the smallest input that reaches it
static StubMat A0(3, 4, 1), A1(3, 4, 2), A2(3, 4, 3), B0(5, 3, 4), B1(5, 3, 5), Empty;

static void run_calc_bound_member() { Lin lin(&A0, 3); std::vector<StubMat> limits; bool_line(lin.calcBound(limits)); show("limits", limits); }
static void run_levels_member() { Lin lin(&A0, 3); std::vector<StubMat> aux(1, B0); bool_line(lin.fmeLevels(aux)); show("aux", aux); }
static std::vector<StubMat *> two_A() { std::vector<StubMat *> s; s.push_back(&A0); s.push_back(&A1); return s; }
static std::vector<StubMat *> A_and_B() { std::vector<StubMat *> s; s.push_back(&A0); s.push_back(&B0); return s; }
static I32 ints(int a, int b = -99, int c = -99) { I32 v(1, a); if (b != -99) v.push_back(b); if (c != -99) v.push_back(c); return v; }
static void run_project_all()
{
    std::vector<StubMat> res; I32 ok;
    rc_line(xpoly_amd::project_all(two_A(), ints(2, 1), 3, res, ok)); show("ok", ok); show("res", res);
}
static void run_levels_all()
{
    std::vector<std::vector<StubMat> > lev; I32 ok;
    rc_line(xpoly_amd::levels_all(two_A(), ints(2, 1), 3, lev, ok)); show("ok", ok); show("lev", lev);
}
static void run_project_each()
{
    std::vector<StubMat> res; I32 ok;
    std::vector<I32> elims; elims.push_back(ints(2, 1)); elims.push_back(ints(1));
    rc_line(xpoly_amd::project_each(A_and_B(), elims, ints(3, 2), res, ok)); show("ok", ok); show("res", res);
}
static void run_levels_nests()
{
    std::vector<std::vector<StubMat> > lev; I32 ok;
    rc_line(xpoly_amd::levels_nests(A_and_B(), ints(3, 2), lev, ok)); show("ok", ok); show("lev", lev);
}
static void run_calc_bound_all()
{
    std::vector<std::vector<StubMat> > lim; I32 ok;
    rc_line(xpoly_amd::calc_bound_all(two_A(), ints(3, 3), lim, ok)); show("ok", ok); show("lim", lim);
}
static void run_calc_bound_each()
{
    std::vector<std::vector<StubMat> > lim; I32 ok;
    rc_line(xpoly_amd::calc_bound_each(A_and_B(), ints(3, 2), lim, ok)); show("ok", ok); show("lim", lim);
}
static std::vector<std::vector<StubMat *> > two_groups() { std::vector<std::vector<StubMat *> > g; g.push_back(two_A()); g.push_back(std::vector<StubMat *>(1, &B0)); return g; }
static std::vector<std::vector<I32> > group_elims()
{
    std::vector<std::vector<I32> > e(2);
    e[0].push_back(ints(2, 1)); e[0].push_back(ints(2)); e[1].push_back(ints(1));
    return e;
}
static void run_hull_all()
{
    std::vector<StubMat> res; I32 ok, mem;
    rc_line(xpoly_amd::hull_all(two_groups(), ints(3, 2), false, res, ok, (xpg_ctx *)0, &mem)); show("ok", ok); show("member", mem); show("res", res);
}
static void run_project_union_each()
{
    std::vector<StubMat> res; I32 ok, mem;
    rc_line(xpoly_amd::project_union_each(two_groups(), group_elims(), ints(3, 2), true, res, ok, (xpg_ctx *)0, true, &mem)); show("ok", ok); show("member", mem); show("res", res);
}

static std::map<int, int> kv(int k0, int v0, int k1 = -99, int v1 = 0) { std::map<int, int> m; m[k0] = v0; if (k1 != -99) m[k1] = v1; return m; }
static void retry_runs(const char * loop, void (*run)(), bool two, bool hull)
{
    const std::string l(loop);
    scenario(l + ": answered at once"); run(); done();
    scenario(l + ": a step short (need > cap)", std::vector<Step>(1, S(0, kv(0, -43), kv(0, 0)))); run(); done();
    scenario(l + ": a slot short (need <= cap)", std::vector<Step>(1, S(0, kv(0, -3), kv(0, 0)))); run(); done();
    if (two) { scenario(l + ": both in one call", std::vector<Step>(1, S(0, kv(0, -43, 1, -3), kv(0, 1, 1, 0)))); run(); done(); }
    if (hull) {
        scenario(l + ": a group short (member -1)", std::vector<Step>(1, S(0, kv(1, -50)))); run(); done();
        scenario(l + ": a member and a group short", std::vector<Step>(1, S(0, kv(0, -43, 1, -50), kv(0, 1)))); run(); done();
    }
    std::vector<Step> then; then.push_back(S(0, kv(0, -43), kv(0, 0))); then.push_back(S(0, kv(two ? 1 : 0, -3), kv(1, 0)));
    scenario(l + ": a step short, then a slot", then); run(); done();
    std::vector<Step> never;
    for (int k = 0; k < 6; k++) never.push_back(S(0, kv(0, -100 * (k + 1)), kv(0, 0)));
    scenario(l + ": never satisfied", never); run(); done();
    std::vector<Step> rc2; rc2.push_back(S(0, kv(0, -43), kv(0, 0))); rc2.push_back(S(XPG_ERR_HIP));
    scenario(l + ": a return code on the second call", rc2); run(); done();
}

// ---------------------------------------------------------------- the class walk
static std::vector<StubMat *> six_systems()
{
    StubMat * s[6] = { &A0, &B0, &A1, &Empty, &B1, &A2 };
    return std::vector<StubMat *>(s, s + 6);
}
static void class_walk()
{
    const std::vector<StubMat *> six = six_systems();
    {
        scenario("class walk: project_all over A B A empty B A", std::vector<Step>(1, S(0, kv(1, 0))));
        std::vector<StubMat> res; I32 ok;
        rc_line(xpoly_amd::project_all(six, ints(2, 1), 3, res, ok, (xpg_ctx *)&g_own_ctx, true)); show("ok", ok); show("res", res); done();
    }
    {
        scenario("class walk: levels_all over A B A empty B A", std::vector<Step>(1, S(0, kv(1, 0))));
        std::vector<std::vector<StubMat> > lev; I32 ok;
        rc_line(xpoly_amd::levels_all(six, ints(2, 1), 3, lev, ok, (xpg_ctx *)&g_own_ctx, true)); show("ok", ok); show("lev", lev); done();
    }
    {
        scenario("class walk: calc_bound_all over A B A empty B A refuses the empty system when its class comes up");
        std::vector<std::vector<StubMat> > lim; I32 ok;
        I32 rhs; rhs.push_back(3); rhs.push_back(2); rhs.push_back(3); rhs.push_back(1); rhs.push_back(2); rhs.push_back(3);
        rc_line(xpoly_amd::calc_bound_all(six, rhs, lim, ok, (xpg_ctx *)&g_own_ctx)); show("ok", ok); show("lim", lim); done();
    }
    {
        scenario("class walk: calc_bound_all, equal shapes and different rhs_idx are two classes");
        std::vector<StubMat *> s; s.push_back(&A0); s.push_back(&A1); s.push_back(&A2);
        std::vector<std::vector<StubMat> > lim; I32 ok;
        rc_line(xpoly_amd::calc_bound_all(s, ints(3, 2, 3), lim, ok)); show("ok", ok); show("lim", lim); done();
    }
    {
        scenario("class walk: refusals before any call");
        std::vector<StubMat> res; std::vector<std::vector<StubMat> > lev; I32 ok;
        rc_line(xpoly_amd::project_all(six, I32(), 3, res, ok)); show("ok", ok); show("res", res);
        rc_line(xpoly_amd::project_all(six, ints(1), 0, res, ok));
        rc_line(xpoly_amd::levels_all(six, I32(), 3, lev, ok)); show("ok", ok); show("lev", lev);
        rc_line(xpoly_amd::calc_bound_all(six, ints(3, 2), lev, ok));
        rc_line(xpoly_amd::calc_bound_each(six, ints(3, 2), lev, ok));
        I32 rhs(6, 2);
        rc_line(xpoly_amd::calc_bound_each(six, rhs, lev, ok)); show("ok", ok); show("lev", lev);           // the empty system
        rc_line(xpoly_amd::calc_bound_each(two_A(), ints(3, 4), lev, ok));                                   // rhs_idx >= cols
        rc_line(xpoly_amd::calc_bound_each(std::vector<StubMat *>(), I32(), lev, ok));                       // no systems: 0
        done();
    }
    {
        scenario("ragged fronts: project_each and levels_nests answer empty systems and depth 1 themselves");
        std::vector<StubMat *> s = six; s.push_back(&B0);
        std::vector<StubMat> res; std::vector<std::vector<StubMat> > lev; I32 ok;
        I32 rhs; rhs.push_back(3); rhs.push_back(2); rhs.push_back(3); rhs.push_back(2); rhs.push_back(2); rhs.push_back(3); rhs.push_back(1);
        std::vector<I32> elims(7, ints(1)); elims[0] = ints(2, 1); elims[5] = ints(2);
        rc_line(xpoly_amd::project_each(s, elims, rhs, res, ok, (xpg_ctx *)&g_own_ctx, true)); show("ok", ok); show("res", res);
        rc_line(xpoly_amd::levels_nests(s, rhs, lev, ok)); show("ok", ok); show("lev", lev);
        elims[2].clear();
        rc_line(xpoly_amd::project_each(s, elims, rhs, res, ok));                                           // an empty list
        rhs[4] = 0;
        rc_line(xpoly_amd::levels_nests(s, rhs, lev, ok));                                                  // rhs_idx < 1
        rc_line(xpoly_amd::levels_nests(s, ints(3), lev, ok));
        std::vector<StubMat *> e(2, &Empty);
        rc_line(xpoly_amd::levels_nests(e, ints(2, 3), lev, ok)); show("ok", ok); show("lev", lev);          // nothing travels: no call
        done();
    }
}

// ---------------------------------------------------------------- fme_all, has_solution_all, dep_is_empty_all
static void flat_collectors()
{
    {
        scenario("fme_all: empty systems are answered, the rest goes up in one call", std::vector<Step>(1, S(0, kv(1, 0))));
        std::vector<StubMat *> s; s.push_back(&Empty); s.push_back(&A0); s.push_back(&B0); s.push_back(&Empty); s.push_back(&A1);
        std::vector<StubMat> res(1, B1); I32 ok;
        I32 u; u.push_back(0); u.push_back(1); u.push_back(0); u.push_back(2); u.push_back(2);
        rc_line(xpoly_amd::fme_all(s, u, I32(), res, ok)); show("ok", ok); show("res", res);
        I32 rhs; rhs.push_back(9); rhs.push_back(2); rhs.push_back(1); rhs.push_back(9); rhs.push_back(3);
        rc_line(xpoly_amd::fme_all(s, u, rhs, res, ok, true, (xpg_ctx *)&g_own_ctx)); show("ok", ok); show("res", res);
        done();
    }
    {
        scenario("fme_all: only empty systems, and the refusals: no call");
        std::vector<StubMat *> s(2, &Empty);
        std::vector<StubMat> res; I32 ok;
        rc_line(xpoly_amd::fme_all(s, ints(0, 0), I32(), res, ok)); show("ok", ok); show("res", res);
        rc_line(xpoly_amd::fme_all(s, ints(0), I32(), res, ok));
        rc_line(xpoly_amd::fme_all(s, ints(0, 0), ints(1), res, ok));
        done();
    }
    {
        scenario("fme_all: a return code is passed on", std::vector<Step>(1, S(XPG_ERR_HIP)));
        std::vector<StubMat> res; I32 ok;
        rc_line(xpoly_amd::fme_all(two_A(), ints(0, 1), I32(), res, ok)); show("ok", ok); show("res", res); done();
    }
    {
        scenario("fme_all: above 64 MiB of worst case a sizing call, then one with exactly that many cells");
        StubMat big(6000, 1, 7);
        std::vector<StubMat *> s; s.push_back(&big); s.push_back(&A0);
        std::vector<StubMat> res; I32 ok;
        rc_line(xpoly_amd::fme_all(s, ints(0, 1), I32(), res, ok)); show("ok", ok); show("res", res); done();
    }
    {
        scenario("fme_all: the sizing call answered by another code ends the call", std::vector<Step>(1, S(XPG_ERR_ALLOC)));
        StubMat big(6000, 1, 7);
        std::vector<StubMat> res; I32 ok;
        rc_line(xpoly_amd::fme_all(std::vector<StubMat *>(1, &big), ints(0), I32(), res, ok)); show("ok", ok); show("res", res); done();
    }
    StubMat vc(2, 3, 8), l0(2, 3, 9), l3(1, 3, 10), e1(1, 3, 11), e2(2, 3, 12), rowless, wrong(2, 4, 13);
    rowless.reinit(0, 3);
    std::vector<StubMat *> leqs, eqs;
    leqs.push_back(&l0); leqs.push_back((StubMat *)0); leqs.push_back(&Empty); leqs.push_back(&l3); leqs.push_back(&rowless);
    eqs.push_back((StubMat *)0); eqs.push_back(&e1); eqs.push_back(&e2); eqs.push_back(&rowless); eqs.push_back((StubMat *)0);
    for (int is_int = 0; is_int < 2; is_int++) {
        scenario(is_int ? "has_solution_all: the integer call" : "has_solution_all: the plain call", std::vector<Step>(1, S(0, kv(1, 0, 3, XPG_ERR_REF_UNDEFINED))));
        I32 out;
        rc_line(xpoly_amd::has_solution_all(leqs, eqs, vc, 2, is_int != 0, is_int == 0, out, is_int ? (xpg_ctx *)&g_own_ctx : (xpg_ctx *)0)); show("out", out); done();
    }
    {
        scenario("has_solution_all: no inequality at all goes up as a null pointer");
        std::vector<StubMat *> none(2, (StubMat *)0), some; some.push_back(&e1); some.push_back(&e2);
        I32 out;
        rc_line(xpoly_amd::has_solution_all(none, some, vc, 2, false, false, out)); show("out", out); done();
    }
    {
        scenario("has_solution_all: every refusal is made before any call");
        I32 out(1, 7);
        std::vector<StubMat *> bad = leqs; bad[3] = &wrong;
        rc_line(xpoly_amd::has_solution_all(leqs, std::vector<StubMat *>(1, &e1), vc, 2, false, false, out));
        rc_line(xpoly_amd::has_solution_all(leqs, eqs, vc, 0, false, false, out));
        rc_line(xpoly_amd::has_solution_all(leqs, eqs, l3, 2, false, false, out));
        rc_line(xpoly_amd::has_solution_all(leqs, eqs, wrong, 2, false, false, out)); show("out", out);
        rc_line(xpoly_amd::has_solution_all(bad, eqs, vc, 2, true, false, out)); show("out", out);
        rc_line(xpoly_amd::has_solution_all(leqs, bad, vc, 2, false, false, out));
        rc_line(xpoly_amd::has_solution_all(std::vector<StubMat *>(), std::vector<StubMat *>(), vc, 2, false, false, out)); show("out", out);
        done();
    }
    {
        scenario("dep_is_empty_all: polyhedra of any shape, row-less and empty ones too", std::vector<Step>(1, S(0, kv(0, 0, 2, XPG_ERR_REF_UNDEFINED))));
        std::vector<StubMat *> p; p.push_back(&A0); p.push_back(&rowless); p.push_back(&B0); p.push_back(&Empty); p.push_back(&A1);
        I32 empty(1, 7);
        rc_line(xpoly_amd::dep_is_empty_all(p, empty)); show("empty", empty);
        rc_line(xpoly_amd::dep_is_empty_all(std::vector<StubMat *>(), empty, (xpg_ctx *)&g_own_ctx)); show("empty", empty);
        done();
    }
    {
        scenario("dep_is_empty_all: a return code is passed on", std::vector<Step>(1, S(XPG_ERR_NO_DEVICE)));
        I32 empty;
        rc_line(xpoly_amd::dep_is_empty_all(two_A(), empty)); show("empty", empty); done();
    }
}

// ---------------------------------------------------------------- hull_groups through its four fronts
static void hull_fronts()
{
    std::vector<Step> one(1, S(0, kv(0, 0), kv(0, 1)));           // group 0: member 1 fails
    scenario("hull_all: two groups of 2 and 1, a failing member, a result without rows", one, 1); run_hull_all(); done();
    scenario("project_union_each: two groups of 2 and 1, a failing member, a result without rows", one, 1); run_project_union_each(); done();
    {
        scenario("hull_all: without a member vector, group 1 inconsistent", std::vector<Step>(1, S(0, kv(1, 0))));
        std::vector<StubMat> res(3, A0); I32 ok;
        rc_line(xpoly_amd::hull_all(two_groups(), ints(3, 2), true, res, ok, (xpg_ctx *)&g_own_ctx)); show("ok", ok); show("res", res); done();
    }
    {
        scenario("hull_all and project_union_each: the refusals, no call");
        std::vector<StubMat> res; I32 ok, mem;
        std::vector<std::vector<StubMat *> > g = two_groups();
        rc_line(xpoly_amd::hull_all(g, ints(3), false, res, ok));
        std::vector<std::vector<I32> > e = group_elims();
        e.pop_back();
        rc_line(xpoly_amd::project_union_each(g, e, ints(3, 2), false, res, ok));
        e = group_elims(); e[0].pop_back();
        rc_line(xpoly_amd::project_union_each(g, e, ints(3, 2), false, res, ok, (xpg_ctx *)0, false, &mem)); show("ok", ok); show("member", mem); show("res", res);
        g[1][0] = &Empty;
        rc_line(xpoly_amd::hull_all(g, ints(3, 2), false, res, ok, (xpg_ctx *)0, &mem)); show("ok", ok); show("member", mem); show("res", res);
        rc_line(xpoly_amd::hull_all(std::vector<std::vector<StubMat *> >(), I32(), false, res, ok, (xpg_ctx *)0, &mem)); show("ok", ok); show("member", mem); show("res", res);
        g[1].clear();                                                // a group without members travels
        rc_line(xpoly_amd::hull_all(g, ints(3, 2), false, res, ok, (xpg_ctx *)0, &mem)); show("ok", ok); show("member", mem); show("res", res);
        done();
    }
    std::vector<StubMat *> lst = two_A();
    StubList list; list.v = lst;
    struct { const char * name; std::vector<Step> script; int zero; } runs[5] = {
        { "a hull", std::vector<Step>(), -1 },
        { "a result without rows cleans res", std::vector<Step>(), 0 },
        { "a failing member cleans res", std::vector<Step>(1, S(0, kv(0, 0), kv(0, 1))), -1 },
        { "an inconsistent intersection cleans res", std::vector<Step>(1, S(0, kv(0, 0))), -1 },
        { "a return code cleans res", std::vector<Step>(1, S(XPG_ERR_HIP)), -1 } };
    for (int k = 0; k < 5; k++) {
        scenario(std::string("ConvexHullUnionAndIntersect: ") + runs[k].name, runs[k].script, runs[k].zero);
        StubMat r1 = B0, r2 = B0;
        Lin lin(0), own(0, -1, (xpg_ctx *)&g_own_ctx);
        lin.ConvexHullUnionAndIntersect(r1, lst, 3, k == 3); show("res", 0, -1, r1);
        own.ConvexHullUnionAndIntersect(r2, list, 3, k == 3); show("res", 1, -1, r2);
        done();
    }
    {
        scenario("ConvexHullUnionAndIntersect: an empty list cleans res, no call");
        std::vector<StubMat *> none; StubList nolist;
        StubMat r1 = B0, r2 = B0;
        Lin lin(0);
        lin.ConvexHullUnionAndIntersect(r1, none, 3, false); show("res", 0, -1, r1);
        lin.ConvexHullUnionAndIntersect(r2, nolist, 3, true); show("res", 1, -1, r2);
        done();
    }
}

// ---------------------------------------------------------------- the members
static void members()
{
    {
        scenario("reduce: kept rows come back, ok is the verdict", std::vector<Step>(1, S(0)));
        Lin lin(0);
        StubMat m = A0; bool_line(lin.reduce(m, 3, true)); show("m", 0, -1, m);
        g_script.assign(2, S(0, kv(0, 0)));
        m = B0; bool_line(lin.reduce(m, 2, false)); show("m", 1, -1, m);
        g_script.assign(3, S(XPG_ERR_HIP));
        m = A1; bool_line(lin.reduce(m, 3, false)); show("m", 2, -1, m);
        m = Empty; bool_line(lin.reduce(m, 0, false)); show("m", 3, -1, m);                 // no rows: true, no call
        done();
    }
    {
        scenario("removeIdenRow");
        Lin lin(0, -1, (xpg_ctx *)&g_own_ctx);
        StubMat m = A0; lin.removeIdenRow(m); show("m", 0, -1, m);
        g_script.assign(2, S(XPG_ERR_HIP));
        m = B0; lin.removeIdenRow(m); show("m", 1, -1, m);
        m = Empty; lin.removeIdenRow(m); show("m", 2, -1, m);
        done();
    }
    {
        scenario("move2var");
        Lin lin(0);
        StubMat m(3, 6, 14);
        unsigned first = 0, last = 0;
        lin.move2var(m, 3, 4, 5, &first, &last); show("m", 0, -1, m); printf("  first %u last %u\n", first, last);
        lin.move2var(m, 3, 4, 4, (unsigned *)0, (unsigned *)0);
        done();
    }
    {
        scenario("fme", std::vector<Step>(1, S(0)), -1);
        StubMat sys = B1, res = A0;
        Lin lin(&sys);                                                // the constant column: the last one
        bool_line(lin.fme(1, res)); show("res", 0, -1, res);
        g_script.assign(2, S(0, kv(0, 0)));
        bool_line(lin.fme(0, res, true)); show("res", 1, -1, res);
        g_script.assign(3, S(XPG_ERR_HIP));
        res = A0; bool_line(lin.fme(0, res)); show("res", 2, -1, res);
        lin.set_param(&Empty, 2);
        res = A0; bool_line(lin.fme(0, res)); show("res", 3, -1, res);                      // an empty system stays empty, no call
        done();
    }
    {
        scenario("has_solution", std::vector<Step>(1, S(0)));
        StubMat vc(2, 3, 8), leq(2, 3, 9), eq(1, 3, 11), none;
        Lin lin(0);
        bool_line(lin.has_solution(leq, eq, vc, 2, true, false));
        g_script.assign(2, S(0, kv(0, 0)));
        bool_line(lin.has_solution(none, eq, vc, 2, false, true));
        g_script.assign(3, S(XPG_ERR_REF_UNDEFINED));
        bool_line(lin.has_solution(leq, none, vc, 2, false, false));
        bool_line(lin.has_solution(none, none, vc, 2, false, false));                       // nothing to ask: false, no call
        done();
    }
    {
        scenario("calcBound into a vector and into a list");
        StubMat sys = A0;
        Lin lin(&sys, 3, (xpg_ctx *)&g_own_ctx);
        std::vector<StubMat> limits(5, B0);
        bool_line(lin.calcBound(limits)); show("limits", limits);
        StubMat l0 = B0, l1 = B0, l2 = B0;
        StubList list; list.v.push_back(&l0); list.v.push_back(&l1); list.v.push_back(&l2);
        bool_line(lin.calcBound(list)); show("l", 0, -1, l0); show("l", 1, -1, l1); show("l", 2, -1, l2);
        list.v.pop_back();
        bool_line(lin.calcBound(list));                                                     // not m_rhs_idx matrices: false, no call
        g_script.assign(3, S(0, kv(0, 0)));
        bool_line(lin.calcBound(limits)); show("limits", limits);                           // inconsistent: false, limits as they were
        done();
    }
    {
        scenario("fmeLevels into a vector: [0] the outermost bound, back() the system");
        StubMat sys = A0, a = B0;
        Lin lin(&sys, 3);
        std::vector<StubMat> aux(1, B0);
        bool_line(lin.fmeLevels(aux, &a)); show("aux", aux); show("A", 0, -1, a);
        bool_line(lin.fmeLevels(aux, &sys)); show("aux", aux); show("sys", 0, -1, sys);       // A being the system itself
        g_script.assign(3, S(0, kv(0, 0)));
        sys = A0; aux.assign(1, B0);
        bool_line(lin.fmeLevels(aux, &a)); show("aux", aux); show("A", 0, -1, a);           // inconsistent: false, all as it was
        done();
    }
    {
        scenario("fmeLevels into a list: the tail receives the system, the head the outermost bound");
        StubMat sys = A0, a = B0, l0 = B0, l1 = B0, l2 = B0;
        Lin lin(&sys, 3, (xpg_ctx *)&g_own_ctx);
        StubList list; list.v.push_back(&l0); list.v.push_back(&l1); list.v.push_back(&l2);
        bool_line(lin.fmeLevels(list, &a)); show("l", 0, -1, l0); show("l", 1, -1, l1); show("l", 2, -1, l2); show("A", 0, -1, a);
        bool_line(lin.fmeLevels(list, &sys)); show("l", 0, -1, l0); show("sys", 0, -1, sys);
        sys = A0;
        bool_line(lin.fmeLevels(list)); show("l", 0, -1, l0);
        list.v[1] = &sys;
        bool_line(lin.fmeLevels(list));                                                     // an entry is the system itself: false, no call
        list.v.pop_back();
        bool_line(lin.fmeLevels(list));                                                     // not m_rhs_idx matrices: false
        done();
    }
    {
        scenario("fmeLevels: depth 1 and an empty system copy and make no call");
        StubMat sys(3, 2, 15), a = B0, l0 = B0;
        Lin lin(&sys, 1);
        std::vector<StubMat> aux;
        bool_line(lin.fmeLevels(aux, &a)); show("aux", aux); show("A", 0, -1, a);
        StubList list; list.v.push_back(&l0);
        bool_line(lin.fmeLevels(list, &a)); show("l", 0, -1, l0);
        lin.set_param(&Empty, 3);
        bool_line(lin.fmeLevels(aux, &a)); show("aux", aux); show("A", 0, -1, a);
        lin.set_param(&sys, 0);
        bool_line(lin.fmeLevels(aux));                                                      // m_rhs_idx < 1: false
        done();
    }
}

// ---------------------------------------------------------------- --time
static StubMat nest(int depth, int extra, int seed) { return StubMat((unsigned)(2 * depth + extra), (unsigned)(depth + 1), seed); }
static const char * g_only = 0;                                  // --time NAME: that collector alone
template <class Fn> static void timed(const char * name, Fn fn)
{
    if (g_only && std::strcmp(g_only, name) != 0) return;
    std::vector<double> us;
    for (int k = 0; k < 5; k++) fn();
    for (int k = 0; k < 101; k++) {
        const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
        fn();
        us.push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(us.begin(), us.end());
    printf("%-20s %10.2f\n", name, us[us.size() / 2]);
}
static int time_mode()
{
    g_quiet = true; g_script.clear();
    const int nb = 692;
    std::vector<StubMat> mats, fives;
    std::vector<StubMat *> sys, five;
    I32 rhs, u;
    std::vector<I32> elims;
    for (int b = 0; b < nb; b++) {
        const int cls = (7 * b) % 20, d = 2 + cls / 4, e = cls % 4;
        mats.push_back(nest(d, e, b % 90)); fives.push_back(nest(4, b % 4, b % 90));
        rhs.push_back(d); u.push_back(d - 1);
        I32 el; for (int v = d - 1; v > 0; v--) el.push_back(v);
        elims.push_back(el);
    }
    for (int b = 0; b < nb; b++) { sys.push_back(&mats[(size_t)b]); five.push_back(&fives[(size_t)b]); }
    std::vector<std::vector<StubMat *> > groups;                  // hulls of 2 members of one class
    std::vector<std::vector<I32> > gelims;
    I32 grhs;
    for (int g = 0; g < nb / 2; g++) {
        const int cls = (7 * g) % 20;
        std::vector<StubMat *> grp; std::vector<I32> ge;
        for (int b = g % 20 + 20 * (g % 9), n = 0; n < 2; b += 20, n++) { grp.push_back(sys[(size_t)b]); ge.push_back(elims[(size_t)b]); }   // system b is of class (7 b) % 20
        groups.push_back(grp); gelims.push_back(ge); grhs.push_back(2 + cls / 4);
    }
    StubMat vc(4, 5, 1);
    std::vector<StubMat> res;
    std::vector<std::vector<StubMat> > nested;
    I32 ok;
    printf("median microseconds per call, %d systems over 20 shape classes, %d groups of 2\n", nb, nb / 2);
    timed("dep_is_empty_all", [&] { xpoly_amd::dep_is_empty_all(sys, ok); });
    timed("has_solution_all", [&] { xpoly_amd::has_solution_all(five, five, vc, 4, false, false, ok); });
    timed("fme_all", [&] { xpoly_amd::fme_all(sys, u, rhs, res, ok); });
    timed("project_all", [&] { xpoly_amd::project_all(sys, ints(1), 2, res, ok); });
    timed("levels_all", [&] { xpoly_amd::levels_all(sys, ints(1), 2, nested, ok); });
    timed("project_each", [&] { xpoly_amd::project_each(sys, elims, rhs, res, ok); });
    timed("levels_nests", [&] { xpoly_amd::levels_nests(sys, rhs, nested, ok); });
    timed("calc_bound_all", [&] { xpoly_amd::calc_bound_all(sys, rhs, nested, ok); });
    timed("calc_bound_each", [&] { xpoly_amd::calc_bound_each(sys, rhs, nested, ok); });
    timed("hull_all", [&] { xpoly_amd::hull_all(groups, grhs, false, res, ok); });
    timed("project_union_each", [&] { xpoly_amd::project_union_each(groups, gelims, grhs, false, res, ok); });
    Lin lin(sys[19], rhs[19]);                                       // the deepest nest with the most bounds
    timed("Lineq::calcBound", [&] { lin.calcBound(res); });
    timed("Lineq::fmeLevels", [&] { lin.fmeLevels(res); });
    return 0;
}

int main(int argc, char ** argv)
{
    if (argc > 1 && std::strcmp(argv[1], "--time") == 0) { g_only = argc > 2 ? argv[2] : 0; return time_mode(); }
    class_walk();
    retry_runs("Lineq::calcBound", run_calc_bound_member, false, false);
    retry_runs("Lineq::fmeLevels", run_levels_member, false, false);
    retry_runs("project_all", run_project_all, true, false);
    retry_runs("levels_all", run_levels_all, true, false);
    retry_runs("project_each", run_project_each, true, false);
    retry_runs("levels_nests", run_levels_nests, true, false);
    retry_runs("calc_bound_all", run_calc_bound_all, true, false);
    retry_runs("calc_bound_each", run_calc_bound_each, true, false);
    retry_runs("hull_all", run_hull_all, true, true);
    retry_runs("project_union_each", run_project_union_each, true, true);
    flat_collectors();
    hull_fronts();
    members();
    return 0;
}
