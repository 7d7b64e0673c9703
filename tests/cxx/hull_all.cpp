// xpoly_amd::Lineq<M>::ConvexHullUnionAndIntersect (a minimal list type, and the std::vector overload), xpoly_amd::hull_all and
// xpoly_amd::project_union_each (include/xpoly_amd/lineq.hpp), checked in here against the composition of the calls that were
// there before them: xpoly_amd::calc_bound_each (project_each for the union) on all members, the bounds of every group
// concatenated behind a zero row on the host, and Lineq::reduce on that matrix. The stub matrix type offers what they rely on.
// Reads groups of rational systems from the file named by argv[1]:
//   groups
//   per group: members rhs_idx, then per member: rows cols, then rows x cols cells, numerator and denominator each
// and prints "rc <hull_all union> <hull_all intersect> <project_union_each>", "route <producer launches> <group launches> <grid>"
// (xpg_lineq_hull_last_route after the first hull_all: what its LAST library call did), one line
// "<g> ok <union> <intersect> rows <union> <intersect> same <0|1>" per group, and "mismatches <n>". Exit status 0 iff every call
// returns 0 and nothing differs. tests/test_lineq_hull_host.py compiles and links it, tests/test_gpu_lineq_hull.py runs it.
#include <cstdio>
#include <cstring>
#include <vector>
#include "xpoly_amd/lineq.hpp"

struct StubMat {
    unsigned rows, cols;
    std::vector<xpg_rat32> cells;
    StubMat() : rows(0), cols(0) {}
    unsigned get_row_size() const { return rows; }
    unsigned get_col_size() const { return cols; }
    unsigned size() const { return rows * cols; }
    const xpg_rat32 * get_matrix() const { return cells.data(); }
    void reinit(unsigned r, unsigned c) { rows = r; cols = c; xpg_rat32 z; z.num = 0; z.den = 1; cells.assign((size_t)r * c, z); }
    void clean() { rows = 0; cols = 0; cells.clear(); }
    void grow(const StubMat & o) { cols = o.cols; rows += o.rows; cells.insert(cells.end(), o.cells.begin(), o.cells.end()); }
    bool read(FILE * f, unsigned r, unsigned c)
    {
        reinit(r, c);
        for (size_t k = 0; k < cells.size(); k++) {
            int x, y;
            if (fscanf(f, "%d %d", &x, &y) != 2) return false;
            cells[k].num = x; cells[k].den = y;
        }
        return true;
    }
    bool same(const StubMat & o) const
    {
        if (size() == 0 || o.size() == 0) return size() == o.size();
        return rows == o.rows && cols == o.cols && std::memcmp((const void *)get_matrix(), (const void *)o.get_matrix(), sizeof(xpg_rat32) * size()) == 0;
    }
};
// what the reference's List<RMat*> offers the member function
struct StubList {
    std::vector<StubMat *> v; size_t at;
    StubList() : at(0) {}
    StubMat * get_head() { at = 0; return v.empty() ? 0 : v[0]; }
    StubMat * get_next() { return ++at < v.size() ? v[at] : 0; }
    unsigned get_elem_count() const { return (unsigned)v.size(); }
};
typedef xpoly_amd::Lineq<StubMat> Lin;

// parts[i]: what member i contributes; lead: a zero row in front. The composition's answer for one group.
static bool composed(const std::vector<const StubMat *> & parts, unsigned cols, bool lead, int rhs, bool is_intersect, StubMat & res)
{
    res.clean();
    if (lead) res.reinit(1, cols);
    for (size_t i = 0; i < parts.size(); i++) if (parts[i]->size() != 0) res.grow(*parts[i]);
    if (res.size() == 0) return true;
    Lin lin(0);
    const bool ok = lin.reduce(res, (unsigned)rhs, is_intersect);
    if (!ok && is_intersect) res.clean();
    return ok;
}

int main(int argc, char ** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: hull_all FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int ng;
    if (fscanf(f, "%d", &ng) != 1 || ng < 0) return 2;
    std::vector<std::vector<StubMat> > sys((size_t)ng);
    std::vector<int32_t> rhs((size_t)ng);
    for (int g = 0; g < ng; g++) {
        int n, h;
        if (fscanf(f, "%d %d", &n, &h) != 2 || n < 0) return 2;
        rhs[(size_t)g] = h;
        sys[(size_t)g].resize((size_t)n);
        for (int i = 0; i < n; i++) {
            int r, c;
            if (fscanf(f, "%d %d", &r, &c) != 2 || r < 0 || c < 0 || !sys[(size_t)g][(size_t)i].read(f, (unsigned)r, (unsigned)c)) return 2;
        }
    }
    fclose(f);
    std::vector<std::vector<StubMat *> > groups((size_t)ng);
    std::vector<StubMat *> flat;
    std::vector<int32_t> flat_rhs;
    std::vector<std::vector<std::vector<int32_t> > > elims((size_t)ng);
    std::vector<std::vector<int32_t> > flat_elims;
    for (int g = 0; g < ng; g++)
        for (size_t i = 0; i < sys[(size_t)g].size(); i++) {
            groups[(size_t)g].push_back(&sys[(size_t)g][i]);
            flat.push_back(&sys[(size_t)g][i]); flat_rhs.push_back(rhs[(size_t)g]);
            std::vector<int32_t> e;                                  // onto variable 0: rhs-1 .. 1 (depth 1: variable 0 itself)
            for (int u = rhs[(size_t)g] - 1; u >= 1; u--) e.push_back(u);
            if (e.empty()) e.push_back(0);
            elims[(size_t)g].push_back(e); flat_elims.push_back(e);
        }
    std::vector<StubMat> got[2], uni;
    std::vector<int32_t> ok[2], mem[2], uok, umem;
    const int rc0 = xpoly_amd::hull_all(groups, rhs, false, got[0], ok[0], (xpg_ctx *)0, &mem[0]);
    long long route[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    xpg_lineq_hull_last_route(route, 10);
    const int rc1 = xpoly_amd::hull_all(groups, rhs, true, got[1], ok[1], (xpg_ctx *)0, &mem[1]);
    const int rc2 = xpoly_amd::project_union_each(groups, elims, rhs, false, uni, uok, (xpg_ctx *)0, false, &umem);
    printf("rc %d %d %d\n", rc0, rc1, rc2);
    printf("route %lld %lld %lld\n", route[0], route[1], route[2]);
    if (rc0 != 0 || rc1 != 0 || rc2 != 0) return 1;
    // the calls that were there before: every member's bounds, every member's projection
    std::vector<std::vector<StubMat> > limits;
    std::vector<StubMat> proj;
    std::vector<int32_t> bok, pok;
    if (xpoly_amd::calc_bound_each(flat, flat_rhs, limits, bok) != 0) { printf("calc_bound_each failed\n"); return 1; }
    if (!flat.empty() && xpoly_amd::project_each(flat, flat_elims, flat_rhs, proj, pok) != 0) { printf("project_each failed\n"); return 1; }
    int mismatches = 0;
    size_t b = 0;
    for (int g = 0; g < ng; g++) {
        const size_t n = groups[(size_t)g].size();
        const unsigned cols = n ? groups[(size_t)g][0]->get_col_size() : 0;
        int bad_b = -1, bad_p = -1;
        std::vector<const StubMat *> bparts, pparts;
        for (size_t i = 0; i < n; i++) {
            if (bok[b + i] != 1 && bad_b < 0) bad_b = (int)i;
            if (pok[b + i] != 1 && bad_p < 0) bad_p = (int)i;
            for (size_t j = 0; j < limits[b + i].size(); j++) bparts.push_back(&limits[b + i][j]);
            pparts.push_back(&proj[b + i]);
        }
        bool same = true;
        for (int flag = 0; flag < 2; flag++) {
            StubMat want;
            int wok = 1;
            if (n == 0) want.clean();
            else if (bad_b >= 0) wok = bok[b + (size_t)bad_b];
            else wok = composed(bparts, cols, true, rhs[(size_t)g], flag != 0, want) ? 1 : 0;
            same = same && ok[flag][(size_t)g] == wok && mem[flag][(size_t)g] == bad_b && got[flag][(size_t)g].same(want);
            // the member function, through the list type and through the vector overload: one list per call
            StubList lst; lst.v = groups[(size_t)g];
            StubMat r1, r2;
            Lin lin(0);
            lin.ConvexHullUnionAndIntersect(r1, lst, (unsigned)rhs[(size_t)g], flag != 0);
            lin.ConvexHullUnionAndIntersect(r2, groups[(size_t)g], (unsigned)rhs[(size_t)g], flag != 0);
            same = same && r1.same(want) && r2.same(want);
        }
        {
            StubMat want;
            int wok = 1;
            if (n != 0 && bad_p >= 0) wok = pok[b + (size_t)bad_p];
            else if (n != 0) wok = composed(pparts, cols, false, rhs[(size_t)g], false, want) ? 1 : 0;
            same = same && uok[(size_t)g] == wok && umem[(size_t)g] == bad_p && uni[(size_t)g].same(want);
        }
        mismatches += same ? 0 : 1;
        printf("%d ok %d %d rows %u %u same %d\n", g, (int)ok[0][(size_t)g], (int)ok[1][(size_t)g], got[0][(size_t)g].rows, got[1][(size_t)g].rows, same ? 1 : 0);
        b += n;
    }
    printf("mismatches %d\n", mismatches);
    return mismatches ? 1 : 0;
}
