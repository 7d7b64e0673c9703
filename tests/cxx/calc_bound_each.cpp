// xpoly_amd::calc_bound_each (include/xpoly_amd/lineq.hpp) on loop nests of several DEPTHS and row counts, checked in here
// against xpoly_amd::calc_bound_all on the same systems: the same limits and the same ok, system for system, from ONE
// xpg_lineq_bounds_batch_ragged_rat32 call over the whole mix instead of one call per shape class. The stub matrix type offers
// what the two collectors rely on alone.
// Reads rational systems from the file named by argv[1]:
//   count
//   per system: rows cols rhs_idx, then rows x cols cells, numerator and denominator each
// and prints "rc <each> <all>", "route <launches> <grid> <steps>" (xpg_lineq_bounds_ragged_last_route after calc_bound_each:
// what its LAST library call did), one line "<k> ok <ok> rows <rows of all its bounds> same <0|1>" per system in the order
// given, and "mismatches <n>". Exit status 0 iff both return 0 and nothing differs. tests/test_lineq_bounds_ragged_host.py
// compiles and links it, tests/test_gpu_lineq_bounds_ragged.py runs it.
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
    void reinit(unsigned r, unsigned c) { rows = r; cols = c; cells.assign((size_t)r * c, xpg_rat32()); }
    void clean() { rows = 0; cols = 0; cells.clear(); }
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

int main(int argc, char ** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: calc_bound_each FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int count;
    if (fscanf(f, "%d", &count) != 1 || count < 0) return 2;
    std::vector<StubMat> sys((size_t)count);
    std::vector<StubMat *> ps;
    std::vector<int32_t> rhs((size_t)count);
    for (int k = 0; k < count; k++) {
        int r, c, h;
        if (fscanf(f, "%d %d %d", &r, &c, &h) != 3 || r < 0 || c < 0 || !sys[(size_t)k].read(f, (unsigned)r, (unsigned)c)) return 2;
        ps.push_back(&sys[(size_t)k]);
        rhs[(size_t)k] = h;
    }
    fclose(f);
    std::vector<std::vector<StubMat> > each, all;
    std::vector<int32_t> ok_each, ok_all;
    const int rc_each = xpoly_amd::calc_bound_each(ps, rhs, each, ok_each);
    long long route[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    xpg_lineq_bounds_ragged_last_route(route, 8);
    const int rc_all = xpoly_amd::calc_bound_all(ps, rhs, all, ok_all);
    printf("rc %d %d\n", rc_each, rc_all);
    printf("route %lld %lld %lld\n", route[0], route[1], route[7]);
    if (rc_each != 0 || rc_all != 0) return 1;
    int mismatches = 0;
    for (int k = 0; k < count; k++) {
        const std::vector<StubMat> & got = each[(size_t)k], & want = all[(size_t)k];
        bool same = ok_each[(size_t)k] == ok_all[(size_t)k] && (int)got.size() == rhs[(size_t)k] && got.size() == want.size();
        unsigned total = 0;
        for (size_t j = 0; same && j < got.size(); j++) {
            total += got[j].rows;
            same = got[j].same(want[j]) && (ok_each[(size_t)k] == 1 || got[j].size() == 0);
        }
        mismatches += same ? 0 : 1;
        printf("%d ok %d rows %u same %d\n", k, (int)ok_each[(size_t)k], total, same ? 1 : 0);
    }
    printf("mismatches %d\n", mismatches);
    return mismatches ? 1 : 0;
}
