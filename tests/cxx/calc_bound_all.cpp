// xpoly_amd::calc_bound_all (include/xpoly_amd/lineq.hpp) on systems of three or more shape classes, checked in here against
// the call it collects: Lineq::calcBound of the adapter on the single system (linsys.cpp:1047-1078; the callers are
// src/eng/ldtran.cpp:178-193 and :241-254, one call per loop nest). The stub matrix type offers what the collector and the
// adapter's calcBound rely on alone.
// Reads integer systems from the file named by argv[1]:
//   count
//   per system: rows cols rhs_idx, then rows x cols integers
// and prints "rc <code>", one line "<k> ok <ok> rows <rows of all its bounds> same <0|1>" per system in the order given, and
// "mismatches <n>". Exit status 0 iff rc == 0 and nothing differs. tests/test_lineq_bounds_host.py compiles and links it,
// tests/test_gpu_lineq_bounds.py runs it.
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
            int x;
            if (fscanf(f, "%d", &x) != 1) return false;
            cells[k].num = x; cells[k].den = 1;
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
    if (argc < 2) { fprintf(stderr, "usage: calc_bound_all FILE\n"); return 2; }
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
    std::vector<std::vector<StubMat> > limits;
    std::vector<int32_t> ok;
    const int rc = xpoly_amd::calc_bound_all(ps, rhs, limits, ok);
    printf("rc %d\n", rc);
    if (rc != 0) return 1;
    int mismatches = 0;
    for (int k = 0; k < count; k++) {
        StubMat one = sys[(size_t)k];
        xpoly_amd::Lineq<StubMat> lin(&one, rhs[(size_t)k]);
        std::vector<StubMat> want;
        const bool good = lin.calcBound(want);
        const std::vector<StubMat> & got = limits[(size_t)k];
        bool same = (ok[(size_t)k] == 1) == good && (int)got.size() == rhs[(size_t)k];
        unsigned total = 0;
        for (size_t j = 0; same && j < got.size(); j++) {
            total += got[j].rows;
            same = good ? got[j].same(want[j]) : got[j].size() == 0;
        }
        mismatches += same ? 0 : 1;
        printf("%d ok %d rows %u same %d\n", k, (int)ok[(size_t)k], total, same ? 1 : 0);
    }
    printf("mismatches %d\n", mismatches);
    return mismatches ? 1 : 0;
}
