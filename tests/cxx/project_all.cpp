// xpoly_amd::project_all (include/xpoly_amd/lineq.hpp) on systems of three or more shape classes, checked in here against the
// loop it replaces: Lineq::fme(u, res) of the adapter, variable after variable, per system (DepPoly::eliminateAuxVar's loop,
// src/eng/poly.cpp:643-651). The stub matrix type offers what the collector and the adapter's fme rely on alone.
// Reads integer systems from the file named by argv[1]:
//   rhs_idx n_elim count
//   n_elim indices
//   per system: rows cols, then rows x cols integers
// and prints "rc <code>", "calls <projection calls that launched, counted through xpg_lineq_project_last_route: 1 or 0>", one
// line "<k> ok <ok> rows <rows> same <0|1>" per system in the order given, and "mismatches <n>". Exit status 0 iff rc == 0
// and nothing differs. tests/test_lineq_project_host.py compiles and links it, tests/test_gpu_lineq_project.py runs it.
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
};

int main(int argc, char ** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: project_all FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int rhs, n_elim, count;
    if (fscanf(f, "%d %d %d", &rhs, &n_elim, &count) != 3 || rhs < 1 || n_elim < 1 || count < 0) return 2;
    std::vector<int32_t> elim((size_t)n_elim);
    for (int k = 0; k < n_elim; k++) { int u; if (fscanf(f, "%d", &u) != 1) return 2; elim[(size_t)k] = u; }
    std::vector<StubMat> sys((size_t)count);
    std::vector<StubMat *> ps;
    for (int k = 0; k < count; k++) {
        int r, c;
        if (fscanf(f, "%d %d", &r, &c) != 2 || r < 0 || c < 0 || !sys[(size_t)k].read(f, (unsigned)r, (unsigned)c)) return 2;
        ps.push_back(&sys[(size_t)k]);
    }
    fclose(f);
    std::vector<StubMat> results;
    std::vector<int32_t> ok;
    const int rc = xpoly_amd::project_all(ps, elim, rhs, results, ok);
    printf("rc %d\n", rc);
    if (rc != 0) return 1;
    long long route[6] = {0, 0, 0, 0, 0, 0};
    if (xpg_lineq_project_last_route(route, 6) != 0) return 1;
    printf("calls %lld\n", route[0]);
    int mismatches = 0;
    for (int k = 0; k < count; k++) {
        StubMat cur = sys[(size_t)k];
        bool good = true;
        for (int e = 0; e < n_elim && good; e++) {
            xpoly_amd::Lineq<StubMat> lin(&cur, rhs);
            StubMat next;
            good = lin.fme((unsigned)elim[(size_t)e], next);
            cur = next;
        }
        const StubMat & got = results[(size_t)k];
        bool same = (ok[(size_t)k] == 1) == good;
        if (same && good) {
            same = got.size() == cur.size() && (got.size() == 0 || (got.rows == cur.rows && got.cols == cur.cols &&
                   std::memcmp((const void *)got.get_matrix(), (const void *)cur.get_matrix(), sizeof(xpg_rat32) * got.size()) == 0));
        } else if (same) {
            same = got.size() == 0;
        }
        mismatches += same ? 0 : 1;
        printf("%d ok %d rows %u same %d\n", k, (int)ok[(size_t)k], got.rows, same ? 1 : 0);
    }
    printf("mismatches %d\n", mismatches);
    return mismatches ? 1 : 0;
}
