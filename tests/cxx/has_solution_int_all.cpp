// xpoly_amd::has_solution_all (include/xpoly_amd/lineq.hpp) with is_int_sol = true on a stub matrix type that offers what the
// collector relies on alone: get_row_size(), get_col_size(), get_matrix(). Reads integer systems from the file named by argv[1]:
//   rhs_idx is_unique_sol count
//   vc: rhs_idx x (rhs_idx + 1) integers
//   per system: leq_rows eq_rows, then leq_rows x cols and eq_rows x cols integers
// and prints "rc <code>", "route <lds> <hbm> <host> <second>" as xpg_has_solution_int_batch_last_route reports the call, and one
// verdict per line, in the order given (the systems may mix shapes: the library forms the shape classes).
// tests/test_has_solution_int_host.py compiles and links it, tests/test_gpu_has_solution_int.py runs it.
#include <cstdio>
#include <vector>
#include "xpoly_amd/lineq.hpp"

struct StubMat {
    unsigned rows, cols;
    std::vector<xpg_rat32> cells;
    StubMat() : rows(0), cols(0) {}
    unsigned get_row_size() const { return rows; }
    unsigned get_col_size() const { return cols; }
    const xpg_rat32 * get_matrix() const { return cells.data(); }
    bool read(FILE * f, unsigned r, unsigned c)
    {
        rows = r; cols = c; cells.resize((size_t)r * c);
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
    if (argc < 2) { fprintf(stderr, "usage: has_solution_int_all FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int rhs, is_unique, count;
    if (fscanf(f, "%d %d %d", &rhs, &is_unique, &count) != 3 || rhs < 1 || count < 0) return 2;
    StubMat vc;
    if (!vc.read(f, (unsigned)rhs, (unsigned)rhs + 1)) return 2;
    std::vector<StubMat> leq((size_t)count), eq((size_t)count);
    std::vector<StubMat *> pl, pe;
    for (int k = 0; k < count; k++) {
        int lr, er;
        if (fscanf(f, "%d %d", &lr, &er) != 2 || lr < 0 || er < 0) return 2;
        if (!leq[(size_t)k].read(f, (unsigned)lr, (unsigned)rhs + 1) || !eq[(size_t)k].read(f, (unsigned)er, (unsigned)rhs + 1)) return 2;
        pl.push_back(&leq[(size_t)k]);
        pe.push_back(er ? &eq[(size_t)k] : (StubMat *)0);        // a system without equalities hands none over
    }
    fclose(f);
    std::vector<int32_t> out;
    const int rc = xpoly_amd::has_solution_all(pl, pe, vc, rhs, true, is_unique != 0, out);
    printf("rc %d\n", rc);
    if (rc != 0) return 1;
    long long route[4] = {-1, -1, -1, -1};
    if (xpg_has_solution_int_batch_last_route(route, 4) != 0) return 1;
    printf("route %lld %lld %lld %lld\n", route[0], route[1], route[2], route[3]);
    for (int k = 0; k < count; k++) printf("%d\n", (int)out[(size_t)k]);
    return 0;
}
