// xpoly_amd::has_solution_all (include/xpoly_amd/lineq.hpp) on systems of three or more shape classes: ONE ragged call of the
// library. The stub matrix type offers what the collector relies on alone: get_row_size(), get_col_size(), get_matrix().
// Reads integer systems from the file named by argv[1], in the format of tests/cxx/has_solution_all.cpp:
//   rhs_idx is_int_sol is_unique_sol count
//   vc: rhs_idx x (rhs_idx + 1) integers
//   per system: leq_rows eq_rows, then leq_rows x cols and eq_rows x cols integers
// and prints "rc <code>", "route" with the seven entries of xpg_has_solution_batch_ragged_last_route, and one verdict per line
// in the order given. tests/test_has_solution_ragged_host.py compiles and links it, tests/test_gpu_has_solution_ragged.py runs it.
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
    if (argc < 2) { fprintf(stderr, "usage: has_solution_ragged FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int rhs, is_int, is_unique, count;
    if (fscanf(f, "%d %d %d %d", &rhs, &is_int, &is_unique, &count) != 4 || rhs < 1 || count < 0) return 2;
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
    const int rc = xpoly_amd::has_solution_all(pl, pe, vc, rhs, is_int != 0, is_unique != 0, out);
    printf("rc %d\n", rc);
    if (rc != 0) return 1;
    long long route[7] = {0, 0, 0, 0, 0, 0, 0};
    if (xpg_has_solution_batch_ragged_last_route(route, 7) != 0) return 1;
    printf("route");
    for (int k = 0; k < 7; k++) printf(" %lld", route[k]);
    printf("\n");
    for (int k = 0; k < count; k++) printf("%d\n", (int)out[(size_t)k]);
    return 0;
}
