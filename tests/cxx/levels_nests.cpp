// xpoly_amd::levels_nests and xpoly_amd::project_each (include/xpoly_amd/lineq.hpp) on loop nests of several DEPTHS and row
// classes in ONE call each, checked in here against the loop they replace -- loop-bound generation,
// LoopTran::transformIterSpace (src/eng/ldtran.cpp:178-196):
//     for (i = rhs - 1; i > 0; i--) { lineq.fme(i, res); *A = res; }
// run with the adapter's own Lineq::fme, one system and one step per call. The stub matrix type offers what the adapter
// relies on alone.
// Reads integer systems from the file named by argv[1]:
//   count, then per system: rhs_idx rows cols, then rows x cols integers
// To these it adds an empty system and a nest of depth 1, which the collectors answer without a call. ALL of them go through
// one levels_nests call; those with something to eliminate through one project_each call with the same lists, whose result is
// the last level. Prints "levels rc <code> launches <n>", "project rc <code> launches <n>" (the route of the last ragged
// call), per system "<k> nv <rhs_idx> rows <rows> ok <ok> lev <0|1> proj <0|1>" (lev: every level equals the loop's; proj: the
// projection equals the loop's last system) and "mismatches <n>". Exit status 0 iff both rc == 0 and nothing differs.
// tests/test_lineq_ragged_host.py compiles and links it, tests/test_gpu_lineq_ragged.py runs it.
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

static bool same_mat(const StubMat & a, const StubMat & b)
{
    if (a.size() == 0 || b.size() == 0) return a.size() == 0 && b.size() == 0;
    return a.rows == b.rows && a.cols == b.cols && std::memcmp((const void *)a.get_matrix(), (const void *)b.get_matrix(), sizeof(xpg_rat32) * a.size()) == 0;
}

// the reference's loop: want[step] the system after step `step`; false where a step is inconsistent (the reference ASSERTs)
static bool loop_of_the_reference(const StubMat & sys, int rhs, std::vector<StubMat> & want)
{
    want.assign((size_t)(rhs - 1), StubMat());
    StubMat A = sys;
    for (int i = rhs - 1; i > 0; i--) {
        xpoly_amd::Lineq<StubMat> lineq(&A, rhs);
        StubMat res;
        if (!lineq.fme((unsigned)i, res, false)) return false;
        A = res;
        want[(size_t)(rhs - 1 - i)] = A;
    }
    return true;
}

static long long launches_of_the_last_call()
{
    long long r[1] = {-1};
    return xpg_lineq_ragged_last_route(r, 1) == 0 ? r[0] : -1;
}

int main(int argc, char ** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: levels_nests FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int count;
    if (fscanf(f, "%d", &count) != 1 || count < 1) return 2;
    std::vector<StubMat> sys((size_t)count + 2);
    std::vector<int32_t> rhs((size_t)count + 2);
    for (int k = 0; k < count; k++) {
        int nv, r, c;
        if (fscanf(f, "%d %d %d", &nv, &r, &c) != 3 || nv < 1 || r < 0 || c < 0 || !sys[(size_t)k].read(f, (unsigned)r, (unsigned)c)) return 2;
        rhs[(size_t)k] = nv;
    }
    fclose(f);
    rhs[(size_t)count] = 3;                                          // an empty system: it stays empty, no call
    sys[(size_t)count + 1].reinit(2, 2);                             // a nest of depth 1: nothing to eliminate
    for (int k = 0; k < 4; k++) { sys[(size_t)count + 1].cells[(size_t)k].num = k % 2 ? 5 : 1; sys[(size_t)count + 1].cells[(size_t)k].den = 1; }
    rhs[(size_t)count + 1] = 1;
    const int total = count + 2;
    std::vector<StubMat *> ps;
    for (int k = 0; k < total; k++) ps.push_back(&sys[(size_t)k]);

    std::vector<std::vector<StubMat> > levels;
    std::vector<int32_t> ok;
    const int rc_l = xpoly_amd::levels_nests(ps, rhs, levels, ok);
    printf("levels rc %d launches %lld\n", rc_l, launches_of_the_last_call());

    std::vector<StubMat *> pp;                                       // the projections: every nest with something to eliminate
    std::vector<std::vector<int32_t> > lists;
    std::vector<int32_t> prhs;
    std::vector<int> at((size_t)total, -1);
    for (int k = 0; k < total; k++) {
        if (rhs[(size_t)k] < 2) continue;
        at[(size_t)k] = (int)pp.size();
        pp.push_back(ps[(size_t)k]); prhs.push_back(rhs[(size_t)k]);
        std::vector<int32_t> el;
        for (int u = rhs[(size_t)k] - 1; u > 0; u--) el.push_back(u);
        lists.push_back(el);
    }
    std::vector<StubMat> proj;
    std::vector<int32_t> pok;
    const int rc_p = xpoly_amd::project_each(pp, lists, prhs, proj, pok);
    printf("project rc %d launches %lld\n", rc_p, launches_of_the_last_call());
    if (rc_l != 0 || rc_p != 0) return 1;

    int mismatches = 0;
    for (int k = 0; k < total; k++) {
        const int nv = rhs[(size_t)k];
        std::vector<StubMat> want;
        const bool good = sys[(size_t)k].size() == 0 ? (want.assign((size_t)(nv - 1), StubMat()), true) : loop_of_the_reference(sys[(size_t)k], nv, want);
        bool lev = (ok[(size_t)k] == 1) == good && (int)levels[(size_t)k].size() == nv - 1;
        for (int s = 0; lev && s < nv - 1; s++)
            lev = good ? same_mat(levels[(size_t)k][(size_t)s], want[(size_t)s]) : levels[(size_t)k][(size_t)s].size() == 0;
        bool pr = true;
        if (at[(size_t)k] >= 0) {
            const size_t i = (size_t)at[(size_t)k];
            pr = (pok[i] == 1) == good && (good ? same_mat(proj[i], want[(size_t)(nv - 2)]) : proj[i].size() == 0);
        }
        mismatches += (lev ? 0 : 1) + (pr ? 0 : 1);
        printf("%d nv %d rows %u ok %d lev %d proj %d\n", k, nv, sys[(size_t)k].rows, (int)ok[(size_t)k], lev ? 1 : 0, pr ? 1 : 0);
    }
    printf("mismatches %d\n", mismatches);
    return mismatches ? 1 : 0;
}
