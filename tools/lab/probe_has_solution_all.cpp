// Times xpoly_amd::has_solution_all (include/xpoly_amd/lineq.hpp) on a SCoP-like mix of systems under one vc: the collector of
// whichever tree's headers and library it is compiled against -- this tree's makes ONE ragged call, its parent's one call per
// shape class. tools/lab/run_has_solution_ragged_ab.sh builds and runs it against both.
//   probe_has_solution_all LABEL [large|small]   (-DPROBE_RAGGED: the tree has xpg_has_solution_batch_ragged_last_route, print it)
// Two mixes (fixed seed), 20 shape classes of 8 + (37 k mod 57) systems each (692 in all), interleaved:
//   large  24 variables, the first two free; class k = 0..17 with 4 + 2k inequalities and, while the inequalities are no more
//          than the variables, k % 4 equalities; classes 18 and 19 with 150 and 170 inequalities, past 64 KB of LDS. Its longest
//          solves take seconds: the call lasts as long as they do.
//   small  10 variables, the first free; class k with 3 + k inequalities and, while those are no more than the variables, k % 3
//          equalities; every class LDS-resident. Solves of microseconds: what a call costs beside them shows.
// Every system holds at a point x >= 0 but one in five, whose constants are pulled down. Host arrays, is_int_sol = 0,
// is_unique_sol = 1; one warm-up call, then the median of 5.
// Prints one JSON line: the call times, the verdict counts and an FNV-1a hash of the verdicts in the order given.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <map>
#include <vector>
#include "xpoly_amd/lineq.hpp"

struct StubMat {
    unsigned rows, cols;
    std::vector<xpg_rat32> cells;
    StubMat() : rows(0), cols(0) {}
    unsigned get_row_size() const { return rows; }
    unsigned get_col_size() const { return cols; }
    const xpg_rat32 * get_matrix() const { return cells.data(); }
    void set(unsigned r, unsigned c, const std::vector<int> & v)
    {
        rows = r; cols = c; cells.resize((size_t)r * c);
        for (size_t k = 0; k < cells.size(); k++) { cells[k].num = v[k]; cells[k].den = 1; }
    }
};

static unsigned long long g_state = 20261019ull;
static int draw(int lo, int hi)                                  // uniform in [lo, hi]
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return lo + (int)((g_state >> 33) % (unsigned long long)(hi - lo + 1));
}

int main(int argc, char ** argv)
{
    const char * label = argc > 1 ? argv[1] : "has_solution_all";
    const bool small = argc > 2 && argv[2][0] == 's';
    const int nv = small ? 10 : 24, nfree = small ? 1 : 2, cols = nv + 1, classes = 20;
    std::vector<int> vcv((size_t)nv * cols, 0);
    for (int i = nfree; i < nv; i++) vcv[(size_t)i * cols + i] = -1;
    StubMat vc;
    vc.set(nv, cols, vcv);
    int lr[classes], er[classes], cnt[classes], most = 0, total = 0;
    for (int k = 0; k < classes; k++) {
        lr[k] = small ? 3 + k : (k < 18 ? 4 + 2 * k : 150 + 20 * (k - 18));
        er[k] = lr[k] <= nv ? k % (small ? 3 : 4) : 0;
        cnt[k] = 8 + (37 * k) % 57;
        most = std::max(most, cnt[k]); total += cnt[k];
    }
    std::vector<StubMat> leq((size_t)total), eq((size_t)total);
    std::vector<StubMat *> pl, pe;
    int at = 0;
    for (int i = 0; i < most; i++)
        for (int k = 0; k < classes; k++) {
            if (i >= cnt[k]) continue;
            std::vector<int> xs((size_t)nv), L((size_t)lr[k] * cols), E((size_t)er[k] * cols);
            for (int j = 0; j < nv; j++) xs[(size_t)j] = draw(0, 3);
            const int pull = at % 5 == 4 ? 40 : 0;
            for (int r = 0; r < lr[k]; r++) {
                int dot = 0;
                for (int j = 0; j < nv; j++) { const int a = draw(-3, 3); L[(size_t)r * cols + j] = a; dot += a * xs[(size_t)j]; }
                L[(size_t)r * cols + nv] = dot + draw(0, 3) - pull;
            }
            for (int r = 0; r < er[k]; r++) {
                int dot = 0;
                for (int j = 0; j < nv; j++) { const int a = draw(-2, 2); E[(size_t)r * cols + j] = a; dot += a * xs[(size_t)j]; }
                E[(size_t)r * cols + nv] = dot;
            }
            leq[(size_t)at].set((unsigned)lr[k], (unsigned)cols, L);
            eq[(size_t)at].set((unsigned)er[k], (unsigned)cols, E);
            pl.push_back(&leq[(size_t)at]);
            pe.push_back(er[k] ? &eq[(size_t)at] : (StubMat *)0);
            at++;
        }
    std::vector<int32_t> out;
    std::vector<double> ms;
    for (int rep = 0; rep < 6; rep++) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = xpoly_amd::has_solution_all(pl, pe, vc, nv, false, true, out);
        const auto t1 = std::chrono::steady_clock::now();
        if (rc != 0) { printf("{\"label\": \"%s\", \"rc\": %d}\n", label, rc); return 1; }
        if (rep > 0) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::vector<double> sorted = ms;
    std::sort(sorted.begin(), sorted.end());
    unsigned long long h = 1469598103934665603ull;
    std::map<int, int> hist;
    for (int32_t v : out) { h = (h ^ (unsigned long long)(unsigned)v) * 1099511628211ull; hist[(int)v]++; }
    printf("{\"label\": \"%s\", \"mix\": \"%s\", \"systems\": %d, \"classes\": %d, \"median_ms\": %.3f, \"call_ms\": [", label, small ? "small" : "large", total, classes, sorted[2]);
    for (size_t k = 0; k < ms.size(); k++) printf("%s%.3f", k ? ", " : "", ms[k]);
    printf("], \"verdicts\": {");
    bool first = true;
    for (const auto & kv : hist) { printf("%s\"%d\": %d", first ? "" : ", ", kv.first, kv.second); first = false; }
    printf("}, \"verdict_hash\": \"%016llx\"", h);
#ifdef PROBE_RAGGED
    long long route[7] = {0, 0, 0, 0, 0, 0, 0};
    xpg_has_solution_batch_ragged_last_route(route, 7);
    printf(", \"route\": {\"lds\": %lld, \"hbm\": %lld, \"host\": %lld, \"second\": %lld, \"grid_lds\": %lld, \"grid_hbm\": %lld, \"no_solve\": %lld}",
           route[0], route[1], route[2], route[3], route[4], route[5], route[6]);
#endif
    printf("}\n");
    return 0;
}
