// xpoly_amd::levels_all and Lineq::fmeLevels (include/xpoly_amd/lineq.hpp) on loop nests of several depths, each depth with
// systems of several shape classes interleaved, checked in here against the loop they replace -- loop-bound generation,
// LoopTran::transformIterSpace (src/eng/ldtran.cpp:178-196):
//     newb = aux_limits.get_tail();
//     for (i = rhs - 1; i > 0; i--) { *newb = *A; lineq.fme(i, res); *A = res; newb = aux_limits.get_prev(); }
//     *newb = *A;
// run with the adapter's own Lineq::fme. The stub matrix and list types offer what the adapter relies on alone.
// Reads integer systems from the file named by argv[1]:
//   groups
//   per group: rhs_idx count, then per system: rows cols, then rows x cols integers
// A group is one levels_all call with elim = rhs_idx-1 .. 1; then every system of it goes through fmeLevels on a StubList
// and, the first of the group, on a std::vector too. Prints per group "group <g> rc <code>", per system
// "<g> <k> ok <ok> all <0|1> list <0|1>" (all: levels_all's entries equal the loop's; list: fmeLevels' list and *A do), and
// at the end "mismatches <n>". Exit status 0 iff every rc == 0 and nothing differs. tests/test_lineq_levels_host.py compiles
// and links it, tests/test_gpu_lineq_levels.py runs it.
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
// The part of the reference's List<RMat*> the loop uses: a cursor that get_tail() puts on the last element and get_prev()
// moves towards the head (NULL past it).
struct StubList {
    std::vector<StubMat *> elems;
    long cur;
    StubList() : cur(-1) {}
    unsigned get_elem_count() const { return (unsigned)elems.size(); }
    StubMat * get_tail() { cur = (long)elems.size() - 1; return cur >= 0 ? elems[(size_t)cur] : 0; }
    StubMat * get_prev() { if (cur >= 0) cur--; return cur >= 0 ? elems[(size_t)cur] : 0; }
};

static bool same_mat(const StubMat & a, const StubMat & b)
{
    if (a.size() == 0 || b.size() == 0) return a.size() == 0 && b.size() == 0;
    return a.rows == b.rows && a.cols == b.cols && std::memcmp((const void *)a.get_matrix(), (const void *)b.get_matrix(), sizeof(xpg_rat32) * a.size()) == 0;
}

// the reference's loop: want[0] the outermost bound (the head) .. want[rhs - 1] the system itself (the tail); false where a
// step is inconsistent (the reference ASSERTs)
static bool loop_of_the_reference(const StubMat & sys, int rhs, std::vector<StubMat> & want, StubMat & a_after)
{
    want.assign((size_t)rhs, StubMat());
    StubMat A = sys;
    int at = rhs - 1;
    for (int i = rhs - 1; i > 0; i--) {
        want[(size_t)at] = A;
        xpoly_amd::Lineq<StubMat> lineq(&A, rhs);
        StubMat res;
        if (!lineq.fme((unsigned)i, res, false)) return false;
        A = res;
        at--;
    }
    want[(size_t)at] = A;
    a_after = A;
    return true;
}

int main(int argc, char ** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: levels_all FILE\n"); return 2; }
    FILE * f = fopen(argv[1], "r");
    if (!f) { perror(argv[1]); return 2; }
    int groups;
    if (fscanf(f, "%d", &groups) != 1 || groups < 1) return 2;
    int mismatches = 0, bad_rc = 0;
    for (int g = 0; g < groups; g++) {
        int rhs, count;
        if (fscanf(f, "%d %d", &rhs, &count) != 2 || rhs < 1 || count < 0) return 2;
        std::vector<StubMat> sys((size_t)count);
        std::vector<StubMat *> ps;
        for (int k = 0; k < count; k++) {
            int r, c;
            if (fscanf(f, "%d %d", &r, &c) != 2 || r < 0 || c < 0 || !sys[(size_t)k].read(f, (unsigned)r, (unsigned)c)) return 2;
            ps.push_back(&sys[(size_t)k]);
        }
        std::vector<int32_t> elim;
        for (int i = rhs - 1; i > 0; i--) elim.push_back(i);
        std::vector<std::vector<StubMat> > levels;
        std::vector<int32_t> ok;
        const int rc = xpoly_amd::levels_all(ps, elim, rhs, levels, ok);
        printf("group %d rc %d\n", g, rc);
        if (rc != 0) { bad_rc++; continue; }
        for (int k = 0; k < count; k++) {
            std::vector<StubMat> want;
            StubMat a_after;
            const bool good = loop_of_the_reference(sys[(size_t)k], rhs, want, a_after);
            // levels_all: levels[k][step] is want[rhs - 2 - step]
            bool all = (ok[(size_t)k] == 1) == good && (int)levels[(size_t)k].size() == rhs - 1;
            for (int s = 0; all && s < rhs - 1; s++)
                all = good ? same_mat(levels[(size_t)k][(size_t)s], want[(size_t)(rhs - 2 - s)]) : levels[(size_t)k][(size_t)s].size() == 0;
            // fmeLevels on a list: the caller's matrices, marked so that an entry left alone shows
            std::vector<StubMat> store((size_t)rhs);
            StubList lst;
            for (int j = 0; j < rhs; j++) { store[(size_t)j].reinit(1, 1); store[(size_t)j].cells[0].num = -77; lst.elems.push_back(&store[(size_t)j]); }
            StubMat A = sys[(size_t)k];
            xpoly_amd::Lineq<StubMat> lineq(&A, rhs);
            const bool got = lineq.fmeLevels(lst, &A);
            bool list = got == good;
            for (int j = 0; list && j < rhs; j++)
                list = good ? same_mat(store[(size_t)j], want[(size_t)j])
                            : (store[(size_t)j].size() == 1 && store[(size_t)j].cells[0].num == -77);     // left as it was
            if (list) list = same_mat(A, good ? a_after : sys[(size_t)k]);
            if (list && k == 0) {                                    // the vector form, and a list of the wrong length
                std::vector<StubMat> vec;
                xpoly_amd::Lineq<StubMat> lv(&sys[(size_t)k], rhs);
                list = lv.fmeLevels(vec) == good;
                for (int j = 0; list && good && j < rhs; j++) list = (int)vec.size() == rhs && same_mat(vec[(size_t)j], want[(size_t)j]);
                StubList shorter;
                for (int j = 0; j + 1 < rhs; j++) shorter.elems.push_back(&store[(size_t)j]);
                if (lv.fmeLevels(shorter)) list = false;
            }
            mismatches += (all ? 0 : 1) + (list ? 0 : 1);
            printf("%d %d ok %d all %d list %d\n", g, k, (int)ok[(size_t)k], all ? 1 : 0, list ? 1 : 0);
        }
    }
    fclose(f);
    printf("mismatches %d\n", mismatches);
    return mismatches || bad_rc ? 1 : 0;
}
