// Host controller of xpoly's branch-and-bound MIP<Mat,T> (src/com/lpsol.h:2087-2702);
// Lineq::has_solution (src/com/linsys.cpp:830-906) and the DepPoly::is_empty front end
// (src/eng/poly.cpp:530-573) on top of it are in mip_front.hip.h.
//
// The tree walk is the reference's depth-first recursion -- its results depend on DFS order
// through the shared fork_count row and the incumbent (lpsol.h:2474-2497) -- written as an
// explicit stack machine per problem so that MANY problems advance in lock step: in every
// round each unfinished problem contributes the LP relaxation of its current node, nodes of
// equal shape are solved by ONE launch of the LDS-resident batch kernel, and the host feeds
// the answers back into the stack machines. A node is a from-scratch SIX solve with
// max_iter = 10000 (lpsol.h:2441), exactly as in the reference.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <stdio.h>
#include <stdlib.h>
#include <thread>
#include <vector>
#include "six_host.hip.h"
#include "lineq_shared.hip.h"
#include "mip_kernels.hip.h"

namespace xpg {

template <class S> struct MipProblem {
    int cols;
    std::vector<S> tgtf, vc, eq, leq;      // flat row-major; vc has cols-1 rows
    int eq_rows, leq_rows;
};

template <class S>
MipProblem<S> make_problem(const S * tgtf, const S * vc, int vc_rows, const S * eqs, int eq_rows, const S * leq,
                           int leq_rows, int cols)
{
    MipProblem<S> Q;
    Q.cols = cols; Q.eq_rows = eq_rows; Q.leq_rows = leq_rows;
    Q.tgtf.assign(tgtf, tgtf + cols);
    Q.vc.assign(vc, vc + (size_t)vc_rows * cols);
    if (eq_rows) Q.eq.assign(eqs, eqs + (size_t)eq_rows * cols);
    if (leq_rows) Q.leq.assign(leq, leq + (size_t)leq_rows * cols);
    return Q;
}

inline bool int_cast_ok(F64) { return true; }
inline bool int_cast_ok(R32 a) { return a.den != 0; }

// One problem's MIP::RecusivePart (lpsol.h:2427-2612) as a resumable stack machine.
template <class S> struct MipTask {
    struct Frame {
        MipProblem<S> Q;
        int stage;                          // 0: LP pending, 1: floor child running, 2: ceiling child running
        int col, lo, hi;
        bool kept; S kept_v; std::vector<S> kept_sol;
    };
    bool is_max, is_bin;
    const uint8_t * allow_rational;         // 1 x cols or null (lpsol.h:2369-2393)
    int rhs0;
    // the by-reference state the reference threads through its recursion
    S v; std::vector<S> sol;
    bool have_best; S best_v; std::vector<S> best_sol;
    std::vector<int> forks;
    std::vector<Frame> stack;
    NormalForm<S> F;                        // normal form of the pending node LP
    bool done; int final_status; long nodes;

    void start(const MipProblem<S> & root, bool mx, bool bin, const uint8_t * allow)
    {
        is_max = mx; is_bin = bin; allow_rational = allow; rhs0 = root.cols - 1;
        v = zero<S>(); sol.clear(); have_best = false; best_v = zero<S>(); best_sol.clear();
        forks.assign(root.cols, 0);
        stack.clear(); done = false; final_status = 0; nodes = 0;
        push(root);
    }
    void push(const MipProblem<S> & Q)
    {
        Frame f; f.Q = Q; f.stage = 0; f.col = 0; f.lo = 0; f.hi = 1; f.kept = false; f.kept_v = zero<S>();
        stack.push_back(f);
    }
    // Normalises the pending node; a negative return is the LP's "status" (shape / undefined).
    int prepare()
    {
        const MipProblem<S> & Q = stack.back().Q;
        nodes++;
        return normalize_host(Q.tgtf.data(), Q.vc.data(), Q.cols - 1, Q.eq_rows ? Q.eq.data() : (const S *)0, Q.eq_rows,
                              Q.leq_rows ? Q.leq.data() : (const S *)0, Q.leq_rows, Q.cols, F);
    }

    // MIP::is_satisfying (lpsol.h:2364-2408); `col` is the first offending entry.
    bool satisfied(std::vector<S> & s, int & col) const
    {
        for (size_t j = 0; j < s.size(); j++) {
            if (allow_rational || is_bin) reduce(s[j]);
            if (allow_rational) {
                if (allow_rational[j]) continue;
                if (!is_int(s[j])) { col = (int)j; return false; }
                if (is_bin && ne(s[j], zero<S>()) && ne(s[j], one<S>())) { col = (int)j; return false; }
            } else if (is_bin) {
                if (ne(s[j], zero<S>()) && ne(s[j], one<S>())) { col = (int)j; return false; }
            } else if (!is_int(s[j])) { col = (int)j; return false; }     // {R,Float}Mat::is_imat
        }
        return true;
    }
    void remember()
    {
        if (!have_best || (is_max ? lt(best_v, v) : gt(best_v, v))) { best_sol = sol; best_v = v; have_best = true; }
    }
    static void add_row(std::vector<S> & rows, int & nrows, int cols, int col, S coef, int rhs, S b)
    {
        rows.resize((size_t)(nrows + 1) * cols, zero<S>());
        for (int j = 0; j < cols; j++) rows[(size_t)nrows * cols + j] = zero<S>();
        rows[(size_t)nrows * cols + col] = coef;
        rows[(size_t)nrows * cols + rhs] = b;
        nrows++;
    }
    // The child of frame `pi`: its problem plus one bound row. Built in place at the top of the stack -- ONE copy of
    // the parent's problem (by index: the emplace may move the frames).
    void push_branch(size_t pi, bool ceiling)
    {
        stack.emplace_back();
        const Frame & p = stack[pi];
        Frame & c = stack.back();
        c.stage = 0; c.col = 0; c.lo = 0; c.hi = 1; c.kept = false; c.kept_v = zero<S>();
        c.Q = p.Q;
        MipProblem<S> & B = c.Q;
        if (is_bin) add_row(B.eq, B.eq_rows, B.cols, p.col, one<S>(), rhs0, S::from_int(ceiling ? p.hi : p.lo));   // lpsol.h:2506-2512, :2548-2553
        else if (!ceiling) add_row(B.leq, B.leq_rows, B.cols, p.col, one<S>(), rhs0, S::from_int(p.lo));          // :2514-2520
        else add_row(B.leq, B.leq_rows, B.cols, p.col, minus_one<S>(), rhs0, S::from_int(-p.hi));                  // :2555-2559
    }

    // Feeds the answer of the pending LP (st: SIX status or a negative error; y: raw values of
    // the normalised variables on success) and runs until the next LP is needed or the tree ends.
    void on_lp(int st, const std::vector<S> & y)
    {
        int ret;
        {
            Frame & f = stack.back();
            v = zero<S>();
            if (st == XPG_SIX_SUCC) {
                std::vector<S> s(f.Q.cols);
                finish_host(F, f.Q.tgtf.data(), y, &v, s.data());
                sol = s;
            }
            if (st < 0) ret = st;
            else if (st == XPG_SIX_UNBOUND) ret = XPG_IP_UNBOUND;
            else if (st == XPG_SIX_TIME_OUT) ret = XPG_ERR_REF_UNDEFINED;     // UNREACH() in the reference
            else if (st != XPG_SIX_SUCC) ret = XPG_IP_NO_PRI_FEASIBLE_SOL;
            else {
                int col = 0;
                if (satisfied(sol, col)) ret = XPG_IP_SUCC;
                else if (have_best && (is_max ? le(v, best_v) : ge(v, best_v))) ret = XPG_IP_NO_BETTER_THAN_BEST_SOL;
                else if (forks[col] >= 1) ret = XPG_IP_NO_PRI_FEASIBLE_SOL;                  // lpsol.h:2486-2496
                else if (!is_bin && !int_cast_ok(sol[col])) ret = XPG_ERR_REF_UNDEFINED;
                else {
                    forks[col]++;
                    f.col = col; f.lo = 0; f.hi = 1;
                    if (!is_bin) { f.lo = to_int(sol[col]); f.hi = f.lo + 1; }
                    f.stage = 1;
                    push_branch(stack.size() - 1, false);
                    return;
                }
            }
        }
        for (;;) {                                      // hand `ret` to the callers up the stack
            stack.pop_back();
            if (stack.empty()) { final_status = ret; done = true; return; }
            Frame & p = stack.back();
            if (ret < 0) continue;
            if (p.stage == 1) {                         // floor branch came back, lpsol.h:2527-2543
                if (ret == XPG_IP_SUCC) { p.kept_sol = sol; p.kept_v = v; p.kept = true; remember(); }
                p.stage = 2;
                push_branch(stack.size() - 1, true);
                return;
            }
            if (ret == XPG_IP_SUCC) {                   // ceiling branch came back, lpsol.h:2563-2611
                if (p.kept && (is_max ? gt(p.kept_v, v) : lt(p.kept_v, v))) { v = p.kept_v; sol = p.kept_sol; }
                remember();
            } else if (p.kept) { v = p.kept_v; sol = p.kept_sol; remember(); ret = XPG_IP_SUCC; }
        }
    }
};

// The host half of a lock-step round -- normalising every tree's pending node (equality substitution, dual
// construction: O(rows x cols^2) exact operations each) and feeding the answers back into the stack machines --
// is independent per tree, and at a few nodes per tree it costs more than the node-batch launches (1024 knapsacks
// of 24 variables on one host thread: prepare 7.9 ms + feed-back 8.6 ms against 8 ms for 15 launches). A small pool
// of persistent host threads (XPG_HOST_THREADS; default 1, i.e. off) can take both loops with STATIC shares --
// worker w always gets the same slice of the index range, so a tree's heap blocks are allocated and freed by one
// thread and stay in one core's cache (handing out chunks dynamically made the loops SLOWER than one thread on a
// 256-core host: 12 + 18 ms) -- and the workers spin for a moment before they sleep: a round has three loops a
// fraction of a millisecond apart. Measured with 1 / 4 / 8 / 16 / 32 threads on one box: 37 / 48 / 38 / 43 / 36 k
// MIPs/s, on another 39 k with 1 and 30 k with 4: loops of half a millisecond do not pay for waking threads on a
// 256-core host reliably, so the default is the calling thread alone.
class MipPool {
    std::vector<std::thread> th_;
    std::mutex m_, run_m_;
    std::condition_variable cv_;
    std::function<void(int)> job_;                      // job_(w): the share of worker w, 0 <= w < size()
    std::atomic<unsigned> gen_{0};
    std::atomic<int> pending_{0};
    std::atomic<bool> stop_{false};
    static void relax() { __builtin_ia32_pause(); }
    void worker(int w)
    {
        unsigned seen = 0;
        for (;;) {
            for (int spin = 0; spin < 20000 && gen_.load(std::memory_order_acquire) == seen; spin++) relax();
            if (gen_.load(std::memory_order_acquire) == seen) {
                std::unique_lock<std::mutex> lk(m_);
                cv_.wait(lk, [&] { return stop_.load() || gen_.load(std::memory_order_acquire) != seen; });
            }
            if (stop_.load()) return;
            seen = gen_.load(std::memory_order_acquire);
            job_(w);
            pending_.fetch_sub(1, std::memory_order_acq_rel);
        }
    }
public:
    MipPool()
    {
        unsigned nt = 1;                                    // the calling thread alone unless XPG_HOST_THREADS says otherwise (see above)
        if (const char * e = xpg_env("XPG_HOST_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 64) nt = (unsigned)v; }
        for (unsigned w = 1; w < nt; w++) th_.emplace_back([this, w] { worker((int)w); });
    }
    ~MipPool()
    {
        { std::unique_lock<std::mutex> lk(m_); stop_.store(true); gen_.fetch_add(1, std::memory_order_release); }
        cv_.notify_all();
        for (auto & t : th_) t.join();
    }
    int size() const { return (int)th_.size() + 1; }
    // f(i) for every i of [0, n): worker w takes the w-th of size() contiguous slices; the caller is worker 0
    void run(size_t n, const std::function<void(size_t)> & f)
    {
        // one caller at a time: a second controller (the _multi entry points run one per device) keeps its loop to itself
        std::unique_lock<std::mutex> mine(run_m_, std::try_to_lock);
        if (n < 128 || th_.empty() || !mine.owns_lock()) { for (size_t i = 0; i < n; i++) f(i); return; }
        const int nt = size();
        std::function<void(int)> share = [&, n, nt](int w) {
            const size_t lo = n * (size_t)w / (size_t)nt, hi = n * (size_t)(w + 1) / (size_t)nt;
            for (size_t i = lo; i < hi; i++) f(i);
        };
        {
            std::unique_lock<std::mutex> lk(m_);
            job_ = share;
            pending_.store(nt - 1, std::memory_order_release);
            gen_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_all();
        share(0);
        while (pending_.load(std::memory_order_acquire) != 0) relax();
    }
};
inline MipPool & mip_pool() { static MipPool p; return p; }
template <class F> inline void mip_parallel_for(size_t n, F f) { mip_pool().run(n, std::function<void(size_t)>(f)); }

// Which route the trees of the calling thread's last MIP / has_solution / dep_is_empty call took (xpg_mip_last_route):
// answers are the same on both routes, so this is the only way to tell them apart. Reset by the C entry points that open with
// XPG_BIND_MIP, by nothing below them: has_solution's two walks add up.
struct MipRoute { long long device_trees, host_trees, free_vars; };
inline MipRoute & mip_route() { static thread_local MipRoute r = {0, 0, 0}; return r; }
// How a C entry point that resets them opens: the handle's device bound, the counters cleared.
#define XPG_BIND_MIP(ctx_) XPG_BIND(ctx_); xpg::mip_route() = xpg::MipRoute{0, 0, 0}

// Advances every task to completion; node LPs of equal shape share one kernel launch.
template <class S> int run_mip_tasks(xpg_ctx * ctx, int kind, std::vector<MipTask<S> > & tasks)
{
    mip_route().host_trees += (long long)tasks.size();
    struct Key { int is_max, rows, cols; bool operator<(const Key & o) const
        { return is_max != o.is_max ? is_max < o.is_max : (rows != o.rows ? rows < o.rows : cols < o.cols); } };
    const std::vector<S> none;
    static const bool dbg = xpg_hook("XPG_MIP_DEBUG") != 0;
    int rounds = 0, launches = 0; double t_prep = 0, t_gpu = 0, t_feed = 0;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    for (;;) {
        const double t0 = now();
        std::map<Key, std::vector<int> > groups;
        std::vector<int> large;
        bool any = false;
        mip_parallel_for(tasks.size(), [&](size_t t) {
            MipTask<S> & T = tasks[t];
            while (!T.done) {
                const int rc = T.prepare();
                if (rc == 0) break;
                T.on_lp(rc, none);                      // malformed / reference-undefined node: no GPU work
            }
        });
        for (size_t t = 0; t < tasks.size(); t++) {
            MipTask<S> & T = tasks[t];
            if (T.done) continue;
            any = true;
            if (T.F.fits_lds(T.is_max)) { Key k = { T.is_max ? 1 : 0, T.F.rows, T.F.n + 1 }; groups[k].push_back((int)t); }
            else large.push_back((int)t);
        }
        t_prep += now() - t0;
        if (!any) {
            if (dbg) fprintf(stderr, "xpoly_amd: MIP controller: %d rounds, %d node-batch launches; host prepare %.1f ms, batches %.1f ms, feed-back %.1f ms\n",
                             rounds, launches, t_prep, t_gpu, t_feed);
            return 0;
        }
        rounds++;
        for (typename std::map<Key, std::vector<int> >::iterator g = groups.begin(); g != groups.end(); ++g) {
            const Key & k = g->first;
            const std::vector<int> & ids = g->second;
            const int nb = (int)ids.size();
            // the round's node LPs are packed straight into the context's pinned staging and the answers are read
            // from it: one copy each way per launch (batch_staged, batch_kernels.hip.h)
            BatchStage<S> bs;
            int rc = batch_stage_prepare<S>(ctx, nb, k.rows, k.cols, bs);
            if (rc) return rc;
            mip_parallel_for((size_t)nb, [&](size_t b) {
                const NormalForm<S> & F = tasks[ids[b]].F;
                S * tg = bs.h_tgtf + b * k.cols;
                S * lq = bs.h_leq + b * (size_t)k.rows * k.cols;
                for (int j = 0; j < k.cols; j++) tg[j] = F.obj[j];
                for (size_t e = 0; e < (size_t)F.rows * (size_t)(F.n + 1); e++) lq[e] = F.Np[e];      // (its own cells, or a view of the node's inequalities: six_host.hip.h)
            });
            const double t1 = now();
            rc = batch_stage_run<S>(ctx, bs, k.is_max, 10000u, /*raw_sol=*/1);
            if (rc) return rc;
            launches++;
            const double t2 = now();
            t_gpu += t2 - t1;
            mip_parallel_for((size_t)nb, [&](size_t b) {
                const S * raw = bs.h_sol + b * k.cols;
                std::vector<S> y(raw, raw + (k.cols - 1));
                tasks[ids[b]].on_lp(bs.h_st[b], y);
            });
            t_feed += now() - t2;
        }
        for (size_t q = 0; q < large.size(); q++) {
            MipTask<S> & T = tasks[large[q]];
            std::vector<S> y;
            const int st = solve_large(ctx, kind, T.is_max, T.F, (const S *)0, (const S *)0, 10000u, y);
            T.on_lp(st, y);
        }
    }
}

// ---- The host half of the MIP entry points, each step stated once: the switch, the fit test, the route rule, the transfer
// object of a one-launch batch, the launcher of k_mip_tree, the device route, the controller's end and the front. ----------

// XPG_MIP_DEVICE=0 keeps every tree with the host controller (A/B runs). Read once per process, here alone: mip_front and
// dep_is_empty_batch (mip_front.hip.h) both ask this reader.
inline bool mip_device_allowed()
{
    static const bool on = [] { const char * e = xpg_env("XPG_MIP_DEVICE"); return !(e && e[0] == '0'); }();
    return on;
}

// Whether the node LPs of the deepest path fit the device tree walk's LDS budget, maximising and minimising.
// Rows of the largest node LP: the root's inequalities, one bound row per ancestor under integer branching, and -- with
// equalities at the root -- two rows for every equality convertEq2Ineq may leave unsubstituted (the root's, and under
// 0-1 branching one per ancestor). Its variables: the problem's plus one twin per free variable (extra).
inline int mip_rmax(int leq_rows, int eq_rows, int n, bool is_bin)
{
    int r = leq_rows + (is_bin ? 0 : n);
    if (eq_rows > 0) r += 2 * (eq_rows + (is_bin ? n : 0));
    return r;
}
template <class S> inline bool mip_device_fits(int leq_rows, int cols, bool is_bin, int eq_rows, int extra)
{
    const int n = cols - 1, rmax = mip_rmax(leq_rows, eq_rows, n, is_bin);
    if (rmax <= 0 || eq_rows + n + 2 > MIP_EQ_MAX || extra < 0 || extra > n) return false;
    return small_lds_bytes<S>(rmax, n + extra) <= 64 * 1024 && small_lds_bytes<S>(n + extra, rmax) <= 64 * 1024;
}
// Launch shape of k_mip_tree for nb trees whose node LPs have at most rmax rows and n variables.
struct MipGeom { size_t lds; int threads, grid; };
template <class S> inline MipGeom mip_geom_cus(int cus, int nb, int rmax, int n, bool is_max)
{
    MipGeom g;
    const int R = is_max ? rmax : n, V = is_max ? n : rmax;
    g.lds = small_lds_bytes<S>(R, V);
    const int cells = R * (V + R + 2);
    g.threads = cells >= 2048 ? 256 : (cells >= 1024 ? 128 : 64);
    // more trees than the chip holds at that width: one wave per tree, more trees in flight (8192 knapsacks of 24
    // variables: 64 / 128 / 256 threads 623 k / 425 k / 318 k MIPs/s; at 1024, where the deepest tree decides, 163 / 171 / 170 k)
    if (nb >= 8 * cus) g.threads = 64;
    const int per_cu = (int)((160 * 1024) / g.lds) > 0 ? (int)((160 * 1024) / g.lds) : 1;
    g.grid = cus * (per_cu > 8 ? 8 : per_cu) * 4;
    if (g.grid > nb) g.grid = nb;
    return g;
}
template <class S> inline MipGeom mip_geom(const xpg_ctx * ctx, int nb, int rmax, int n, bool is_max)
{ return mip_geom_cus<S>(ctx_cus(ctx), nb, rmax, n, is_max); }

// Which fit test an entry point puts in front of the device tree walk -- the one difference between the entry points that
// the rule below keeps, as found:
//   MIP_FIT_BOTH    mip_device_fits: the largest node LP fits 64 KB of LDS maximising AND minimising, and its equality list
//                   the node (mip_solve, mip_batch_eq, mip_batch_vc)
//   MIP_FIT_LAUNCH  what mip_batch_device itself refuses: the LDS of the direction the call asks for, alone (mip_batch).
//                   112 inequalities in 8 integer variables, minimising: the device under this test, the host controller
//                   under the other.
// Whether the two should be one is a decision of its own, to be made with a timing.
enum MipFit { MIP_FIT_LAUNCH = 0, MIP_FIT_BOTH = 1 };
// THE route rule of mip_front (the front and xpg_test_mip_front_route both ask it): true = the device tree walk
// (mip_batch_device), false = the host controller (mip_batch_vc_host). pattern / extra: whether vc is a sign pattern
// (vc_sign_pattern, six_host.hip.h) and its free variables; allowed: mip_device_allowed().
template <class S>
inline bool mip_front_route(MipFit fit, bool pattern, int extra, int leq_rows, int eq_rows, int cols, bool is_bin, bool is_max, bool allowed)
{
    if (!allowed || !pattern) return false;
    if (fit == MIP_FIT_BOTH) return mip_device_fits<S>(leq_rows, cols, is_bin, eq_rows, extra);
    const int n = cols - 1 + extra, rmax = mip_rmax(leq_rows, eq_rows, cols - 1, is_bin);
    return small_lds_bytes<S>(is_max ? rmax : n, is_max ? n : rmax) <= 64 * 1024;     // mip_geom's lds
}

// The device side of a one-launch MIP batch of 8-byte cells (k_mip_tree, k_mip_tree_hbm), in the manner of BatchIo
// (ctx.hip.h): the caller's arrays, the workgroups' workspaces, the answers. The caller's out_sol goes up and the kernels
// write the rows of solved trees only, so what comes down holds the caller's rows wherever a tree found no solution.
struct MipIo {
    DevBuf dfv, dl, dt, dws, dst, dv, dsol, dn, dal, de, dq;
    // free_var [extra], eqs and allow_rational where the batch has them (their blocks stay NULL otherwise); ws_bytes: the
    // workspaces of all workgroups; queue_bytes > 0: dq, a zeroed block of that size (k_mip_tree's speculation queue)
    int up(xpg_ctx * ctx, int nb, const void * tgtf, const void * leq, int leq_rows, const void * eqs, int eq_rows, int cols,
           const uint8_t * allow_rational, const int * free_var, int extra, const void * out_sol, size_t ws_bytes, size_t queue_bytes = 0)
    {
        const size_t bl = (size_t)nb * leq_rows * cols * 8, bt = (size_t)nb * cols * 8, be = (size_t)nb * eq_rows * cols * 8;
        if (extra > 0) {
            XPG_TRY(dfv.alloc(ctx, (size_t)extra * 4));
            XPG_TRY(hipMemcpyAsync(dfv.p, free_var, (size_t)extra * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        if (eq_rows > 0) {
            XPG_TRY(de.alloc(ctx, be));
            XPG_TRY(hipMemcpyAsync(de.p, eqs, be, hipMemcpyHostToDevice, ctx->stream));
        }
        if (allow_rational) {
            XPG_TRY(dal.alloc(ctx, (size_t)cols));
            XPG_TRY(hipMemcpyAsync(dal.p, allow_rational, (size_t)cols, hipMemcpyHostToDevice, ctx->stream));
        }
        if (queue_bytes) { XPG_TRY(dq.alloc(ctx, queue_bytes)); XPG_TRY(hipMemsetAsync(dq.p, 0, queue_bytes, ctx->stream)); }
        XPG_TRY(dl.alloc(ctx, bl)); XPG_TRY(dt.alloc(ctx, bt)); XPG_TRY(dws.alloc(ctx, ws_bytes));
        XPG_TRY(dst.alloc(ctx, (size_t)nb * 4)); XPG_TRY(dv.alloc(ctx, (size_t)nb * 8)); XPG_TRY(dsol.alloc(ctx, bt));
        XPG_TRY(dn.alloc(ctx, (size_t)nb * 4));
        if (bl) XPG_TRY(hipMemcpyAsync(dl.p, leq, bl, hipMemcpyHostToDevice, ctx->stream));
        XPG_TRY(hipMemcpyAsync(dt.p, tgtf, bt, hipMemcpyHostToDevice, ctx->stream));
        if (out_sol) XPG_TRY(hipMemcpyAsync(dsol.p, out_sol, bt, hipMemcpyHostToDevice, ctx->stream));
        return 0;
    }
    // Synchronises once. out_sol and out_nodes (the batch's node count) may be NULL.
    int down(xpg_ctx * ctx, int nb, int cols, int32_t * out_status, void * out_v, void * out_sol, long long * out_nodes)
    {
        std::vector<int32_t> nodes((size_t)nb);
        XPG_TRY(hipMemcpyAsync(out_status, dst.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipMemcpyAsync(out_v, dv.p, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (out_sol) XPG_TRY(hipMemcpyAsync(out_sol, dsol.p, (size_t)nb * cols * 8, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipMemcpyAsync(nodes.data(), dn.p, (size_t)nb * 4, hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        if (out_nodes) { long long t = 0; for (int b = 0; b < nb; b++) t += nodes[(size_t)b]; *out_nodes = t; }
        return 0;
    }
};

// THE launch of k_mip_tree: nb trees on g.grid walking workgroups with nhelp helper workgroups behind them (0: none, and
// spq NULL). Every pointer is a device pointer, as the kernel takes it: NULL where its comment allows.
template <class S>
int mip_tree_launch(xpg_ctx * ctx, const MipGeom & g, int nhelp, int nb, const void * tgtf, const void * leq, int leq_rows, int cols,
                    bool is_max, bool is_bin, int rmax, int depth, void * ws, size_t ws_words, void * status, void * v, void * sol,
                    void * nodes, const void * rows_of, const void * active, const void * allow, const void * eqs, int eq_rows,
                    void * spq, const void * free_var, int extra)
{
    XPG_TRY(lds_limit((const void *)k_mip_tree<S>, ctx->device, g.lds));
    hipLaunchKernelGGL((k_mip_tree<S>), dim3(g.grid + nhelp), dim3(g.threads), g.lds, ctx->stream, nb, (const S *)tgtf, (const S *)leq,
                       leq_rows, cols, is_max ? 1 : 0, is_bin ? 1 : 0, rmax, depth, (unsigned long long *)ws, ws_words,
                       (int32_t *)status, (S *)v, (S *)sol, (int *)nodes, (const int *)rows_of, (const int *)active,
                       (const uint8_t *)allow, (const S *)eqs, eq_rows, g.grid, (int *)spq, (const int *)free_var, extra);
    XPG_TRY(hipGetLastError());
    return 0;
}

// nb MIPs of one shape (x >= 0 but for the free variables free_var [extra], host, ascending; may be NULL / 0) with the tree
// walks on the device (mip_kernels.hip.h): one workgroup per problem, host arrays in and out, one launch. Returns
// XPG_ERR_UNSUPPORTED where a node LP of the deepest path would not fit the LDS budget -- the caller then takes the host
// controller below.
template <class S>
int mip_batch_device(xpg_ctx * ctx, int nb, bool is_max, bool is_bin, const S * tgtf, const S * leq, int leq_rows,
                     int cols, int32_t * out_status, S * out_v, S * out_sol, long long * out_nodes,
                     const uint8_t * allow_rational, const S * eqs, int eq_rows, const int * free_var, int extra)
{
    const int n = cols - 1;
    const int rmax = mip_rmax(leq_rows, eq_rows, n, is_bin);
    const int depth = n + 2;
    const MipGeom g = mip_geom<S>(ctx, nb, rmax, n + extra, is_max);
    if (g.lds > 64 * 1024) return XPG_ERR_UNSUPPORTED;
    const size_t ws_words = mip_ws_words(rmax, cols, depth, extra);
    // Speculative ceiling children (mip_kernels.hip.h, SP_*): for batches that leave the chip under-filled -- one tree per
    // walking workgroup, the batch lasts as long as its deepest tree -- helper workgroups behind the walkers solve the node
    // LPs the walks will need next, one helper per CU. Not with root equalities (the helper builds plain nodes only).
    const int cus = ctx_cus(ctx);
    const bool spec = eq_rows == 0 && g.grid == nb && nb <= 8 * cus;
    const int nhelp = spec ? cus : 0;        // (256 / 512 / 2048 helpers measured alike: 3.72 / 3.77 / 3.86 ms for 1024 knapsacks, 4.41 without)
    MipIo io;
    if (const int rc = io.up(ctx, nb, tgtf, leq, leq_rows, eqs, eq_rows, cols, allow_rational, free_var, extra, out_sol,
                             (size_t)(g.grid + nhelp) * ws_words * 8, spec ? spq_bytes() : 0)) return rc;
    if (const int rc = mip_tree_launch<S>(ctx, g, nhelp, nb, io.dt.p, io.dl.p, leq_rows, cols, is_max, is_bin, rmax, depth, io.dws.p, ws_words,
                                          io.dst.p, io.dv.p, out_sol ? io.dsol.p : (void *)0, io.dn.p, (const void *)0, (const void *)0,
                                          io.dal.p, io.de.p, eq_rows, io.dq.p, io.dfv.p, extra)) return rc;
    if (spec && xpg_hook("XPG_MIP_DEBUG")) {
        int hq[4] = {0, 0, 0, 0};
        XPG_TRY(hipMemcpyAsync(hq, io.dq.p, sizeof(hq), hipMemcpyDeviceToHost, ctx->stream));
        XPG_TRY(hipStreamSynchronize(ctx->stream));
        fprintf(stderr, "xpoly_amd: MIP tree walk, %d trees, %d helpers: %d ceiling children requested, %d answers taken parked\n", nb, nhelp, hq[0], hq[3]);
    }
    if (const int rc = io.down(ctx, nb, cols, out_status, out_v, out_sol, out_nodes)) return rc;
    MipRoute & rt = mip_route();
    rt.device_trees += nb;
    if (extra > rt.free_vars) rt.free_vars = extra;
    return 0;
}

// The host controller's end, the only one: every tree a MipTask under the caller's vc [cols - 1][cols], advanced in lock
// step, the answers stored as the device route stores them -- out_sol (may be NULL) in the rows of solved trees only
// (arguments checked by the caller, nb > 0).
template <class S>
int mip_batch_vc_host(xpg_ctx * ctx, int kind, int nb, bool is_max, bool is_bin, const S * tgtf, const S * vc, const S * eqs, int eq_rows,
                      const S * leq, int leq_rows, int cols, const uint8_t * allow_rational, int32_t * out_status, S * out_v, S * out_sol,
                      long long * out_nodes)
{
    std::vector<MipTask<S> > tasks(nb);
    for (int b = 0; b < nb; b++)
        tasks[b].start(make_problem<S>(tgtf + (size_t)b * cols, vc, cols - 1, eq_rows > 0 ? eqs + (size_t)b * eq_rows * cols : (const S *)0, eq_rows,
                                       leq_rows > 0 ? leq + (size_t)b * leq_rows * cols : (const S *)0, leq_rows, cols),
                       is_max, is_bin, allow_rational);
    int rc = run_mip_tasks<S>(ctx, kind, tasks);
    if (rc) return rc;
    long long nodes = 0;
    for (int b = 0; b < nb; b++) {
        const MipTask<S> & T = tasks[b];
        out_status[b] = T.final_status;
        out_v[b] = T.v;
        nodes += T.nodes;
        if (T.final_status == XPG_IP_SUCC && out_sol && (int)T.sol.size() == cols)
            for (int j = 0; j < cols; j++) out_sol[(size_t)b * cols + j] = T.sol[j];
    }
    if (out_nodes) *out_nodes = nodes;
    return 0;
}

// THE front of the four entry points below: MIP::maxm / minm (lpsol.h:2636-2657, :2681-2702) for nb problems of one shape
// under the variable constraints vc [cols - 1][cols] shared by the batch (NULL: x >= 0), with equalities and / or
// inequalities at the root and an optional rational_indicator. A vc that is a sign pattern (every variable x >= 0 or free)
// goes to the device tree walk in one launch where mip_front_route finds that the node LPs, widened by one twin per free
// variable, fit; every other vc, what does not fit and what the launch still refuses go to the host controller under the
// caller's vc, so the call is defined wherever MIP::maxm / minm is.
template <class S>
int mip_front(xpg_ctx * ctx, int kind, MipFit fit, int nb, bool is_max, bool is_bin, const S * tgtf, const S * vc, const S * eqs, int eq_rows,
              const S * leq, int leq_rows, int cols, const uint8_t * allow_rational, int32_t * out_status, S * out_v, S * out_sol,
              long long * out_nodes)
{
    if (!ctx || nb < 0 || !tgtf || eq_rows < 0 || leq_rows < 0 || (eq_rows == 0 && leq_rows == 0) || (eq_rows > 0 && !eqs) ||
        (leq_rows > 0 && !leq) || cols < 2 || !out_status || !out_v)
        return XPG_ERR_SHAPE;
    if (nb == 0) return 0;
    std::vector<int> fv;
    const bool pattern = !vc || vc_sign_pattern(vc, cols - 1, cols, fv);
    if (mip_front_route<S>(fit, pattern, (int)fv.size(), leq_rows, eq_rows, cols, is_bin, is_max, mip_device_allowed())) {
        const int rc = mip_batch_device<S>(ctx, nb, is_max, is_bin, tgtf, leq, leq_rows, cols, out_status, out_v, out_sol, out_nodes,
                                           allow_rational, eqs, eq_rows, fv.data(), (int)fv.size());
        if (rc != XPG_ERR_UNSUPPORTED) return rc;
    }
    std::vector<S> nonneg;                                              // x >= 0 as the controller takes it: -x_i <= 0
    if (!vc) {
        nonneg.assign((size_t)(cols - 1) * cols, zero<S>());
        for (int i = 0; i < cols - 1; i++) nonneg[(size_t)i * cols + i] = minus_one<S>();
        vc = nonneg.data();
    }
    return mip_batch_vc_host<S>(ctx, kind, nb, is_max, is_bin, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, allow_rational, out_status, out_v,
                                out_sol, out_nodes);
}

// One MIP::maxm / minm: a batch of one with its outputs adapted -- the status is the return value, *out_v is written
// whatever it is, out_sol (may be NULL) on XPG_IP_SUCC only.
template <class S>
int mip_solve(xpg_ctx * ctx, int kind, bool is_max, bool is_bin, const S * tgtf, const S * vc, int vc_rows,
              const S * eqs, int eq_rows, const S * leq, int leq_rows, int cols, const uint8_t * allow_rational,
              S * out_v, S * out_sol, long * out_nodes)
{
    if (!vc || cols < 2 || vc_rows != cols - 1) return XPG_ERR_SHAPE;
    int32_t st = 0; long long nodes = 0;
    std::vector<S> sol((size_t)cols, zero<S>());
    if (out_sol) for (int j = 0; j < cols; j++) sol[(size_t)j] = out_sol[j];
    const int rc = mip_front<S>(ctx, kind, MIP_FIT_BOTH, 1, is_max, is_bin, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, allow_rational, &st,
                                out_v, sol.data(), &nodes);
    if (rc) return rc;
    if (st == XPG_IP_SUCC && out_sol) for (int j = 0; j < cols; j++) out_sol[j] = sol[(size_t)j];
    if (out_nodes) *out_nodes = (long)nodes;
    return st;
}
// nb independent MIPs of one shape (x >= 0, inequalities only).
template <class S>
int mip_batch(xpg_ctx * ctx, int kind, int nb, bool is_max, bool is_bin, const S * tgtf, const S * leq, int leq_rows,
              int cols, int32_t * out_status, S * out_v, S * out_sol, long long * out_nodes)
{
    if (!leq || leq_rows <= 0) return XPG_ERR_SHAPE;
    return mip_front<S>(ctx, kind, MIP_FIT_LAUNCH, nb, is_max, is_bin, tgtf, (const S *)0, (const S *)0, 0, leq, leq_rows, cols, (const uint8_t *)0,
                        out_status, out_v, out_sol, out_nodes);
}
// nb independent MIPs of one shape WITH equalities at the root (x >= 0; the shape PolyTran::FeaSchedule passes,
// src/eng/poly.cpp:5118-5130, batched): leq may be NULL with leq_rows = 0. On the device every node runs convertEq2Ineq over
// the root's and the branches' equalities in its workgroup.
template <class S>
int mip_batch_eq(xpg_ctx * ctx, int kind, int nb, bool is_max, bool is_bin, const S * tgtf, const S * leq, int leq_rows,
                 const S * eqs, int eq_rows, int cols, int32_t * out_status, S * out_v, S * out_sol, long long * out_nodes)
{
    if (eq_rows <= 0) return XPG_ERR_SHAPE;
    return mip_front<S>(ctx, kind, MIP_FIT_BOTH, nb, is_max, is_bin, tgtf, (const S *)0, eqs, eq_rows, leq, leq_rows, cols, (const uint8_t *)0,
                        out_status, out_v, out_sol, out_nodes);
}
// nb independent MIPs of one shape under the caller's vc (what the single-problem entry points take).
template <class S>
int mip_batch_vc(xpg_ctx * ctx, int kind, int nb, bool is_max, bool is_bin, const S * tgtf, const S * vc, const S * eqs, int eq_rows,
                 const S * leq, int leq_rows, int cols, const uint8_t * allow_rational, int32_t * out_status, S * out_v, S * out_sol,
                 long long * out_nodes)
{
    if (!vc) return XPG_ERR_SHAPE;
    return mip_front<S>(ctx, kind, MIP_FIT_BOTH, nb, is_max, is_bin, tgtf, vc, eqs, eq_rows, leq, leq_rows, cols, allow_rational, out_status, out_v,
                        out_sol, out_nodes);
}

} // namespace xpg
