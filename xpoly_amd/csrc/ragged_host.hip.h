// Host helpers that several of the library's sources share (nothing here is a kernel): run_sharded, a batch over
// several devices, and the run_ragged family, problems of different shapes in one call. A source that needs one
// includes this header; xpg_create / xpg_destroy are the C entry points (include/xpoly_amd.h, through ctx.hip.h).
#pragma once
#include <string.h>
#include <algorithm>
#include <map>
#include <thread>
#include <vector>
#include "scalar.hip.h"
#include "ctx.hip.h"

namespace {
// ---- the same batches over several devices: one context + host thread per shard ------------------
// fn(ctx, lo, hi) runs shard [lo, hi) on its own context; the first error wins.
template <class F> int run_sharded(int ndev, const int * devices, int nb, F fn)
{
    if (ndev <= 0 || nb < 0) return XPG_ERR_SHAPE;
    std::vector<int> rcs((size_t)ndev, 0);
    std::vector<std::thread> th;
    const int base = nb / ndev, extra = nb % ndev;
    for (int g = 0; g < ndev; g++) {
        const int lo = g * base + (g < extra ? g : extra), hi = lo + base + (g < extra ? 1 : 0);
        const int dev = devices ? devices[g] : g;
        th.emplace_back([=, &rcs] {
            xpg_ctx * c = 0;
            int rc = xpg_create(&c, dev);
            if (rc == 0 && hi > lo) rc = fn(c, lo, hi);
            if (c) xpg_destroy(c);
            rcs[(size_t)g] = rc;
        });
    }
    for (auto & t : th) t.join();
    for (int rc : rcs) if (rc) return rc;
    return 0;
}

// ---- ragged batches: problems of DIFFERENT shapes in one call -----------------------------
// The dependence analysis of one SCoP emits polyhedra whose shape follows the statements' depths and the number of
// parameters (src/eng/poly.cpp:1120-1224, :1009-1053) and tests each (poly.cpp:268-314, :530-573); padding them to
// one shape is not parity-neutral (extra 0 <= 0 rows change the bug-compatible pivot sequence). A ragged call takes
// rows[nb], cols[nb] and the cell offsets of the concatenated systems, sorts the problems into shape classes and runs
// the classes CONCURRENTLY -- each on a lane: an extra handle (stream, scratch) on the same device that the caller's
// handle keeps, driven by a host thread for the duration of the call -- so that small classes share the chip instead
// of each waiting for the deepest problem of the one before. Results are scattered back in problem order.
struct RaggedClass { int rows, cols; std::vector<int> idx; size_t work; };
inline int ragged_lanes()
{
    static const int n = [] { const char * e = xpg_env("XPG_RAGGED_LANES"); const int v = e ? atoi(e) : 8; return v < 1 ? 1 : (v > 32 ? 32 : v); }();
    return n;
}
// fn(lane_ctx, class) for every shape class; the first error wins.
template <class F> int run_ragged(xpg_ctx * ctx, int nb, const int32_t * rows, const int32_t * cols, F fn)
{
    std::map<std::pair<int, int>, size_t> where;
    std::vector<RaggedClass> cls;
    for (int b = 0; b < nb; b++) {
        if (rows[b] <= 0 || cols[b] < 2) return XPG_ERR_SHAPE;
        const auto key = std::make_pair((int)rows[b], (int)cols[b]);
        auto it = where.find(key);
        if (it == where.end()) { it = where.insert(std::make_pair(key, cls.size())).first; cls.push_back(RaggedClass{rows[b], cols[b], {}, 0}); }
        cls[it->second].idx.push_back(b);
    }
    if (cls.empty()) return 0;                                      // nb == 0
    for (auto & c : cls) c.work = c.idx.size() * (size_t)c.rows * c.cols;
    std::sort(cls.begin(), cls.end(), [](const RaggedClass & a, const RaggedClass & b) { return a.work > b.work; });
    const int nl = (int)cls.size() < ragged_lanes() ? (int)cls.size() : ragged_lanes();
    while ((int)ctx->lanes.size() < nl - 1) {                       // lane 0 is the caller's handle
        xpg_ctx * l = 0;
        const int rc = xpg_create(&l, ctx->device);
        if (rc) return rc;
        ctx->lanes.push_back(l);
    }
    std::vector<std::vector<int> > mine((size_t)nl);               // longest class first, each to the least loaded lane
    std::vector<size_t> load((size_t)nl, 0);
    for (int k = 0; k < (int)cls.size(); k++) {
        int best = 0;
        for (int l = 1; l < nl; l++) if (load[(size_t)l] < load[(size_t)best]) best = l;
        mine[(size_t)best].push_back(k); load[(size_t)best] += cls[(size_t)k].work;
    }
    std::vector<int> rcs((size_t)nl, 0);
    auto lane_body = [&](int l) {
        xpg_ctx * c = l == 0 ? ctx : ctx->lanes[(size_t)l - 1];
        xpg::DeviceGuard bind(c->device);
        for (int k : mine[(size_t)l]) { const int rc = fn(c, cls[(size_t)k]); if (rc) { rcs[(size_t)l] = rc; return; } }
    };
    std::vector<std::thread> th;
    for (int l = 1; l < nl; l++) th.emplace_back(lane_body, l);
    lane_body(0);
    for (auto & t : th) t.join();
    for (int l = 0; l < nl; l++)
        if (rcs[(size_t)l]) {                                        // the first failing lane's code and message (after the join: no race)
            if (l) ctx->err = ctx->lanes[(size_t)l - 1]->err;
            return rcs[(size_t)l];
        }
    return 0;
}
template <class T> inline void ragged_gather(std::vector<T> & buf, const T * src, const long long * off, const RaggedClass & c, size_t per)
{
    buf.resize(c.idx.size() * per);
    for (size_t k = 0; k < c.idx.size(); k++) memcpy((void *)(buf.data() + k * per), (const void *)(src + off[c.idx[k]]), per * sizeof(T));
}
} // namespace
