"""Python face of the C ABI, shaped after the reference's solver classes so the
parity tests read like calls into xpoly:

    SIX<FloatMat,Float>  ->  SIX(ctx, F64)      maxm / minm / set_param / TwoStageMethod
    SIX<RMat,Rational>   ->  SIX(ctx, RAT)      (src/com/lpsol.h:204-338)

Arrays: fp64 problems are float64 numpy arrays; rational problems are int32
arrays with a trailing axis of 2 = (num, den) -- the in-memory layout of RMat.
Everything numeric happens in libxpoly_amd.so on the GPU.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import XPG_RUNNING, XpgError, lib, vp

F64, RAT = 0, 1
SIX_SUCC, SIX_UNBOUND, SIX_NO_PRI_FEASIBLE_SOL, SIX_OPTIMAL_IS_INFEASIBLE, SIX_TIME_OUT = range(5)


def as_kind(a, kind, ndim):
    """The array as the ABI wants it. `ndim` is the number of LOGICAL axes (1: a row such as tgtf,
    2: a matrix, 3: a stack of matrices). A rational problem is given either as integers of exactly
    that many axes (each becomes n/1) or as (num, den) pairs with ONE more, trailing axis of length 2
    -- the in-memory layout of RMat. Nothing is inferred from the shape alone: an integer matrix that
    happens to have two columns stays an integer matrix."""
    if a is None:
        return None
    if kind == F64:
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.ndim != ndim:
            raise ValueError("expected %d axes, got shape %s" % (ndim, a.shape))
        return a
    a = np.asarray(a)
    if a.dtype != np.int32 and a.size and np.issubdtype(a.dtype, np.number):
        # Rational is int32 / int32 (rational.h:66-67): a wider integer (or a float) that does not fit must not wrap silently
        lim = np.iinfo(np.int32)
        if (np.asarray(a) > lim.max).any() or (np.asarray(a) < lim.min).any():
            raise ValueError("rational input holds values outside the int32 range of xpoly's Rational")
        if not np.issubdtype(a.dtype, np.integer) and (np.asarray(a) != np.floor(a)).any():
            raise ValueError("rational input must be integers, got fractional %s values" % a.dtype)
    if a.ndim == ndim + 1:
        if a.shape[-1] != 2 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("rational input must be integer (num, den) pairs [..., 2], got %s %s" % (a.dtype, a.shape))
        return np.ascontiguousarray(a, dtype=np.int32)
    if a.ndim != ndim:
        raise ValueError("expected %d axes (integers) or %d (num/den pairs), got shape %s" % (ndim, ndim + 1, a.shape))
    out = np.empty(a.shape + (2,), dtype=np.int32)
    out[..., 0] = a
    out[..., 1] = 1
    return out


def empty_kind(shape, kind):
    if kind == F64:
        return np.zeros(shape, dtype=np.float64)
    return np.zeros(tuple(shape) + (2,), dtype=np.int32)


def _name(stem, kind, tail=""):
    return "xpg_%s_%s%s" % (stem, "f64" if kind == F64 else "rat32", tail)


def _sym(stem, kind, tail=""):
    """The entry point xpg_<stem>_<f64 | rat32><tail> of a kind: the one place a symbol is chosen by kind."""
    return getattr(lib(), _name(stem, kind, tail))


def _solved(nb, cols, kind):
    """The (status[nb], v[nb], sol[nb, cols]) triple a batch solver writes into."""
    return np.zeros(nb, dtype=np.int32), empty_kind((nb,), kind), empty_kind((nb, cols), kind)


class Context:
    """xpg_ctx: one GPU, one HIP stream."""

    def __init__(self, device=0):
        self._h = C.c_void_p()
        rc = lib().xpg_create(C.byref(self._h), C.c_int(device))
        if rc != 0:
            raise XpgError("xpg_create(device=%d) failed: %s" % (device, _capi.ERRORS.get(rc, rc)))
        self.device = device

    def check(self, rc, what):
        if rc < 0 and rc != XPG_RUNNING:
            raise XpgError("%s: %s (%s)" % (what, _capi.ERRORS.get(rc, rc),
                                            lib().xpg_last_error(self._h).decode()))
        return rc

    @property
    def stream(self):
        return lib().xpg_stream(self._h)

    def sync(self):
        self.check(lib().xpg_sync(self._h), "xpg_sync")

    def profile_begin(self, cap, stride=1):
        self.check(lib().xpg_profile_begin(self._h, C.c_int(cap), C.c_int(stride)), "xpg_profile_begin")

    def profile_end(self):
        n, ms = C.c_int(), C.c_double()
        self.check(lib().xpg_profile_end(self._h, C.byref(n), C.byref(ms)), "xpg_profile_end")
        return n.value, ms.value

    def malloc(self, nbytes):
        p = C.c_void_p()
        self.check(lib().xpg_malloc(self._h, C.byref(p), C.c_size_t(nbytes)), "xpg_malloc")
        return p.value

    def free(self, ptr):
        self.check(lib().xpg_free(self._h, C.c_void_p(ptr)), "xpg_free")

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.check(lib().xpg_upload(self._h, C.c_void_p(dptr), vp(arr), C.c_size_t(arr.nbytes)), "xpg_upload")

    def download(self, arr, dptr):
        self.check(lib().xpg_download(self._h, vp(arr), C.c_void_p(dptr), C.c_size_t(arr.nbytes)), "xpg_download")
        return arr

    def close(self):
        if self._h:
            for r in list(getattr(self, "_lps", ())):       # device LPs of this context first: they hold its stream and buffers
                lp = r()
                if lp is not None:
                    lp.close()
            lib().xpg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- K1 ---------------------------------------------------------------------------
    def pivot(self, kind, tab, obj, rhs_idx, row, col):
        """SIX::pivot arithmetic (lpsol.h:1471-1501) on host arrays, in place."""
        tab = as_kind(tab, kind, 2); obj = as_kind(obj, kind, 1)
        m, W = tab.shape[0], tab.shape[1]
        self.check(_sym("pivot", kind)(self._h, vp(tab), C.c_int(m), C.c_int(W), vp(obj), C.c_int(rhs_idx),
                                       C.c_int(row), C.c_int(col)), "xpg_pivot")
        return tab, obj

    def pivot_dev(self, kind, tab_ptr, m, W, ld, obj_ptr, rhs_idx, row, col):
        self.check(_sym("pivot", kind, "_dev")(self._h, vp(tab_ptr), C.c_int(m), C.c_int(W), C.c_int(ld), vp(obj_ptr),
                                               C.c_int(rhs_idx), C.c_int(row), C.c_int(col)), "xpg_pivot_dev")

    # ---- batches --------------------------------------------------------------------------
    def six_batch(self, kind, is_max, tgtf, leq, max_iter=0xFFFFFFFF):
        return _six_batch(self, "six_batch", kind, is_max, tgtf, leq, max_iter, None)

    def _batch_dev(self, stem, kind, is_max, nb, tgtf_ptr, leq_ptr, m, cols, status_ptr, v_ptr, sol_ptr, pivots_ptr, max_iter):
        """xpg_<stem>_*_dev: device pointers, enqueue only; pivots_ptr may be None."""
        self.check(_sym(stem, kind, "_dev")(self._h, C.c_int(int(is_max)), C.c_int(nb), vp(tgtf_ptr), vp(leq_ptr), C.c_int(m),
                                            C.c_int(cols), C.c_uint(max_iter), vp(status_ptr), vp(v_ptr), vp(sol_ptr),
                                            vp(pivots_ptr)), "xpg_%s_dev" % stem)

    def _batch_vc_dev(self, stem, kind, is_max, nb, tgtf_ptr, vc_ptr, eq_ptr, eq_rows, leq_ptr, leq_rows, cols, status_ptr, v_ptr,
                      sol_ptr, max_iter, *pivots):
        """xpg_<stem>_*_dev: device pointers for every array (vc included), enqueue only; eq_ptr / leq_ptr may be None with 0
        rows (not both). pivots: the pivot counts' pointer (or None) where the entry point takes one."""
        self.check(_sym(stem, kind, "_dev")(self._h, C.c_int(int(is_max)), C.c_int(nb), vp(tgtf_ptr), vp(vc_ptr), vp(eq_ptr),
                                            C.c_int(eq_rows), vp(leq_ptr), C.c_int(leq_rows), C.c_int(cols), C.c_uint(max_iter),
                                            vp(status_ptr), vp(v_ptr), vp(sol_ptr), *(vp(p) for p in pivots)),
                   "xpg_%s_dev" % stem)

    def six_batch_dev(self, kind, is_max, nb, tgtf_ptr, leq_ptr, m, cols, status_ptr, v_ptr, sol_ptr,
                      pivots_ptr=None, max_iter=0xFFFFFFFF):
        self._batch_dev("six_batch", kind, is_max, nb, tgtf_ptr, leq_ptr, m, cols, status_ptr, v_ptr, sol_ptr, pivots_ptr, max_iter)

    def six_batch_vc_dev(self, kind, is_max, nb, tgtf_ptr, vc_ptr, eq_ptr, eq_rows, leq_ptr, leq_rows, cols, status_ptr, v_ptr,
                         sol_ptr, max_iter=0xFFFFFFFF):
        """xpg_six_batch_vc_*_dev: device pointers for every array (vc included), enqueue only -- results after sync().
        eq_ptr / leq_ptr may be None with 0 rows (not both). Nothing falls back here: a vc that is no sign pattern, or a shape
        beyond 64 KB of LDS, ends every LP with status -4."""
        self._batch_vc_dev("six_batch_vc", kind, is_max, nb, tgtf_ptr, vc_ptr, eq_ptr, eq_rows, leq_ptr, leq_rows, cols, status_ptr,
                           v_ptr, sol_ptr, max_iter)

    def six_batch_hbm_dev(self, kind, is_max, nb, tgtf_ptr, leq_ptr, m, cols, status_ptr, v_ptr, sol_ptr,
                          pivots_ptr=None, max_iter=0xFFFFFFFF):
        """xpg_six_batch_hbm_*_dev: six_batch_dev for LPs of any size (device pointers, enqueue only)."""
        self._batch_dev("six_batch_hbm", kind, is_max, nb, tgtf_ptr, leq_ptr, m, cols, status_ptr, v_ptr, sol_ptr, pivots_ptr, max_iter)

    def six_batch_vc_hbm_dev(self, kind, is_max, nb, tgtf_ptr, vc_ptr, eq_ptr, eq_rows, leq_ptr, leq_rows, cols, status_ptr, v_ptr,
                             sol_ptr, pivots_ptr=None, max_iter=0xFFFFFFFF):
        """xpg_six_batch_vc_hbm_*_dev: six_batch_vc_dev for shapes of any size (device pointers for every array, enqueue only).
        Sized for every variable free: within 64 KB the LDS-resident launch, untouched (pivots_ptr then reads 0xFFFFFFFF, "not
        counted"), otherwise every LP on a slot in device memory (pivots_ptr: each LP's pivot count). Beyond that kernel's
        limits: XpgError (XPG_ERR_UNSUPPORTED), nothing launched or written."""
        self._batch_vc_dev("six_batch_vc_hbm", kind, is_max, nb, tgtf_ptr, vc_ptr, eq_ptr, eq_rows, leq_ptr, leq_rows, cols, status_ptr,
                           v_ptr, sol_ptr, max_iter, pivots_ptr)

    def has_solution_batch_dev(self, nb, leq_ptr, leq_rows, eq_ptr, eq_rows, vc_ptr, cols, is_unique_sol, has_ptr, status_ptr=None,
                               max_iter=0xFFFFFFFF, is_int_sol=False):
        """xpg_has_solution_batch_rat32_dev: has_solution_batch on device pointers (vc included), enqueue only -- results after
        sync(). Sized for every variable free. A vc that is no sign pattern ends every system -4; a shape beyond both kernels, or
        is_int_sol, raises XpgError and launches nothing."""
        self.check(lib().xpg_has_solution_batch_rat32_dev(
            self._h, C.c_int(nb), vp(leq_ptr), C.c_int(leq_rows), vp(eq_ptr), C.c_int(eq_rows), vp(vc_ptr),
            C.c_int(cols - 1), C.c_int(cols), C.c_int(cols - 1), C.c_int(int(is_int_sol)), C.c_int(int(is_unique_sol)),
            C.c_uint(max_iter), vp(has_ptr), vp(status_ptr)), "xpg_has_solution_batch_rat32_dev")

    def trim(self):
        """xpg_trim: cached device blocks, pinned staging and the scratch of six_batch_vc / six_batch_hbm / six_batch_vc_hbm /
        has_solution_batch go back to the runtime."""
        self.check(lib().xpg_trim(self._h), "xpg_trim")


def _check_multi(rc, what):
    if rc < 0:
        raise XpgError("%s: %s" % (what, _capi.ERRORS.get(rc, rc)))


def six_batch_multi(devices, kind, is_max, tgtf, leq, max_iter=0xFFFFFFFF):
    """xpg_six_batch_*_multi: the batch cut into contiguous shards, one per entry of `devices`, each on a
    context and host thread of its own inside the library; results land in these host arrays."""
    tgtf = as_kind(tgtf, kind, 2); leq = as_kind(leq, kind, 3)
    nb, m, cols = leq.shape[0], leq.shape[1], leq.shape[2]
    status, v, sol = _solved(nb, cols, kind)
    dev = (C.c_int * len(devices))(*devices)
    _check_multi(_sym("six_batch", kind, "_multi")(C.c_int(len(devices)), dev, C.c_int(int(is_max)), C.c_int(nb), vp(tgtf), vp(leq),
                                                   C.c_int(m), C.c_int(cols), C.c_uint(max_iter), vp(status), vp(v), vp(sol)),
                 "xpg_six_batch_multi")
    return status, v, sol


def mip_batch_multi(devices, is_max, is_bin, tgtf, leq):
    tgtf = as_kind(tgtf, RAT, 2); leq = as_kind(leq, RAT, 3)
    nb, rows, cols = leq.shape[0], leq.shape[1], leq.shape[2]
    st, v, sol = _solved(nb, cols, RAT)
    nodes = C.c_longlong()
    dev = (C.c_int * len(devices))(*devices)
    _check_multi(lib().xpg_mip_batch_rat32_multi(C.c_int(len(devices)), dev, C.c_int(nb), C.c_int(int(is_max)),
                                                 C.c_int(int(is_bin)), vp(tgtf), vp(leq), C.c_int(rows), C.c_int(cols),
                                                 vp(st), vp(v), vp(sol), C.byref(nodes)), "xpg_mip_batch_rat32_multi")
    return st, v, sol, nodes.value


def dep_is_empty_batch_multi(devices, mats):
    mats = as_kind(mats, RAT, 3)
    nb, rows, cols = mats.shape[0], mats.shape[1], mats.shape[2]
    out = np.zeros(nb, dtype=np.int32)
    nodes = C.c_longlong()
    dev = (C.c_int * len(devices))(*devices)
    _check_multi(lib().xpg_dep_is_empty_batch_rat32_multi(C.c_int(len(devices)), dev, C.c_int(nb), vp(mats), C.c_int(rows),
                                                          C.c_int(cols), vp(out), C.byref(nodes)),
                 "xpg_dep_is_empty_batch_rat32_multi")
    return out, nodes.value


class DeviceLP:
    """xpg_lp: a slack-form LP living in HBM (tableau, objective row, basis)."""

    def __init__(self, ctx, kind, leq, tgtf, vc_diag=None, vc_rhs=None, on_device=False, m=None, cols=None):
        self.ctx, self.kind = ctx, kind
        if on_device:
            leq_p, tg_p = C.c_void_p(leq), C.c_void_p(tgtf)
        else:
            leq = as_kind(leq, kind, 2); tgtf = as_kind(tgtf, kind, 1)
            m, cols = leq.shape[0], leq.shape[1]
            leq_p, tg_p = vp(leq), vp(tgtf)
        self.m, self.cols = m, cols
        vd = as_kind(vc_diag, kind, 1); vr = as_kind(vc_rhs, kind, 1)
        self._h = C.c_void_p()
        ctx.check(lib().xpg_lp_create(ctx._h, C.c_int(kind), leq_p, C.c_int(m), C.c_int(cols), tg_p,
                                      vp(vd), vp(vr), C.c_int(int(on_device)), C.byref(self._h)),
                  "xpg_lp_create")
        import weakref
        if not hasattr(ctx, "_lps"):
            ctx._lps = []
        ctx._lps.append(weakref.ref(self))

    def set_options(self, pricing=0, feas_rel_tol=0.0):
        """Opt-in NON-PARITY modes (xpg_lp_set_options): pricing=1 Dantzig's rule, feas_rel_tol>0 a
        tolerant SIX::is_feasible. (0, 0.0) is the reference's behaviour."""
        return self.ctx.check(lib().xpg_lp_set_options(self._h, C.c_int(pricing), C.c_double(feas_rel_tol)),
                              "xpg_lp_set_options")

    def two_stage(self, max_iter=0xFFFFFFFF):
        return self.ctx.check(lib().xpg_lp_two_stage(self._h, C.c_uint(max_iter)), "xpg_lp_two_stage")

    def begin(self):
        return self.ctx.check(lib().xpg_lp_begin(self._h), "xpg_lp_begin")

    def iterate(self, pivots):
        return self.ctx.check(lib().xpg_lp_iterate(self._h, C.c_uint(pivots)), "xpg_lp_iterate")

    def pivots_done(self):
        n = C.c_uint()
        self.ctx.check(lib().xpg_lp_pivots_done(self._h, C.byref(n)), "xpg_lp_pivots_done")
        return n.value

    def counters(self):
        """(sweeps of a full 16-pivot batch, sweeps of a shorter one) of the blocked loop since begin()."""
        f, p = C.c_uint(), C.c_uint()
        self.ctx.check(lib().xpg_lp_counters(self._h, C.byref(f), C.byref(p)), "xpg_lp_counters")
        return f.value, p.value

    def chain_aborts(self):
        """(chain launches given up at their roll call in this solve, whether the solve switched to launch-per-stage)."""
        n, off, runs = C.c_uint(), C.c_int(), C.c_uint()
        self.ctx.check(lib().xpg_lp_chain_aborts(self._h, C.byref(n), C.byref(off), C.byref(runs)), "xpg_lp_chain_aborts")
        self.chain_runs = runs.value
        return n.value, bool(off.value)

    def chain_folds(self):
        """chain launches of this solve that did their batch's stage 0 themselves."""
        n = C.c_uint()
        self.ctx.check(lib().xpg_lp_chain_folds(self._h, C.byref(n)), "xpg_lp_chain_folds")
        return n.value

    def loop_info(self):
        """xpg_lp_loop_info: which loop and kernel instances run the LP in its current shape."""
        o = (C.c_int32 * 10)()
        self.ctx.check(lib().xpg_lp_loop_info(self._h, o, C.c_int(10)), "xpg_lp_loop_info")
        return dict(loop={0: "pipelined", 3: "blocked"}.get(o[0], o[0]), pivots_per_pass=o[1],
                    chain={0: "launch per stage", 1: "one launch, one XCD", 2: "one launch, spread"}[o[2]] if o[0] == 3 else None,
                    chain_line=o[3], sweep_rows=o[4], ld=o[5], chain_workers=o[6], pick_workers=o[7], prep_workers=o[8],
                    chain_lds_bytes=o[9])

    def r32_loop_ran(self):
        """The device-resident loop a Rational handle's last iterations ran on: None (none yet), "fused" (one launch per
        pivot, lp_fused_r32.hip.h) or "pipe" (two launches, lp_pipe_r32.hip.h) -- the 11th figure of xpg_lp_loop_info."""
        o = (C.c_int32 * 11)()
        self.ctx.check(lib().xpg_lp_loop_info(self._h, o, C.c_int(11)), "xpg_lp_loop_info")
        return {0: None, 1: "fused", 2: "pipe"}[o[10]]

    def shape(self):
        r, w, rhs = C.c_int(), C.c_int(), C.c_int()
        self.ctx.check(lib().xpg_lp_shape(self._h, C.byref(r), C.byref(w), C.byref(rhs)), "xpg_lp_shape")
        return r.value, w.value, rhs.value

    def read(self, want_tab=True):
        r, W, rhs = self.shape()
        k = self.kind
        tab = empty_kind((r, W), k) if want_tab else None
        obj = empty_kind((W,), k)
        nv = np.zeros(rhs, dtype=np.uint8); bv = np.zeros(rhs, dtype=np.uint8)
        bv2eq = np.zeros(rhs, dtype=np.int32); eq2bv = np.zeros(r, dtype=np.int32)
        maxv = empty_kind((1,), k); sol = empty_kind((W,), k)
        self.ctx.check(lib().xpg_lp_read(self._h, vp(tab), vp(obj), vp(nv), vp(bv), vp(bv2eq), vp(eq2bv),
                                         vp(maxv), vp(sol)), "xpg_lp_read")
        return dict(tab=tab, tgtf=obj, nvset=nv, bvset=bv, bv2eq=bv2eq, eq2bv=eq2bv, rhs=rhs,
                    maxv=maxv[0], sol=sol)

    def trace(self, cap=65536):
        pairs = np.zeros((cap, 2), dtype=np.int32)
        n = C.c_int()
        self.ctx.check(lib().xpg_lp_trace(self._h, vp(pairs), C.c_int(cap), C.byref(n)), "xpg_lp_trace")
        return pairs[: min(n.value, cap)].copy()

    def close(self):
        if self._h:
            lib().xpg_lp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MIP:
    """Mirror of MIP<Mat,T> (src/com/lpsol.h:2087-2157): maxm / minm with is_bin and
    rational_indicator; IP_* status codes."""

    def __init__(self, ctx, kind):
        self.ctx, self.kind = ctx, kind

    def _solve(self, is_max, tgtf, vc, eq, leq, is_bin, rational_indicator):
        ind = None if rational_indicator is None else np.ascontiguousarray(rational_indicator, dtype=np.uint8)
        return _solve_one(self.ctx, "mip", self.kind, is_max, tgtf, vc, eq, leq, C.c_int(int(is_bin)), vp(ind))

    def maxm(self, tgtf, vc, eq, leq, is_bin=False, rational_indicator=None):     # lpsol.h:2636-2657
        return self._solve(True, tgtf, vc, eq, leq, is_bin, rational_indicator)

    def minm(self, tgtf, vc, eq, leq, is_bin=False, rational_indicator=None):     # lpsol.h:2681-2702
        return self._solve(False, tgtf, vc, eq, leq, is_bin, rational_indicator)


PROFILE_FIELDS = ("total_ms", "host_reshape_ms", "create_and_upload_ms", "dual_on_device_ms", "device_solve_ms", "read_back_ms", "release_ms",
                  "route", "pivots")


def six_last_profile():
    """Where the calling thread's last SIX.maxm / minm call spent its time (xpg_six_last_profile), milliseconds."""
    d = {k: round(x, 3) for k, x in _view("xpg_six_last_profile", PROFILE_FIELDS, ctype=C.c_double).items()}
    d["route"] = {1: "LDS batch kernel", 2: "HBM-resident loop"}.get(int(d["route"]), "none")
    d["pivots"] = int(d["pivots"])                   # HBM-resident route: pivots of the loop that ended the solve
    return d


def mip_warm(ctx, is_max, tgtf, leq, is_bin=False):
    """OPT-IN, NON-PARITY (xpg_mip_warm_f64): fp64 branch and bound warm-started from the parent's tableau by the dual
    simplex. Returns (status, v, sol, dict(nodes, dual_pivots, root_pivots, max_depth))."""
    tgtf = as_kind(tgtf, F64, 1); leq = as_kind(leq, F64, 2)
    rows, cols = leq.shape
    v = C.c_double(); sol = np.zeros(cols); stats = (C.c_longlong * 4)()
    st = lib().xpg_mip_warm_f64(ctx._h, C.c_int(int(is_max)), vp(tgtf), vp(leq), C.c_int(rows), C.c_int(cols),
                                C.c_int(int(is_bin)), C.byref(v), vp(sol), stats)
    ctx.check(st, "xpg_mip_warm_f64")
    return st, v.value, sol, dict(nodes=stats[0], dual_pivots=stats[1], root_pivots=stats[2], max_depth=stats[3])


def mip_warm_batch(ctx, is_max, tgtf, leq, is_bin=False):
    """OPT-IN, NON-PARITY (xpg_mip_warm_batch_f64): nb fp64 integer programs of one shape, each tree walked by one workgroup
    with the dual simplex warm-started from the parent's tableau. tgtf [nb, cols], leq [nb, rows, cols].
    Returns (status[nb], v[nb], sol[nb, cols], dict(nodes, dual_pivots, root_pivots, max_depth))."""
    tgtf = as_kind(tgtf, F64, 2); leq = as_kind(leq, F64, 3)
    nb, rows, cols = leq.shape
    st = np.zeros(nb, dtype=np.int32); v = np.zeros(nb); sol = np.zeros((nb, cols)); stats = (C.c_longlong * 4)()
    ctx.check(lib().xpg_mip_warm_batch_f64(ctx._h, C.c_int(nb), C.c_int(int(is_max)), vp(tgtf), vp(leq), C.c_int(rows), C.c_int(cols),
                                           C.c_int(int(is_bin)), vp(st), vp(v), vp(sol), stats), "xpg_mip_warm_batch_f64")
    return st, v, sol, dict(nodes=stats[0], dual_pivots=stats[1], root_pivots=stats[2], max_depth=stats[3])


def mip_batch(ctx, is_max, is_bin, tgtf, leq, kind=RAT):
    """nb independent MIPs (x >= 0, inequalities only), each tree walked on the device by one workgroup.
    tgtf [nb, cols(,2)], leq [nb, rows, cols(,2)]. Returns (status[nb], v[nb(,2)], sol[nb,cols(,2)], nodes)."""
    tgtf = as_kind(tgtf, kind, 2); leq = as_kind(leq, kind, 3)
    nb, rows, cols = leq.shape[0], leq.shape[1], leq.shape[2]
    st, v, sol = _solved(nb, cols, kind)
    nodes = C.c_longlong()
    ctx.check(_sym("mip_batch", kind)(ctx._h, C.c_int(nb), C.c_int(int(is_max)), C.c_int(int(is_bin)), vp(tgtf), vp(leq), C.c_int(rows),
                                      C.c_int(cols), vp(st), vp(v), vp(sol), C.byref(nodes)), "xpg_mip_batch")
    return st, v, sol, nodes.value


def mip_batch_eq(ctx, is_max, is_bin, tgtf, leq, eq, kind=RAT):
    """nb independent MIPs with equalities at the root (x >= 0): tgtf [nb, cols(,2)], leq [nb, rows, cols(,2)] or None,
    eq [nb, eq_rows, cols(,2)]. Returns (status[nb], v[nb(,2)], sol[nb,cols(,2)], nodes)."""
    tgtf = as_kind(tgtf, kind, 2); eq = as_kind(eq, kind, 3)
    leq = None if leq is None else as_kind(leq, kind, 3)
    nb, eq_rows, cols = eq.shape[0], eq.shape[1], eq.shape[2]
    rows = 0 if leq is None else leq.shape[1]
    st, v, sol = _solved(nb, cols, kind)
    nodes = C.c_longlong()
    ctx.check(_sym("mip_batch_eq", kind)(ctx._h, C.c_int(nb), C.c_int(int(is_max)), C.c_int(int(is_bin)), vp(tgtf), vp(leq), C.c_int(rows),
                                         vp(eq), C.c_int(eq_rows), C.c_int(cols), vp(st), vp(v), vp(sol), C.byref(nodes)),
              "xpg_mip_batch_eq")
    return st, v, sol, nodes.value


def _vc_batch_args(kind, tgtf, vc, leq, eq):
    """The arrays of a batch under one vc as the ABI wants them, checked against each other:
    (tgtf, vc, leq, eq, nb, cols, leq rows, eq rows)."""
    tgtf = as_kind(tgtf, kind, 2); vc = as_kind(vc, kind, 2)
    leq = None if leq is None else as_kind(leq, kind, 3)
    eq = None if eq is None else as_kind(eq, kind, 3)
    nb, cols = tgtf.shape[0], tgtf.shape[1]
    if vc.shape[0] != cols - 1 or vc.shape[1] != cols:
        raise ValueError("vc must be [cols - 1, cols] = %s, got %s" % ((cols - 1, cols), vc.shape[:2]))
    for a in (leq, eq):
        if a is not None and (a.shape[0] != nb or a.shape[2] != cols):
            raise ValueError("leq / eq must be [nb, rows, cols]")
    rows = 0 if leq is None else leq.shape[1]
    eq_rows = 0 if eq is None else eq.shape[1]
    return tgtf, vc, leq, eq, nb, cols, rows, eq_rows


def _view(name, fields, *args, ctype=C.c_longlong):
    """A host-only view of the library that fills n values of `ctype` (long long; double for the profile): its values under
    `fields`. The one way any "fill n values" view of the package is read."""
    out = (ctype * len(fields))()
    rc = getattr(lib(), name)(*args, out, C.c_int(len(fields)))
    if rc != 0:
        raise XpgError("%s: %s" % (name, _capi.ERRORS.get(rc, rc)))
    return dict(zip(fields, out))


def _six_batch(ctx, stem, kind, is_max, tgtf, leq, max_iter, out):
    """xpg_<stem>_*: nb LPs of one shape (x >= 0, inequalities only) in one call. out: a triple to write into, or None."""
    tgtf = as_kind(tgtf, kind, 2); leq = as_kind(leq, kind, 3)
    nb, m, cols = leq.shape[0], leq.shape[1], leq.shape[2]
    status, v, sol = _solved(nb, cols, kind) if out is None else out
    ctx.check(_sym(stem, kind)(ctx._h, C.c_int(int(is_max)), C.c_int(nb), vp(tgtf), vp(leq), C.c_int(m), C.c_int(cols),
                               C.c_uint(max_iter), vp(status), vp(v), vp(sol)), "xpg_" + stem)
    return status, v, sol


def _six_batch_vc(ctx, stem, kind, is_max, tgtf, vc, leq, eq, max_iter, out):
    """xpg_<stem>_*: nb LPs of one shape under one vc in one call. out: a triple to write into, or None."""
    tgtf, vc, leq, eq, nb, cols, rows, eq_rows = _vc_batch_args(kind, tgtf, vc, leq, eq)
    st, v, sol = _solved(nb, cols, kind) if out is None else out
    ctx.check(_sym(stem, kind)(ctx._h, C.c_int(int(is_max)), C.c_int(nb), vp(tgtf), vp(vc), vp(eq if eq_rows else None), C.c_int(eq_rows),
                               vp(leq if rows else None), C.c_int(rows), C.c_int(cols), C.c_uint(max_iter), vp(st), vp(v), vp(sol)),
              "xpg_" + stem)
    return st, v, sol


def _mip_batch_vc(ctx, stem, is_max, is_bin, tgtf, vc, leq, eq, ind, kind):
    """xpg_<stem>_*: nb MIPs of one shape under one vc in one call: (status[nb], v[nb(,2)], sol[nb,cols(,2)], nodes)."""
    tgtf, vc, leq, eq, nb, cols, rows, eq_rows = _vc_batch_args(kind, tgtf, vc, leq, eq)
    ind = None if ind is None else np.ascontiguousarray(ind, dtype=np.uint8)
    st, v, sol = _solved(nb, cols, kind)
    nodes = C.c_longlong()
    ctx.check(_sym(stem, kind)(ctx._h, C.c_int(nb), C.c_int(int(is_max)), C.c_int(int(is_bin)), vp(tgtf), vp(vc), vp(eq), C.c_int(eq_rows),
                               vp(leq), C.c_int(rows), C.c_int(cols), vp(ind), vp(st), vp(v), vp(sol), C.byref(nodes)), "xpg_" + stem)
    return st, v, sol, nodes.value


def _solve_one(ctx, stem, kind, is_max, tgtf, vc, eq, leq, *mid):
    """xpg_<six | mip>_<maxm | minm>_*: one problem; `mid` are the arguments between cols and the results (max_iter, or is_bin
    and the rational indicator). Status -7 (the reference is undefined) is an answer, any other negative status is raised."""
    tgtf = as_kind(tgtf, kind, 1); vc = as_kind(vc, kind, 2)
    cols = tgtf.shape[0]
    eq_rows = 0 if eq is None else len(eq)
    leq_rows = 0 if leq is None else len(leq)
    eq_a = as_kind(eq, kind, 2) if eq_rows else None
    leq_a = as_kind(leq, kind, 2) if leq_rows else None
    v = empty_kind((1,), kind); sol = empty_kind((cols,), kind)
    stem = "%s_%s" % (stem, "maxm" if is_max else "minm")
    st = _sym(stem, kind)(ctx._h, vp(tgtf), vp(vc), C.c_int(vc.shape[0]), vp(eq_a), C.c_int(eq_rows), vp(leq_a), C.c_int(leq_rows), C.c_int(cols),
                          *mid, vp(v), vp(sol))
    if st < 0 and st != -7:
        ctx.check(st, _name(stem, kind))
    return st, v[0], sol


def mip_batch_vc(ctx, is_max, is_bin, tgtf, vc, leq, eq=None, rational_indicator=None, kind=RAT):
    """nb independent MIPs under the variable constraints vc [cols - 1, cols(,2)] shared by the batch: tgtf [nb, cols(,2)],
    leq [nb, rows, cols(,2)] or None, eq [nb, eq_rows, cols(,2)] or None (not both None), rational_indicator cols bytes or None.
    A vc that is a sign pattern (diagonal -1 = x >= 0, 0 = free, nothing else) is walked on the device, free variables split
    v = v' - v'' in front of every node LP; any other vc by the host controller. Returns (status[nb], v[nb(,2)], sol[nb,cols(,2)], nodes)."""
    return _mip_batch_vc(ctx, "mip_batch_vc", is_max, is_bin, tgtf, vc, leq, eq, rational_indicator, kind)

def mip_last_route():
    """Which route the trees of the calling thread's last MIP / has_solution / dep_is_empty call took (xpg_mip_last_route):
    device_trees walked by the tree-walk kernel, host_trees by the host controller, free_vars split per tree on the device."""
    return _view("xpg_mip_last_route", ("device_trees", "host_trees", "free_vars"))

def mip_batch_vc_hbm(ctx, is_max, is_bin, tgtf, vc, leq, eq=None, ind=None, kind=RAT):
    """xpg_mip_batch_vc_hbm_*: mip_batch_vc for node LPs of any size. A sign-pattern vc and node LPs within 64 KB of LDS: the
    launch mip_batch_vc makes; a sign-pattern vc past that: still one launch, a workgroup per tree with the node tableaux in
    device memory; anything else by the host controller. Arrays as mip_batch_vc takes them (ind: the rational_indicator).
    Returns (status[nb], v[nb(,2)], sol[nb,cols(,2)], nodes)."""
    return _mip_batch_vc(ctx, "mip_batch_vc_hbm", is_max, is_bin, tgtf, vc, leq, eq, ind, kind)

def mip_hbm_last_route():
    """{'lds', 'hbm', 'host', 'free', 'grid'}: trees of this thread's last mip_batch_vc_hbm call on the LDS-resident walk / on
    the device-memory walk / on the host controller, the free variables split per tree, and the grid of its launch."""
    return _view("xpg_mip_hbm_last_route", ("lds", "hbm", "host", "free", "grid"))


MIP_HBM_FIELDS = ("route", "free", "R", "V", "lds", "slot", "ld", "ws_words", "threads", "grid", "scratch")


def mip_hbm_plan(kind, vc, leq_rows, eq_rows, cols, is_bin, is_max, nb, num_cus=256):
    """xpg_test_mip_hbm_plan (host only, no device): what mip_batch_vc_hbm does with nb trees of a shape under vc
    [cols - 1, cols(,2)] -- route (0 LDS-resident walk, 1 device-memory walk, 2 host controller), free variables, the rows and
    variables the largest node LP is solved with, LDS bytes, slot bytes, ld, workspace words, threads, grid, scratch bytes."""
    vc_a = as_kind(vc, kind, 2)
    free = np.zeros(cols - 1, dtype=np.uint8)
    pat = lib().xpg_test_vc_pattern(C.c_int(kind), vp(vc_a), C.c_int(vc_a.shape[0]), C.c_int(cols), vp(free))
    if pat < 0:
        raise XpgError("xpg_test_vc_pattern: %s" % _capi.ERRORS.get(pat, pat))
    return _view("xpg_test_mip_hbm_plan", MIP_HBM_FIELDS, C.c_int(kind), C.c_int(pat), C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(cols),
                 C.c_int(int(is_bin)), C.c_int(int(is_max)), C.c_int(int(free.sum())), C.c_int(nb), C.c_int(num_cus))


def six_batch_vc(ctx, kind, is_max, tgtf, vc, leq, eq=None, max_iter=0xFFFFFFFF):
    """SIX::maxm / minm for nb problems of one shape WITH equalities and free variables in one call (xpg_six_batch_vc_*):
    tgtf [nb, cols(,2)], vc [cols - 1, cols(,2)] shared by the batch, leq [nb, rows, cols(,2)] or None, eq [nb, eq_rows, cols(,2)]
    or None (not both None). A vc that is a sign pattern (diagonal -1 = x >= 0, 0 = free, nothing else) and a shape within
    64 KB of LDS: SIX::normalize, the solve and calcFinalSolution run on the device for the whole batch; anything else is
    solved per problem as SIX.maxm / minm would. Returns (status[nb], v[nb(,2)], sol[nb, cols(,2)]); status -7 marks the
    problems the reference is undefined on; sol rows are written on status 0 only."""
    return _six_batch_vc(ctx, "six_batch_vc", kind, is_max, tgtf, vc, leq, eq, max_iter, None)

def six_batch_hbm(ctx, kind, is_max, tgtf, leq, max_iter=0xFFFFFFFF, out=None):
    """xpg_six_batch_hbm_*: Context.six_batch for LPs of any size -- an LP that fits one CU's LDS is solved as six_batch
    solves it, a larger one by a workgroup of its own on a tableau in device memory. tgtf [nb, cols], leq [nb, m, cols].
    Returns (status[nb], v[nb], sol[nb, cols]); `out`: such a triple to write into (rows of sol whose status is not 0 are
    left alone). A shape beyond the kernel's limits raises XpgError (XPG_ERR_UNSUPPORTED) and writes nothing."""
    return _six_batch(ctx, "six_batch_hbm", kind, is_max, tgtf, leq, max_iter, out)

def six_batch_hbm_last_route():
    """{'lds', 'hbm', 'grid'}: LPs of this thread's last six_batch_hbm call solved LDS-resident / on tableaux in device
    memory, and the grid of its launch."""
    return _view("xpg_six_batch_hbm_last_route", ("lds", "hbm", "grid"))


BATCH_HBM_FIELDS = ("route", "lds", "slot", "ld", "threads", "grid", "scratch")


def six_batch_hbm_geometry(kind, R, V, nb, num_cus=256):
    """xpg_test_batch_hbm_geometry (host only, no device): what six_batch_hbm does with nb LPs solved as R rows x V
    variables -- route (0 LDS-resident, 1 tableau in device memory, 2 refused), LDS bytes, slot bytes, ld, threads, grid,
    scratch bytes of the launch."""
    return _view("xpg_test_batch_hbm_geometry", BATCH_HBM_FIELDS, C.c_int(kind), C.c_int(R), C.c_int(V), C.c_int(nb), C.c_int(num_cus))


def six_batch_vc_hbm(ctx, kind, is_max, tgtf, vc, leq, eq=None, max_iter=0xFFFFFFFF, out=None):
    """xpg_six_batch_vc_hbm_*: six_batch_vc for shapes of any size. A sign-pattern vc and a shape within 64 KB of LDS: the
    launch six_batch_vc makes; a sign-pattern vc past that: still one launch, a workgroup per LP that normalises, solves and
    finishes on a slot in device memory; anything else per problem as SIX.maxm / minm would. Arrays as six_batch_vc takes
    them. Returns (status[nb], v[nb(,2)], sol[nb, cols(,2)]); `out`: such a triple to write into (rows of sol whose status is
    not 0 are left alone)."""
    return _six_batch_vc(ctx, "six_batch_vc_hbm", kind, is_max, tgtf, vc, leq, eq, max_iter, out)

def six_batch_vc_hbm_last_route():
    """{'lds', 'hbm', 'fallback', 'free', 'grid'}: LPs of this thread's last six_batch_vc_hbm / six_batch_vc_hbm_dev call on the
    LDS-resident kernel / on slots in device memory / solved one by one, the free variables split per LP (-1 after a _dev
    call), and the grid of its launch."""
    return _view("xpg_six_batch_vc_hbm_last_route", ("lds", "hbm", "fallback", "free", "grid"))


SIX_BATCH_VC_HBM_FIELDS = ("route", "nfree", "Rmax", "Vmax", "lds", "slot", "ld", "threads", "grid", "scratch")


def six_batch_vc_hbm_plan(kind, vc, leq_rows, eq_rows, cols, is_max, nb, num_cus=256):
    """xpg_test_six_batch_vc_hbm_plan (host only, no device): what six_batch_vc_hbm does with nb problems of a shape under vc
    [cols - 1, cols(,2)] -- route (0 LDS-resident kernel, 1 device-memory kernel, 2 neither), free variables, the rows and
    variables the largest normal form is solved with, LDS bytes, slot bytes, ld, threads, grid, scratch bytes. vc=None: the
    view of six_batch_vc_hbm_dev, which sizes for every variable free."""
    vc_a = None if vc is None else as_kind(vc, kind, 2)
    return _view("xpg_test_six_batch_vc_hbm_plan", SIX_BATCH_VC_HBM_FIELDS, C.c_int(kind), vp(vc_a), C.c_int(0 if vc_a is None else vc_a.shape[0]),
                 C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(cols), C.c_int(int(is_max)), C.c_int(nb), C.c_int(num_cus))


def six_batch_last_route():
    """Which route the LPs of the calling thread's last six_batch_vc call took (xpg_six_batch_last_route): device = LPs
    reshaped and solved on the device, fallback = LPs solved one by one, free = free variables split per LP on the device
    route (-1 after a _dev call: only the device has read vc)."""
    return _view("xpg_six_batch_last_route", ("device", "fallback", "free"))

def dep_is_empty_batch(ctx, mats, rhs_idx=None, vc=None):
    """DepPoly::is_empty(keepit, vc) (src/eng/poly.cpp:530-573) for a stack of dependence polyhedra
    [nb, rows, cols(,2)]: the constant is column rhs_idx (default: the last), the columns behind it are constant
    symbols (moved to the variables first, Lineq::move2var); vc [rhs_idx, rhs_idx + 1] are the caller's variable
    constraints (default -x_i <= 0). Returns (empty[nb], nodes); -7 where the reference is undefined."""
    mats = as_kind(mats, RAT, 3)
    nb, rows, cols = mats.shape[0], mats.shape[1], mats.shape[2]
    rhs_idx = cols - 1 if rhs_idx is None else rhs_idx
    vc_a = None if vc is None else as_kind(vc, RAT, 2)
    out = np.zeros(nb, dtype=np.int32)
    nodes = C.c_longlong()
    ctx.check(lib().xpg_dep_is_empty_batch_ex_rat32(ctx._h, C.c_int(nb), vp(mats), C.c_int(rows), C.c_int(cols),
                                                    C.c_int(rhs_idx), vp(vc_a), vp(out), C.byref(nodes)),
              "xpg_dep_is_empty_batch_ex_rat32")
    return out, nodes.value


def dep_is_empty_batch_symbols_as_vars(ctx, mats, rhs_idx, vc=None):
    """OPT-IN, NON-PARITY (xpg_dep_is_empty_batch_mode_rat32, XPG_DEP_SYMBOLS_AS_VARS): parametrised dependence polyhedra the
    reference leaves undefined -- the constant symbols behind column rhs_idx become free variables of the widened system.
    Returns (empty[nb], nodes)."""
    mats = as_kind(mats, RAT, 3)
    nb, rows, cols = mats.shape[0], mats.shape[1], mats.shape[2]
    vc_a = None if vc is None else as_kind(vc, RAT, 2)
    out = np.zeros(nb, dtype=np.int32)
    nodes = C.c_longlong()
    ctx.check(lib().xpg_dep_is_empty_batch_mode_rat32(ctx._h, C.c_int(nb), vp(mats), C.c_int(rows), C.c_int(cols), C.c_int(rhs_idx),
                                                      vp(vc_a), C.c_int(1), vp(out), C.byref(nodes)),
              "xpg_dep_is_empty_batch_mode_rat32")
    return out, nodes.value


def has_solution(ctx, leq, eq, vc, rhs_idx, is_int_sol, is_unique_sol):
    """Lineq::has_solution (src/com/linsys.cpp:830-906) on rational systems."""
    vc = as_kind(vc, RAT, 2)
    cols = vc.shape[1]
    leq_rows = 0 if leq is None else len(leq)
    eq_rows = 0 if eq is None else len(eq)
    leq_a = as_kind(leq, RAT, 2) if leq_rows else None
    eq_a = as_kind(eq, RAT, 2) if eq_rows else None
    r = lib().xpg_has_solution_rat32(ctx._h, vp(leq_a), C.c_int(leq_rows), vp(eq_a), C.c_int(eq_rows), vp(vc),
                                     C.c_int(vc.shape[0]), C.c_int(cols), C.c_int(rhs_idx),
                                     C.c_int(int(is_int_sol)), C.c_int(int(is_unique_sol)))
    if r < 0 and r != -7:
        ctx.check(r, "xpg_has_solution_rat32")
    return r


HS_NOT_RUN = 0x7FFFFFFF                  # XPG_HS_NOT_RUN: the solve did not run


def _hs_answers(nb, want_status):
    """(has[nb], status[nb, 2] filled with HS_NOT_RUN, or None)"""
    return np.zeros(nb, dtype=np.int32), np.full((nb, 2), HS_NOT_RUN, dtype=np.int32) if want_status else None


def _hs_front(ctx, leq, eq, vc, want_status):
    """The arguments the two uniform has_solution entry points share, shaped and checked: (ctx .. rhs_idx, has, status)."""
    vc = as_kind(vc, RAT, 2)
    cols = vc.shape[1]
    leq_a = None if leq is None else as_kind(leq, RAT, 3)
    eq_a = None if eq is None else as_kind(eq, RAT, 3)
    if leq_a is None and eq_a is None:
        raise ValueError("leq and eq are both None: the batch size is unknown")
    nb = (leq_a if leq_a is not None else eq_a).shape[0]
    for a in (leq_a, eq_a):
        if a is not None and (a.shape[0] != nb or a.shape[2] != cols):
            raise ValueError("leq / eq must be [nb, rows, cols]")
    rows = 0 if leq_a is None else leq_a.shape[1]
    eq_rows = 0 if eq_a is None else eq_a.shape[1]
    head = (ctx._h, C.c_int(nb), vp(leq_a if rows else None), C.c_int(rows), vp(eq_a if eq_rows else None), C.c_int(eq_rows), vp(vc),
            C.c_int(vc.shape[0]), C.c_int(cols), C.c_int(cols - 1))
    return (head,) + _hs_answers(nb, want_status)


def has_solution_batch(ctx, leq, eq, vc, is_int_sol, is_unique_sol, max_iter=0xFFFFFFFF, want_status=False):
    """Lineq::has_solution for nb rational systems of one shape in one call (xpg_has_solution_batch_rat32): leq [nb, rows,
    cols(,2)], eq [nb, eq_rows, cols(,2)] or None, vc [cols - 1, cols(,2)] shared by the batch; the constant is the last column.
    is_int_sol False: a sign-pattern vc within the batch kernels' limits is answered in ONE launch -- the feasibility objective,
    SIX::normalize once, maxm, then minm where that left the question open -- anything else per system as has_solution does.
    is_int_sol True: two batched MIP walks, the second on the systems the first left open. Returns has[nb] (1 / 0, or the
    negative status a solve returned: -7 where the reference is undefined), and with want_status also status[nb, 2]: the SIX /
    IP status of the maxm and of the minm solve, HS_NOT_RUN for a solve that did not run."""
    head, has, st = _hs_front(ctx, leq, eq, vc, want_status)
    ctx.check(lib().xpg_has_solution_batch_rat32(*head, C.c_int(int(is_int_sol)), C.c_int(int(is_unique_sol)), C.c_uint(max_iter), vp(has),
                                                 vp(st)), "xpg_has_solution_batch_rat32")
    return (has, st) if want_status else has

def has_solution_batch_last_route():
    """{'lds', 'hbm', 'host', 'second', 'grid'}: systems of this thread's last has_solution_batch / has_solution_batch_dev call on
    the LDS-resident kernel / the device-memory kernel / answered per system, the systems whose second solve ran (-1 after a
    _dev call), and the grid of its launch."""
    return _view("xpg_has_solution_batch_last_route", ("lds", "hbm", "host", "second", "grid"))


HAS_SOLUTION_BATCH_FIELDS = ("route", "nfree", "Rmax", "lds", "slot", "ld", "threads", "grid", "scratch")


def has_solution_batch_plan(vc, leq_rows, eq_rows, cols, nb, num_cus=256):
    """xpg_test_has_solution_batch_plan (host only, no device): what has_solution_batch (is_int_sol False) does with nb systems
    of a shape under vc [cols - 1, cols(,2)] -- route (0 LDS-resident kernel, 1 device-memory kernel, 2 neither), free
    variables, rows of the largest tableau of either direction, LDS bytes, slot bytes, ld, threads, grid, scratch bytes.
    vc=None: the view of has_solution_batch_dev, which sizes for every variable free."""
    vc_a = None if vc is None else as_kind(vc, RAT, 2)
    return _view("xpg_test_has_solution_batch_plan", HAS_SOLUTION_BATCH_FIELDS, vp(vc_a), C.c_int(0 if vc_a is None else vc_a.shape[0]),
                 C.c_int(leq_rows), C.c_int(eq_rows), C.c_int(cols), C.c_int(nb), C.c_int(num_cus))


class SIX:
    """Mirror of SIX<Mat,T> (src/com/lpsol.h:204-338): same method names,
    argument order and status codes; `kind` picks the FloatMat or RMat flavour."""

    def __init__(self, ctx, kind):
        self.ctx, self.kind = ctx, kind
        self.max_iter = 0xFFFFFFFF

    def set_param(self, indent, max_iter=0xFFFFFFFF):       # lpsol.h:380-385
        self.max_iter = max_iter

    def _solve(self, is_max, tgtf, vc, eq, leq):
        return _solve_one(self.ctx, "six", self.kind, is_max, tgtf, vc, eq, leq, C.c_uint(self.max_iter))

    def maxm(self, tgtf, vc, eq, leq):                      # lpsol.h:1993-2033
        return self._solve(True, tgtf, vc, eq, leq)

    def minm(self, tgtf, vc, eq, leq):                      # lpsol.h:1662-1732
        return self._solve(False, tgtf, vc, eq, leq)

    def TwoStageMethod(self, leq, tgtf, vc_diag=None, vc_rhs=None):   # lpsol.h:1907-1930
        lp = DeviceLP(self.ctx, self.kind, leq, tgtf, vc_diag, vc_rhs)
        st = lp.two_stage(self.max_iter)
        out = lp.read()
        out["status"] = st
        out["trace"] = lp.trace()
        lp.close()
        return out


# ---- ragged batches: problems of different shapes in one call (include/xpoly_amd.h, "ragged batches") ----------
def _ragged_pack(arrays, kind, ndim):
    """A list of per-problem arrays -> (flat concatenation, cell offsets[nb + 1]); cells are 8 bytes of either kind."""
    parts = [np.ascontiguousarray(as_kind(a, kind, ndim)) for a in arrays]
    cells = [int(np.prod(p.shape[:ndim])) for p in parts]
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    off[1:] = np.cumsum(cells)
    flat = np.concatenate([p.reshape(-1) for p in parts]) if parts else np.zeros(0, dtype=np.float64 if kind == F64 else np.int32)
    return np.ascontiguousarray(flat), off, parts


def six_batch_ragged(ctx, kind, is_max, tgtfs, leqs, max_iter=0xFFFFFFFF):
    """SIX::maxm / minm (x >= 0, inequalities only) on LPs of DIFFERENT shapes in one call: leqs[b] is rows_b x cols_b,
    tgtfs[b] has cols_b entries. Returns (status[nb], [v_b], [sol_b])."""
    nb = len(leqs)
    leq_flat, rows, cols, leq_off, _ = ragged_systems(leqs, kind=kind)
    tg_flat, tg_off, _ = _ragged_pack(tgtfs, kind, 1)
    assert np.array_equal(np.diff(tg_off), cols), "tgtfs[b] must have cols_b entries"
    status = np.zeros(nb, dtype=np.int32)
    v = empty_kind((nb,), kind)
    sol = np.zeros_like(tg_flat)
    ctx.check(_sym("six_batch", kind, "_ragged")(ctx._h, C.c_int(int(is_max)), C.c_int(nb), vp(tg_flat), vp(leq_flat), vp(rows), vp(cols),
                                                 vp(leq_off), vp(tg_off), C.c_uint(max_iter), vp(status), vp(v), vp(sol)),
              "xpg_six_batch_ragged")
    esz = 1 if kind == F64 else 2
    sols = [sol[int(tg_off[b]) * esz: int(tg_off[b + 1]) * esz].reshape((-1,) if kind == F64 else (-1, 2)) for b in range(nb)]
    return status, v, sols


def _hs_ragged_shapes(systems, cols):
    """A list of per-system arrays or None -> the [rows_b, cols(,2)] arrays _ragged_pack takes and rows[nb]."""
    mats = [np.zeros((0, cols, 2), dtype=np.int32) if a is None or len(a) == 0 else as_kind(a, RAT, 2) for a in systems]
    for m in mats:
        if m.shape[1] != cols:
            raise ValueError("every system must have cols = %d columns, got %d" % (cols, m.shape[1]))
    return mats, np.array([m.shape[0] for m in mats], dtype=np.int32)


def _hs_ragged_front(ctx, leqs, eqs, vc, want_status):
    """The arguments the two ragged has_solution entry points share, shaped and checked: (ctx .. rhs_idx, has, status)."""
    vc = as_kind(vc, RAT, 2)
    cols = vc.shape[1]
    nb = len(leqs)
    if eqs is None:
        eqs = [None] * nb
    if len(eqs) != nb:
        raise ValueError("leqs and eqs must list the same systems")
    lm, leq_rows = _hs_ragged_shapes(leqs, cols)
    em, eq_rows = _hs_ragged_shapes(eqs, cols)
    leq_flat, leq_off, _ = _ragged_pack(lm, RAT, 2)
    eq_flat, eq_off, _ = _ragged_pack(em, RAT, 2)
    any_eq = bool(eq_rows.sum())
    head = (ctx._h, C.c_int(nb), vp(leq_flat if leq_rows.sum() else None), vp(leq_rows), vp(leq_off), vp(eq_flat if any_eq else None),
            vp(eq_rows), vp(eq_off if any_eq else None), vp(vc), C.c_int(vc.shape[0]), C.c_int(cols), C.c_int(cols - 1))
    return (head,) + _hs_answers(nb, want_status)


def has_solution_ragged(ctx, leqs, eqs, vc, is_int_sol, is_unique_sol, max_iter=0xFFFFFFFF, want_status=False):
    """Lineq::has_solution for rational systems of MIXED shapes under one vc in one call
    (xpg_has_solution_batch_ragged_rat32): leqs[b] [rows_b, cols(,2)] and eqs[b] [eq_rows_b, cols(,2)], either None or without
    rows; eqs=None: no system has equalities. Every system takes the route has_solution_batch takes for its shape -- the systems
    of a route share ONE launch -- and gets that call's answers. Returns has[nb], and with want_status also status[nb, 2]."""
    head, has, st = _hs_ragged_front(ctx, leqs, eqs, vc, want_status)
    ctx.check(lib().xpg_has_solution_batch_ragged_rat32(*head, C.c_int(int(is_int_sol)), C.c_int(int(is_unique_sol)), C.c_uint(max_iter),
                                                        vp(has), vp(st)), "xpg_has_solution_batch_ragged_rat32")
    return (has, st) if want_status else has

HAS_SOLUTION_RAGGED_ROUTE_FIELDS = ("lds", "hbm", "host", "second", "grid_lds", "grid_hbm", "no_solve")


def has_solution_ragged_last_route():
    """{'lds', 'hbm', 'host', 'second', 'grid_lds', 'grid_hbm', 'no_solve'}: systems of this thread's last has_solution_ragged
    call on the LDS-resident kernel / the device-memory kernel / answered per system, the systems whose second solve ran, the
    grids of the two launches (0 without one), the systems answered without a solve."""
    return _view("xpg_has_solution_batch_ragged_last_route", HAS_SOLUTION_RAGGED_ROUTE_FIELDS)


HAS_SOLUTION_RAGGED_FIELDS = ("lds_count", "lds_lds", "lds_threads", "lds_slot", "lds_grid",
                              "hbm_count", "hbm_lds", "hbm_slot", "hbm_Rmax", "hbm_ld", "hbm_threads", "hbm_grid")


def has_solution_ragged_plan(vc, leq_rows, eq_rows, num_cus=256):
    """xpg_test_has_solution_batch_ragged_plan (host only, no device): what has_solution_ragged (is_int_sol False) does with
    systems of leq_rows[b] inequalities and eq_rows[b] equalities under vc [cols - 1, cols(,2)]. Returns (route[nb] -- 0
    LDS-resident kernel, 1 device-memory kernel, 2 per system, 3 without inequalities --, the two launches' sizes under
    HAS_SOLUTION_RAGGED_FIELDS)."""
    vc_a = as_kind(vc, RAT, 2)
    lr = np.ascontiguousarray(leq_rows, dtype=np.int32); er = np.ascontiguousarray(eq_rows, dtype=np.int32)
    if lr.shape != er.shape or lr.ndim != 1:
        raise ValueError("leq_rows and eq_rows must list the same systems")
    route = np.zeros(len(lr), dtype=np.int32)
    sizes = _view("xpg_test_has_solution_batch_ragged_plan", HAS_SOLUTION_RAGGED_FIELDS, vp(vc_a), C.c_int(vc_a.shape[0]), C.c_int(vc_a.shape[1]),
                  C.c_int(len(lr)), vp(lr), vp(er), C.c_int(num_cus), vp(route))
    return route, sizes


def has_solution_int_batch(ctx, leq, eq, vc, is_unique_sol, want_status=False):
    """Lineq::has_solution(..., is_int_sol=True, is_unique_sol) for nb rational systems of one shape in one call that
    synchronises once (xpg_has_solution_int_batch_rat32): the arrays of has_solution_batch; the feasibility objective, both MIP
    walks and the verdict run on the device wherever vc is a sign pattern and the shape is within the walks' limits, anything
    else as has_solution_batch(is_int_sol=True) answers it. Returns has[nb], and with want_status also status[nb, 2] -- bit for
    bit what has_solution_batch(..., True, is_unique_sol) returns."""
    head, has, st = _hs_front(ctx, leq, eq, vc, want_status)
    ctx.check(lib().xpg_has_solution_int_batch_rat32(*head, C.c_int(int(is_unique_sol)), vp(has), vp(st)), "xpg_has_solution_int_batch_rat32")
    return (has, st) if want_status else has

def has_solution_int_ragged(ctx, leqs, eqs, vc, is_unique_sol, want_status=False):
    """has_solution_int_batch for systems of MIXED shapes under one vc (xpg_has_solution_int_batch_ragged_rat32): the lists of
    has_solution_ragged; the shape classes are formed by the library, each answered by the uniform call, the answers come back
    in the order given. Returns has[nb], and with want_status also status[nb, 2]."""
    head, has, st = _hs_ragged_front(ctx, leqs, eqs, vc, want_status)
    ctx.check(lib().xpg_has_solution_int_batch_ragged_rat32(*head, C.c_int(int(is_unique_sol)), vp(has), vp(st)),
              "xpg_has_solution_int_batch_ragged_rat32")
    return (has, st) if want_status else has

HAS_SOLUTION_INT_ROUTE_FIELDS = ("lds", "hbm", "host", "second", "grid", "grid2")


def has_solution_int_last_route():
    """{'lds', 'hbm', 'host', 'second', 'grid', 'grid2'}: systems of this thread's last has_solution_int_batch /
    has_solution_int_ragged call on the LDS-resident walk / the device-memory kernel / answered by has_solution_batch, the
    systems whose second walk ran, the grid of the maxm pass (or of the one device-memory launch) and of the LDS-resident minm
    pass. After a ragged call: counts summed over the classes, the largest grids."""
    return _view("xpg_has_solution_int_batch_last_route", HAS_SOLUTION_INT_ROUTE_FIELDS)


HAS_SOLUTION_INT_FIELDS = ("route", "free", "rmax", "lds_max", "lds_min", "threads_max", "threads_min", "grid_max", "grid_min",
                           "help_max", "help_min", "slot", "ld_max", "ld_min", "ws_words", "obj_word", "scratch")


def has_solution_int_plan(vc, leq_rows, eq_rows, cols, nb, num_cus=256):
    """xpg_test_has_solution_int_plan (host only, no device): what has_solution_int_batch does with nb systems of a shape under
    vc [cols - 1, cols(,2)] -- route (0 LDS-resident walk twice, 1 device-memory kernel, 2 has_solution_batch's composition),
    free variables, rows of the largest node LP, and per direction (_max: the maxm walk, _min: the minm walk) LDS bytes, threads,
    grid, helper workgroups and ld; bytes of one tableau slot, workspace words, the word the objective starts at, scratch bytes."""
    vc_a = as_kind(vc, RAT, 2)
    return _view("xpg_test_has_solution_int_plan", HAS_SOLUTION_INT_FIELDS, vp(vc_a), C.c_int(vc_a.shape[0]), C.c_int(leq_rows),
                 C.c_int(eq_rows), C.c_int(cols), C.c_int(nb), C.c_int(num_cus))


def ragged_pack_rat(mats_list):
    """(flat cells, rows[nb], cols[nb], cell offsets[nb + 1]) of a list of rational systems: the arrays the ragged C entry points take."""
    return ragged_systems(mats_list)[:4]


def ragged_systems(mats_list, rhs_idx=None, kind=RAT):
    """The one pack of a list of systems of mixed shapes: (flat cells, rows[nb], cols[nb], cell offsets[nb + 1], rhs) with rhs
    the per-system rhs_idx as a flat int32 array, or None (every system's last column). Whoever takes an rhs_idx checks its
    count against what it is one of -- systems, groups or members -- under its own message."""
    flat, off, parts = _ragged_pack(mats_list, kind, 2)
    rows = np.array([p.shape[0] for p in parts], dtype=np.int32); cols = np.array([p.shape[1] for p in parts], dtype=np.int32)
    rhs = None if rhs_idx is None else np.ascontiguousarray(rhs_idx, dtype=np.int32).reshape(-1)
    return flat, rows, cols, off, rhs


def dep_is_empty_ragged(ctx, mats_list=None, packed=None):
    """DepPoly::is_empty (src/eng/poly.cpp:530-573) on dependence polyhedra of mixed shapes (constant in the last
    column of each): (empty[nb], nodes). `packed` = ragged_pack_rat(...) of the list, for callers that keep it."""
    flat, rows, cols, off = packed if packed is not None else ragged_pack_rat(mats_list)
    nb = len(rows)
    out = np.zeros(nb, dtype=np.int32)
    nodes = C.c_longlong()
    ctx.check(lib().xpg_dep_is_empty_batch_ragged_rat32(ctx._h, C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off), vp(out),
                                                        C.byref(nodes)), "xpg_dep_is_empty_batch_ragged_rat32")
    return out, nodes.value
