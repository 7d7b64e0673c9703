"""Python face of the row-elimination entry points, shaped after xpoly's Lineq
(src/com/linsys.h:61-186) and Matrix<Rational> (src/com/matt.h). Batched: every
call takes a stack of equally shaped systems [nb, rows, cols, 2] (int32 num/den)
and runs one wavefront per system on the GPU.
"""
import ctypes as C
import math

import numpy as np

from ._capi import lib, vp
from .six import RAT, _view, as_kind, ragged_systems


def _stack(mats):
    """One system [rows, cols, 2] or a stack [nb, rows, cols, 2] of (num, den) pairs. Integer systems
    are converted explicitly by the caller (xpoly_amd.six.as_kind(a, RAT, ndim)), never guessed."""
    a = np.asarray(mats)
    if a.ndim not in (3, 4) or a.shape[-1] != 2 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError("Lineq takes (num, den) pairs [rows, cols, 2] or [nb, rows, cols, 2], got %s %s" % (a.dtype, a.shape))
    a = as_kind(a, RAT, a.ndim - 1)
    if a.ndim == 3:
        a = a[None]
    return np.ascontiguousarray(a)


def _rows_down(view, total, cell, copy):
    """The `total` rows a packed call left behind its view pointer, as an int32 array [total, *cell] -- cell (cols, 2) for rows of
    one width, (2,) for cells of mixed widths. The one place that reads the handle's pinned buffer. That buffer is the handle's:
    its next packed call writes it again. copy=True takes the rows out before that can happen; copy=False hands out a view that
    is valid only until then (what a C++ caller reads its results from). No rows: always an owned, empty array, never a view of a
    pointer the library may not have set."""
    shape = (total,) + cell
    if total and not copy:
        return np.frombuffer((C.c_int32 * math.prod(shape)).from_address(view.value), dtype=np.int32).reshape(shape)
    rows = np.empty(shape, dtype=np.int32)
    if total:
        C.memmove(rows.ctypes.data, view.value, rows.nbytes)
    return rows


def _cut(packed, off, widths=None):
    """[result r] of a packed readout: rows off[r] .. off[r + 1], or with widths (ragged) those cells as rows of widths[r] columns
    (a width of 0: a result of no rows and no columns)."""
    o = off.tolist()
    if widths is None:
        return [packed[a: b] for a, b in zip(o, o[1:])]
    return [packed[a: b].reshape((b - a) // w if w else 0, w, 2) for a, b, w in zip(o, o[1:], widths)]


def _nest(results, first):
    """[[the results first[b] .. first[b + 1] of system b]]"""
    return [results[a: b] for a, b in zip(first, first[1:])]


def _every(n, nb):
    """first[] of nb systems with n results each (n may be 0)"""
    return [b * n for b in range(nb + 1)]


def _flat_lists(lists):
    """Elimination lists as the ragged entry points take them: (all entries in one int32 array, offsets[len(lists) + 1]).
    Without any entry the array is one zero: the library is never handed a pointer to nothing."""
    lists = [np.asarray(e, dtype=np.int32).reshape(-1) for e in lists]
    eoff = np.zeros(len(lists) + 1, dtype=np.int32)
    eoff[1:] = np.cumsum([e.size for e in lists])
    return np.ascontiguousarray(np.concatenate(lists)) if int(eoff[-1]) else np.zeros(1, dtype=np.int32), eoff


class Lineq:
    def __init__(self, ctx):
        self.ctx = ctx

    def reduce(self, mats, rhs_idx, is_intersect=True):
        """Lineq::reduce (linsys.cpp:359-626). Returns (ok[nb], [system b's surviving rows]) -- through the packed entry
        point; the rows are slices of one array."""
        ok, off, packed = self.reduce_packed(mats, rhs_idx, is_intersect)
        return ok, _cut(packed, off)

    def reduce_packed(self, mats, rhs_idx, is_intersect=True, copy=True):
        """xpg_lineq_reduce_batch_packed_rat32: (ok[nb], row_offsets[nb + 1], rows[row_offsets[nb], cols, 2]); the input is
        not modified. copy=False returns the rows as a view of the handle's pinned buffer (valid until the handle's next
        packed call): what a C++ caller reads its results from."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        off = np.zeros(nb + 1, dtype=np.int64); ok = np.zeros(nb, dtype=np.int32)
        view = C.c_void_p()
        self.ctx.check(lib().xpg_lineq_reduce_batch_packed_rat32(
            self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), C.c_int(rhs_idx), C.c_int(int(is_intersect)),
            None, C.c_longlong(0), C.byref(view), vp(off), None, vp(ok)), "xpg_lineq_reduce_batch_packed_rat32")
        return ok, off, _rows_down(view, int(off[nb]), (cols, 2), copy)

    def reduce_inplace(self, mats, rhs_idx, is_intersect=True):
        """xpg_lineq_reduce_batch_rat32, the in-place form of the reference's signature: `mats` [nb, rows, cols, 2] (int32,
        contiguous) is overwritten -- system b's surviving rows at the front of its slot. Returns (ok[nb], out_rows[nb])."""
        a = mats
        assert isinstance(a, np.ndarray) and a.dtype == np.int32 and a.ndim == 4 and a.flags.c_contiguous
        nb, rows, cols = a.shape[:3]
        out_rows = np.zeros(nb, dtype=np.int32); ok = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_lineq_reduce_batch_rat32(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols),
                                                          C.c_int(rhs_idx), C.c_int(int(is_intersect)), vp(out_rows), vp(ok)),
                       "xpg_lineq_reduce_batch_rat32")
        return ok, out_rows

    def move2var(self, mats, rhs_idx, first_sym, last_sym):
        """Lineq::move2var (linsys.cpp:1177-1200): constant symbols become variables in front of the constant."""
        a = _stack(mats).copy()
        nb, rows, cols = a.shape[:3]
        self.ctx.check(lib().xpg_lineq_move2var_batch_rat32(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols),
                                                            C.c_int(rhs_idx), C.c_int(first_sym), C.c_int(last_sym)),
                       "xpg_lineq_move2var_batch_rat32")
        return a

    def removeIdenRow(self, mats):
        """Lineq::removeIdenRow (linsys.cpp:1209-1268)."""
        a = _stack(mats).copy()
        nb, rows, cols = a.shape[:3]
        out_rows = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_lineq_remove_iden_batch_rat32(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows),
                                                               C.c_int(cols), vp(out_rows)),
                       "xpg_lineq_remove_iden_batch_rat32")
        return [a[b, : out_rows[b]].copy() for b in range(nb)]

    def fme(self, mats, rhs_idx, u, darkshadow=False, cap_rows=None, slots=False):
        """Lineq::fme (linsys.cpp:656-774). Returns (ok[nb], [result of system b]). Through the packed entry point
        (row offsets + live rows only); slots=True takes the cap_rows-slot entry point instead (A/B, tests)."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        if slots:
            cap = cap_rows or max(rows, rows * rows // 4 + rows + 1)
            outs = np.zeros((nb, cap, cols, 2), dtype=np.int32)
            out_rows = np.zeros(nb, dtype=np.int32); ok = np.zeros(nb, dtype=np.int32)
            self.ctx.check(lib().xpg_lineq_fme_batch_rat32(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols),
                                                           C.c_int(rhs_idx), C.c_int(u), C.c_int(int(darkshadow)), vp(outs),
                                                           C.c_int(cap), vp(out_rows), vp(ok)),
                           "xpg_lineq_fme_batch_rat32")
            if (out_rows < 0).any():
                raise ValueError("fme result needs %d rows, cap_rows is %d" % (-out_rows.min(), cap))
            return ok, [outs[b, : out_rows[b]].copy() for b in range(nb)]
        ok, off, packed = self.fme_packed(a, rhs_idx, u, darkshadow, cap_rows)
        return ok, _cut(packed, off)

    def fme_packed(self, mats, rhs_idx, u, darkshadow=False, cap_rows=None, copy=True):
        """xpg_lineq_fme_batch_packed_rat32: (ok[nb], row_offsets[nb + 1], rows[row_offsets[nb], cols, 2]).
        copy=False returns the rows as a view of the handle's pinned buffer, valid until the next packed call
        on this handle (what a C++ caller reads its results from)."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        off = np.zeros(nb + 1, dtype=np.int64); ok = np.zeros(nb, dtype=np.int32)
        view = C.c_void_p()
        self.ctx.check(lib().xpg_lineq_fme_batch_packed_rat32(
            self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), C.c_int(rhs_idx), C.c_int(u),
            C.c_int(int(darkshadow)), C.c_int(cap_rows or 0), None, C.c_longlong(0), C.byref(view), vp(off), vp(ok)),
            "xpg_lineq_fme_batch_packed_rat32")
        return ok, off, _rows_down(view, int(off[nb]), (cols, 2), copy)

    def _chain_packed(self, levels, mats, rhs_idx, elim, darkshadow, cap_rows, cap_out_rows, copy):
        """xpg_lineq_{project,levels}_batch_packed_rat32: (ok[nb], steps[nb], results) with one result per system, or (levels)
        one per system and list entry -- level k of system b at b * len(elim) + k."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        el = np.ascontiguousarray(elim, dtype=np.int32).reshape(-1)
        n = int(el.size)
        off = np.zeros((nb * n if levels else nb) + 1, dtype=np.int64); ok = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
        if nb == 0:
            return ok, steps, []
        name = "xpg_lineq_%s_batch_packed_rat32" % ("levels" if levels else "project")
        view = C.c_void_p()
        self.ctx.check(getattr(lib(), name)(
            self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), C.c_int(rhs_idx), vp(el), C.c_int(n),
            C.c_int(int(darkshadow)), C.c_int(cap_rows or 0), C.c_int(cap_out_rows or 0), None, C.c_longlong(0), C.byref(view),
            vp(off), vp(ok), vp(steps)), name)
        res = _cut(_rows_down(view, int(off[-1]), (cols, 2), copy), off)
        return ok, steps, _nest(res, _every(n, nb)) if levels else res

    def project_packed(self, mats, rhs_idx, elim, darkshadow=False, cap_rows=None, cap_out_rows=None, copy=True):
        """xpg_lineq_project_batch_packed_rat32: the variables of `elim` eliminated one after the other (each Lineq::fme's result
        the next one's input) in one launch. Returns (ok[nb], steps[nb], [rows of system b]): ok 1 with steps == len(elim), 0
        with the step that found the system inconsistent, or -need with the step that needs `need` rows (steps == len(elim):
        the final result against cap_out_rows); a system with ok <= 0 has no rows. copy=False: the rows are views of the
        handle's pinned buffer, valid until the next packed call on this handle."""
        return self._chain_packed(False, mats, rhs_idx, elim, darkshadow, cap_rows, cap_out_rows, copy)

    PROJECT_ROUTE_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes")

    @staticmethod
    def project_last_route():
        """xpg_lineq_project_last_route of the calling thread's last projection call, as a dict."""
        return _view("xpg_lineq_project_last_route", Lineq.PROJECT_ROUTE_KEYS)

    def levels_packed(self, mats, rhs_idx, elim, darkshadow=False, cap_rows=None, cap_out_rows=None, copy=True):
        """xpg_lineq_levels_batch_packed_rat32: the projection that keeps every level -- the variables of `elim` eliminated one
        after the other in one launch, the rows after EACH step kept (loop-nest limits, LoopTran::transformIterSpace). Returns
        (ok[nb], steps[nb], levels) with levels[b][k] the rows of system b once elim[0 .. k] are eliminated: ok 1 with steps ==
        len(elim), 0 with the step that found the system inconsistent, or -need with the step k concerned -- need > cap_rows:
        step k's unreduced result needs `need` rows; else level k has `need` > cap_out_rows rows. A system with ok <= 0 has no
        rows at any level. copy=False: the levels are views of the handle's pinned buffer, valid until the next packed call."""
        return self._chain_packed(True, mats, rhs_idx, elim, darkshadow, cap_rows, cap_out_rows, copy)

    @staticmethod
    def levels_last_route():
        """xpg_lineq_levels_last_route of the calling thread's last levels call, as a dict."""
        return _view("xpg_lineq_levels_last_route", Lineq.PROJECT_ROUTE_KEYS + ("level_bytes",))

    def transform_levels_packed(self, mats, tmats, rhs_idx, mode=0, shared_nest=False, cap_rows=None, cap_out_rows=None, copy=True):
        """xpg_lineq_transform_levels_batch_packed_rat32: the limits of transformed loop nests in one launch
        (LoopTran::transformIterSpace, src/eng/ldtran.cpp:131-300). tmats [nb, n, n, 2] with n = rhs_idx; mats one nest per
        transformation [nb, rows, cols, 2], or with shared_nest ONE nest [rows, cols, 2] for all of them. mode 0: tmats are
        the transformations T (det, T^-1); mode 1: they are the right multipliers M themselves. Returns (ok[nb], steps[nb],
        kind[nb], det[nb, 2], mult[nb, n, n, 2], levels): kind 0 with levels[b][0] = (A * M | C) and levels[b][k] that system
        with rhs_idx-1 .. rhs_idx-k eliminated, under levels_packed's verdicts; kind 1 (T singular) or 2 (|det| != 1) with no
        rows at any level, ok 1 and steps 0. det is None in mode 1. copy=False: the levels are views of the handle's pinned
        buffer, valid until the next packed call."""
        a, t = _stack(mats), _stack(tmats)
        nb, n = t.shape[0], int(rhs_idx)
        rows, cols = a.shape[1:3]
        if t.shape[1:3] != (n, n) or a.shape[0] != (1 if shared_nest else nb):
            raise ValueError("transformations [nb, %d, %d, 2] and %s, got %s and %s"
                             % (n, n, "one nest" if shared_nest else "one nest each", t.shape, a.shape))
        off = np.zeros(nb * n + 1, dtype=np.int64)
        ok, steps, kind = (np.zeros(nb, dtype=np.int32) for _ in range(3))
        det = np.zeros((nb, 2), dtype=np.int32) if mode == 0 else None
        mult = np.zeros((nb, n, n, 2), dtype=np.int32)
        if nb == 0:
            return ok, steps, kind, det, mult, []
        view = C.c_void_p()
        self.ctx.check(lib().xpg_lineq_transform_levels_batch_packed_rat32(
            self.ctx._h, C.c_int(nb), vp(a), C.c_int(int(shared_nest)), vp(t), C.c_int(rows), C.c_int(cols), C.c_int(n), C.c_int(mode),
            C.c_int(cap_rows or 0), C.c_int(cap_out_rows or 0), None, C.c_longlong(0), C.byref(view), vp(off), vp(ok), vp(steps),
            vp(kind), vp(det), vp(mult)), "xpg_lineq_transform_levels_batch_packed_rat32")
        res = _cut(_rows_down(view, int(off[-1]), (cols, 2), copy), off)
        return ok, steps, kind, det, mult, _nest(res, _every(n, nb))

    @staticmethod
    def transform_last_route():
        """xpg_lineq_transform_last_route of the calling thread's last transformed-nest call, as a dict."""
        return _view("xpg_lineq_transform_last_route", Lineq.PROJECT_ROUTE_KEYS + ("level_bytes",))

    def _chain_ragged(self, levels, mats_list, rhs_idx, elims, darkshadow, cap_rows, cap_out_rows, copy):
        """xpg_lineq_{project,levels}_batch_ragged_rat32: (ok[nb], steps[nb], results) with results[r] the rows of result r --
        one per system, or (levels) one per list entry, level k of system b at elim_offsets[b] + k -- and the offsets of the
        lists. The rows are cols[b] wide."""
        flat, rows, cols, off, rhs = ragged_systems(mats_list, rhs_idx)
        nb = len(rows)
        if elims is None:                                   # loop-nest limits: rhs_idx - 1 .. 1 of each system
            elims = [list(range(int(r) - 1, 0, -1)) for r in (rhs if rhs is not None else cols - 1)]
        if len(elims) != nb or (rhs is not None and rhs.size != nb):
            raise ValueError("one list and one rhs_idx per system: %d systems, %d lists" % (nb, len(elims)))
        el, eoff = _flat_lists(elims)
        nres = int(eoff[nb]) if levels else nb
        ooff = np.zeros(nres + 1, dtype=np.int64); orows = np.zeros(max(nres, 1), dtype=np.int32)
        ok = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
        if nb == 0:
            return ok, steps, [], eoff
        name = "xpg_lineq_levels_batch_ragged_rat32" if levels else "xpg_lineq_project_batch_ragged_rat32"
        view = C.c_void_p()
        self.ctx.check(getattr(lib(), name)(
            self.ctx._h, C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off), vp(rhs), vp(el), vp(eoff), C.c_int(int(darkshadow)),
            C.c_int(cap_rows or 0), C.c_int(cap_out_rows or 0), None, C.c_longlong(0), C.byref(view), vp(ooff), vp(orows), vp(ok),
            vp(steps)), name)
        width = np.repeat(cols, np.diff(eoff)).tolist() if levels else cols.tolist()
        return ok, steps, _cut(_rows_down(view, int(ooff[nres]), (2,), copy), ooff, width), eoff

    def project_ragged(self, mats_list, rhs_idx, elims, darkshadow=False, cap_rows=None, cap_out_rows=None, copy=True):
        """xpg_lineq_project_batch_ragged_rat32: Lineq.project_packed for systems of DIFFERENT shapes, each with its own
        rhs_idx[b] (None: its last column) and its own list elims[b], in ONE launch. Returns (ok[nb], steps[nb], [rows of system
        b]) with project_packed's verdicts; the capacities are the call's -- cap_rows defaults to fme's worst case for the system
        with the most rows. copy=False: views of the handle's pinned buffer, valid until the next packed call on this handle."""
        ok, steps, res, _ = self._chain_ragged(False, mats_list, rhs_idx, elims, darkshadow, cap_rows, cap_out_rows, copy)
        return ok, steps, res

    def levels_ragged(self, mats_list, rhs_idx, elims=None, darkshadow=False, cap_rows=None, cap_out_rows=None, copy=True):
        """xpg_lineq_levels_batch_ragged_rat32: Lineq.levels_packed for systems of DIFFERENT shapes and depths in ONE launch --
        the loop-nest limits of a SCoP's statements. elims None: the list rhs_idx[b]-1 .. 1 of each system, as
        LoopTran::transformIterSpace runs it. Returns (ok[nb], steps[nb], levels) with levels[b][k] the rows of system b once
        elims[b][0 .. k] are eliminated, and levels_packed's verdicts."""
        ok, steps, res, eoff = self._chain_ragged(True, mats_list, rhs_idx, elims, darkshadow, cap_rows, cap_out_rows, copy)
        return ok, steps, _nest(res, eoff.tolist())

    @staticmethod
    def ragged_last_route():
        """xpg_lineq_ragged_last_route of the calling thread's last project_ragged / levels_ragged call, as a dict."""
        return _view("xpg_lineq_ragged_last_route", Lineq.PROJECT_ROUTE_KEYS + ("out_bytes",))

    def reduce_ragged(self, mats_list, rhs_idx=None, is_intersect=True):
        """Lineq::reduce on systems of different shapes in one call: (ok[nb], [system b's surviving rows])."""
        flat, rows, cols, off, rhs = ragged_systems(mats_list, rhs_idx)
        nb = len(rows)
        out_rows = np.zeros(nb, dtype=np.int32); ok = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_lineq_reduce_batch_ragged_rat32(self.ctx._h, C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off),
                                                                 vp(rhs), C.c_int(int(is_intersect)), vp(out_rows), vp(ok)),
                       "xpg_lineq_reduce_batch_ragged_rat32")
        return ok, [flat[2 * int(off[b]): 2 * int(off[b]) + 2 * int(out_rows[b]) * int(cols[b])].reshape(int(out_rows[b]), int(cols[b]), 2).copy()
                    for b in range(nb)]

    RAGGED_FME_ONE_CALL_BYTES = 256 << 20

    def fme_ragged(self, mats_list, u, rhs_idx=None, darkshadow=False):
        """Lineq::fme on systems of different shapes, eliminating variable u[b] of system b: (ok[nb], [result b])."""
        flat, rows, cols, off, rhs = ragged_systems(mats_list, rhs_idx)
        nb = len(rows)
        uu = np.ascontiguousarray(u, dtype=np.int32)
        out_rows = np.zeros(nb, dtype=np.int32); ok = np.zeros(nb, dtype=np.int32); ooff = np.zeros(nb + 1, dtype=np.int64)
        # ONE call where the worst case is small: the entry point computes every elimination before it looks at the output
        # buffer, so a sizing call does the whole batch twice. An elimination of R rows leaves at most R*R/4 + R rows (P
        # positive x N negative combinations with P + N <= R, plus the rows without the variable): the buffer is sized for
        # that and trimmed. Above 256 MB of worst case (large batches: several GB of zero pages that raise MemoryError where
        # the real result fits easily) the sizing call is the cheaper evil: the first call returns XPG_ERR_SHAPE with the
        # offsets filled (include/xpoly_amd.h), the second gets a buffer of exactly that size.
        capc = int(sum((int(r) * int(r) // 4 + int(r)) * int(c) for r, c in zip(rows, cols)))

        def call(buf, cap_cells):
            return lib().xpg_lineq_fme_batch_ragged_rat32(
                self.ctx._h, C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off), vp(rhs), vp(uu), C.c_int(int(darkshadow)), vp(buf),
                C.c_longlong(cap_cells), vp(ooff), vp(out_rows), vp(ok))

        if capc * 8 <= self.RAGGED_FME_ONE_CALL_BYTES:
            outs = np.zeros((max(capc, 1), 2), dtype=np.int32)
            self.ctx.check(call(outs, capc), "xpg_lineq_fme_batch_ragged_rat32")
        else:
            rc = call(None, 0)
            # XPG_ERR_SHAPE from a sizing call means "too small, offsets filled" -- or malformed input (cols > 255, u out of
            # range, a bad rhs_idx), refused before any offset is written: told apart by whether anything was filled in
            if rc != -3 or not (int(ooff[nb]) > 0 or out_rows.any()):
                self.ctx.check(rc, "xpg_lineq_fme_batch_ragged_rat32 (sizing)")
            need = int(ooff[nb])
            outs = np.zeros((max(need, 1), 2), dtype=np.int32)
            if need:
                self.ctx.check(call(outs, need), "xpg_lineq_fme_batch_ragged_rat32")
        return ok, [outs[int(ooff[b]): int(ooff[b + 1])].reshape(int(out_rows[b]), int(cols[b]), 2).copy() for b in range(nb)]

    def calcBound(self, mats, rhs_idx, cap_rows=None):
        """Lineq::calcBound (linsys.cpp:1047-1078): chained eliminations on the device.
        Returns (ok[nb], bounds[b][j] = rows x cols x 2 array bounding variable j alone)."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        cap = cap_rows or max(16, rows * rows)
        out = np.zeros((nb, rhs_idx, cap, cols, 2), dtype=np.int32)
        out_rows = np.zeros((nb, rhs_idx), dtype=np.int32); ok = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_lineq_calc_bound_batch_rat32(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols),
                                                              C.c_int(rhs_idx), C.c_int(cap), vp(out), vp(out_rows), vp(ok)),
                       "xpg_lineq_calc_bound_batch_rat32")
        return ok, [[out[b, j, : max(out_rows[b, j], 0)].copy() for j in range(rhs_idx)] for b in range(nb)]

    def calcBound_packed(self, mats, rhs_idx, cap_rows=None):
        """The same through the packed entry point (xpg_lineq_calc_bound_batch_packed_rat32): only live rows cross the link.
        Returns (ok[nb], bounds[b][j]) like calcBound; ok[b] < 0 (a step needed -ok[b] rows) leaves every bound empty."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        off = np.zeros(nb * rhs_idx + 1, dtype=np.int64); ok = np.zeros(nb, dtype=np.int32)
        view = C.c_void_p()
        self.ctx.check(lib().xpg_lineq_calc_bound_batch_packed_rat32(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols),
                                                                     C.c_int(rhs_idx), C.c_int(cap_rows or 0), None, C.c_longlong(0),
                                                                     C.byref(view), vp(off), vp(ok)),
                       "xpg_lineq_calc_bound_batch_packed_rat32")
        res = [r.copy() for r in _cut(_rows_down(view, int(off[-1]), (cols, 2), True), off)]
        return ok, _nest(res, _every(rhs_idx, nb))

    def bounds_packed(self, mats, rhs_idx, cap_rows=0, cap_out_rows=0, copy=True):
        """xpg_lineq_bounds_batch_packed_rat32: Lineq::calcBound for every system in one launch. Returns (ok[nb], chain[nb],
        steps[nb], bounds[b][j]): ok 1 with chain -1, or the verdict of the lowest failing chain -- 0 (step `steps` of chain
        `chain` found the system inconsistent) or -need (that step needs `need` rows; steps == rhs_idx - 1: the chain's result
        against cap_out_rows). A system with ok <= 0 has every bound empty, the others are packed all the same. copy=False: the
        bounds are views of the handle's pinned buffer, valid until the next packed call on this handle."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        nres = nb * rhs_idx
        off = np.zeros(max(nres, 0) + 1, dtype=np.int64)
        ok = np.zeros(nb, dtype=np.int32); chain = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
        if nb == 0:
            return ok, chain, steps, []
        view = C.c_void_p()
        self.ctx.check(lib().xpg_lineq_bounds_batch_packed_rat32(
            self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), C.c_int(rhs_idx), C.c_int(cap_rows or 0),
            C.c_int(cap_out_rows or 0), None, C.c_longlong(0), C.byref(view), vp(off), vp(ok), vp(chain), vp(steps)),
            "xpg_lineq_bounds_batch_packed_rat32")
        res = _cut(_rows_down(view, int(off[-1]), (cols, 2), copy), off)
        return ok, chain, steps, _nest(res, _every(rhs_idx, nb))

    @staticmethod
    def bounds_last_route():
        """xpg_lineq_bounds_last_route of the calling thread's last fused calcBound call, as a dict."""
        return _view("xpg_lineq_bounds_last_route", Lineq.PROJECT_ROUTE_KEYS + ("steps",))

    def bounds_ragged(self, mats_list, rhs_idx=None, cap_rows=None, cap_out_rows=None, copy=True):
        """xpg_lineq_bounds_batch_ragged_rat32: Lineq.bounds_packed for systems of DIFFERENT shapes, each with its own rhs_idx[b]
        (None: its last column), in ONE launch -- the bounds of every variable of a SCoP's statements. Returns (ok[nb], chain[nb],
        steps[nb], bounds) with bounds[b][j] the rows x cols[b] x 2 bounds of variable j of system b and bounds_packed's verdicts;
        the capacities are the call's -- cap_rows defaults to 4 * (most rows) + 16. copy=False: views of the handle's pinned
        buffer, valid until the next packed call on this handle."""
        flat, rows, cols, off, rhs = ragged_systems(mats_list, rhs_idx)
        nb = len(rows)
        if rhs is not None and rhs.size != nb:
            raise ValueError("one rhs_idx per system: %d systems, %d rhs_idx" % (nb, rhs.size))
        first = np.zeros(nb + 1, dtype=np.int64)
        first[1:] = np.cumsum(rhs if rhs is not None else cols - 1)
        nres = max(int(first[nb]), 0)
        ooff = np.zeros(nres + 1, dtype=np.int64); orows = np.zeros(max(nres, 1), dtype=np.int32)
        ok = np.zeros(nb, dtype=np.int32); chain = np.zeros(nb, dtype=np.int32); steps = np.zeros(nb, dtype=np.int32)
        if nb == 0:
            return ok, chain, steps, []
        view = C.c_void_p()
        self.ctx.check(lib().xpg_lineq_bounds_batch_ragged_rat32(
            self.ctx._h, C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off), vp(rhs), C.c_int(cap_rows or 0), C.c_int(cap_out_rows or 0),
            None, C.c_longlong(0), C.byref(view), vp(ooff), vp(orows), vp(ok), vp(chain), vp(steps)),
            "xpg_lineq_bounds_batch_ragged_rat32")
        width = np.repeat(cols, np.diff(first)).tolist()
        return ok, chain, steps, _nest(_cut(_rows_down(view, int(ooff[nres]), (2,), copy), ooff, width), first.tolist())

    @staticmethod
    def bounds_ragged_last_route():
        """xpg_lineq_bounds_ragged_last_route of the calling thread's last bounds_ragged call, as a dict."""
        return _view("xpg_lineq_bounds_ragged_last_route", Lineq.PROJECT_ROUTE_KEYS + ("out_bytes", "steps"))

    def _hull_ragged(self, groups, rhs_idx, elims, darkshadow, is_intersect, cap_rows, cap_out_rows, cap_hull_rows, copy):
        """xpg_lineq_{hull,project_union}_batch_ragged_rat32 (elims None: the hull). groups: a list of lists of systems."""
        ng = len(groups)
        goff = np.zeros(ng + 1, dtype=np.int32)
        goff[1:] = np.cumsum([len(g) for g in groups])
        members = [m for g in groups for m in g]
        nb = len(members)
        ok = np.zeros(ng, dtype=np.int32); member = np.zeros(ng, dtype=np.int32); chain = np.zeros(ng, dtype=np.int32)
        steps = np.zeros(ng, dtype=np.int32)
        if ng == 0:
            return ok, member, chain, steps, []
        flat, rows, cols, off, rhs = ragged_systems(members, rhs_idx)
        if not nb:                                          # groups without any member: no arrays at all
            flat, rows, cols, off = None, None, None, None
        if rhs is not None:                                 # one per group, or one per member
            if rhs.size == ng and rhs.size != nb:
                rhs = np.ascontiguousarray(np.repeat(rhs, np.diff(goff)))
            if rhs.size != nb:
                raise ValueError("one rhs_idx per group or per member: %d groups, %d members, %d rhs_idx" % (ng, nb, rhs.size))
        ooff = np.zeros(ng + 1, dtype=np.int64); orows = np.zeros(ng, dtype=np.int32)
        view = C.c_void_p()
        caps = (C.c_int(cap_rows or 0), C.c_int(cap_out_rows or 0), C.c_int(cap_hull_rows or 0))
        tail = (None, C.c_longlong(0), C.byref(view), vp(ooff), vp(orows), vp(ok), vp(member), vp(chain), vp(steps))
        if elims is None:
            name = "xpg_lineq_hull_batch_ragged_rat32"
            code = getattr(lib(), name)(self.ctx._h, C.c_int(ng), vp(goff), C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off), vp(rhs),
                                        C.c_int(int(is_intersect)), *caps, *tail)
        else:
            name = "xpg_lineq_project_union_batch_ragged_rat32"
            lists = [e for g in elims for e in g]
            if len(lists) != nb:
                raise ValueError("one list per member: %d members, %d lists" % (nb, len(lists)))
            el, eoff = _flat_lists(lists)
            code = getattr(lib(), name)(self.ctx._h, C.c_int(ng), vp(goff), C.c_int(nb), vp(flat), vp(rows), vp(cols), vp(off), vp(rhs),
                                        vp(el), vp(eoff), C.c_int(int(darkshadow)), C.c_int(int(is_intersect)), *caps, *tail)
        self.ctx.check(code, name)
        g0 = goff.tolist()
        width = [int(cols[g0[g]]) if g0[g + 1] > g0[g] else 0 for g in range(ng)]     # a group without members: a (0, 0, 2) result
        return ok, member, chain, steps, _cut(_rows_down(view, int(ooff[ng]), (2,), copy), ooff, width)

    def hull_ragged(self, groups, rhs_idx=None, is_intersect=False, cap_rows=None, cap_out_rows=None, cap_hull_rows=None, copy=True):
        """xpg_lineq_hull_batch_ragged_rat32: Lineq::ConvexHullUnionAndIntersect (linsys.cpp:283-336) for MANY lists of polyhedra
        in one call -- groups[g] is a list of systems that share cols and rhs_idx (one rhs_idx per group or per member; None:
        the last column). calcBound on every member in one launch, then ONE reduce per group over the members' bounds behind a
        zero row, in a second launch. Returns (ok[ng], member[ng], chain[ng], steps[ng], [rows of group g]): ok 1; 0 with member
        -1 where reduce found the group inconsistent (is_intersect: no rows); member m >= 0 with that member's calcBound verdict
        where a member failed (no rows: a stated deviation from the reference, which goes on with stale bounds); -need with
        member -1 where the group gathers need > cap_hull_rows rows. copy=False: views of the handle's pinned buffer."""
        return self._hull_ragged(groups, rhs_idx, None, False, is_intersect, cap_rows, cap_out_rows, cap_hull_rows, copy)

    def project_union_ragged(self, groups, rhs_idx, elims, is_intersect=False, darkshadow=False, cap_rows=None, cap_out_rows=None,
                             cap_hull_rows=None, copy=True):
        """xpg_lineq_project_union_batch_ragged_rat32: PolyTran::step_4's shape -- every member of groups[g] projected by its own
        list elims[g][i] in one launch, the results of a group concatenated in list order and ONE reduce per group. Returns what
        hull_ragged returns; a member's verdict is the chain's (chain is -1)."""
        return self._hull_ragged(groups, rhs_idx, elims, darkshadow, is_intersect, cap_rows, cap_out_rows, cap_hull_rows, copy)

    HULL_ROUTE_KEYS = ("producer_launches", "launches", "grid", "lds", "groups_lds", "groups_device", "seat_bytes", "slot_bytes",
                       "out_bytes", "gathered_rows")

    @staticmethod
    def hull_ragged_last_route():
        """xpg_lineq_hull_last_route of the calling thread's last hull_ragged / project_union_ragged call, as a dict."""
        return _view("xpg_lineq_hull_last_route", Lineq.HULL_ROUTE_KEYS)

    def rank(self, mats):
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        out = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_rat_rank_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), vp(out)),
                       "xpg_rat_rank_batch")
        return out

    def rankBasis(self, mats, is_unitarize):
        """Matrix<Rational>::rank(&basis, is_unitarize) (matt.h:2614-2726): (rank[nb], [basis b])."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        rk = np.zeros(nb, dtype=np.int32); brows = np.zeros(nb, dtype=np.int32)
        out = np.zeros((nb, rows, cols, 2), dtype=np.int32)
        self.ctx.check(lib().xpg_rat_rank_basis_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols),
                                                      C.c_int(int(is_unitarize)), vp(rk), vp(out), vp(brows)),
                       "xpg_rat_rank_basis_batch")
        return rk, [out[b, : brows[b]].copy() for b in range(nb)]

    def null(self, mats):
        """Matrix<Rational>::null (matt.h:2546-2584): [nb, cols, cols, 2], column convention."""
        a = _stack(mats)
        nb, rows, cols = a.shape[:3]
        out = np.zeros((nb, cols, cols, 2), dtype=np.int32)
        self.ctx.check(lib().xpg_rat_null_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), vp(out)),
                       "xpg_rat_null_batch")
        return out

    def hnf(self, imats):
        """INTMat::hnf (xmat.cpp:912-992) of int32 matrices [nb, rows, cols]: (status[nb], h, u)."""
        a = np.ascontiguousarray(imats, dtype=np.int32)
        if a.ndim == 2:
            a = a[None]
        nb, rows, cols = a.shape
        h = np.zeros((nb, rows, cols), dtype=np.int32); u = np.zeros((nb, cols, cols), dtype=np.int32)
        st = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_int_hnf_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols), vp(h), vp(u),
                                               vp(st)), "xpg_int_hnf_batch")
        return st, h, u

    def gcd(self, imats):
        """INTMat::gcd (xmat.cpp:996-1030): rows divided by the gcd of their nonzero magnitudes."""
        a = np.ascontiguousarray(imats, dtype=np.int32).copy()
        if a.ndim == 2:
            a = a[None]
        nb, rows, cols = a.shape
        self.ctx.check(lib().xpg_int_gcd_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(rows), C.c_int(cols)),
                       "xpg_int_gcd_batch")
        return a

    def det(self, mats):
        a = _stack(mats)
        nb, n = a.shape[0], a.shape[1]
        out = np.zeros((nb, 2), dtype=np.int32)
        self.ctx.check(lib().xpg_rat_det_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(n), vp(out)), "xpg_rat_det_batch")
        return out

    def inv(self, mats):
        a = _stack(mats)
        nb, n = a.shape[0], a.shape[1]
        out = np.zeros((nb, n, n, 2), dtype=np.int32); ok = np.zeros(nb, dtype=np.int32)
        self.ctx.check(lib().xpg_rat_inv_batch(self.ctx._h, C.c_int(nb), vp(a), C.c_int(n), vp(out), vp(ok)),
                       "xpg_rat_inv_batch")
        return ok, out


def reduce_dev(ctx, nb, mats_ptr, rows, cols, rhs_idx, is_intersect, out_rows_ptr, out_ok_ptr):
    """xpg_lineq_reduce_batch_rat32_dev: Lineq::reduce in place on device arrays, enqueue only (ctx.sync() after)."""
    ctx.check(lib().xpg_lineq_reduce_batch_rat32_dev(ctx._h, C.c_int(nb), C.c_void_p(mats_ptr), C.c_int(rows), C.c_int(cols),
                                                     C.c_int(rhs_idx), C.c_int(int(is_intersect)), C.c_void_p(out_rows_ptr),
                                                     C.c_void_p(out_ok_ptr)), "xpg_lineq_reduce_batch_rat32_dev")


def fme_dev(ctx, nb, mats_ptr, rows, cols, rhs_idx, u, darkshadow, outs_ptr, cap_rows, out_rows_ptr, out_ok_ptr):
    """xpg_lineq_fme_batch_rat32_dev: Lineq::fme on device arrays, enqueue only."""
    ctx.check(lib().xpg_lineq_fme_batch_rat32_dev(ctx._h, C.c_int(nb), C.c_void_p(mats_ptr), C.c_int(rows), C.c_int(cols),
                                                  C.c_int(rhs_idx), C.c_int(u), C.c_int(int(darkshadow)), C.c_void_p(outs_ptr),
                                                  C.c_int(cap_rows), C.c_void_p(out_rows_ptr), C.c_void_p(out_ok_ptr)),
              "xpg_lineq_fme_batch_rat32_dev")


def project_dev(ctx, nb, mats_ptr, rows, cols, rhs_idx, elim, darkshadow, cap_rows, cap_out_rows, outs_ptr, out_rows_ptr,
                out_ok_ptr, out_steps_ptr):
    """xpg_lineq_project_batch_rat32_dev: a list of eliminations on device arrays in one launch, enqueue only. `elim` is a
    host list; outs is [nb][cap_out_rows][cols] (cap_out_rows <= 0: cap_rows)."""
    el = np.ascontiguousarray(elim, dtype=np.int32).reshape(-1)
    ctx.check(lib().xpg_lineq_project_batch_rat32_dev(ctx._h, C.c_int(nb), C.c_void_p(mats_ptr), C.c_int(rows), C.c_int(cols),
                                                      C.c_int(rhs_idx), vp(el), C.c_int(el.size), C.c_int(int(darkshadow)),
                                                      C.c_int(cap_rows), C.c_int(cap_out_rows), C.c_void_p(outs_ptr),
                                                      C.c_void_p(out_rows_ptr), C.c_void_p(out_ok_ptr), C.c_void_p(out_steps_ptr)),
              "xpg_lineq_project_batch_rat32_dev")


def levels_dev(ctx, nb, mats_ptr, rows, cols, rhs_idx, elim, darkshadow, cap_rows, cap_out_rows, outs_ptr, out_rows_ptr,
               out_ok_ptr, out_steps_ptr):
    """xpg_lineq_levels_batch_rat32_dev: every level of a projection on device arrays in one launch, enqueue only. `elim` is a
    host list; outs is [nb][len(elim)][cap_out_rows][cols], out_rows [nb][len(elim)], the other two [nb]. Both capacities are
    the caller's: none is defaulted."""
    el = np.ascontiguousarray(elim, dtype=np.int32).reshape(-1)
    ctx.check(lib().xpg_lineq_levels_batch_rat32_dev(ctx._h, C.c_int(nb), C.c_void_p(mats_ptr), C.c_int(rows), C.c_int(cols),
                                                     C.c_int(rhs_idx), vp(el), C.c_int(el.size), C.c_int(int(darkshadow)),
                                                     C.c_int(cap_rows), C.c_int(cap_out_rows), C.c_void_p(outs_ptr),
                                                     C.c_void_p(out_rows_ptr), C.c_void_p(out_ok_ptr), C.c_void_p(out_steps_ptr)),
              "xpg_lineq_levels_batch_rat32_dev")


def transform_levels_dev(ctx, nb, nests_ptr, shared_nest, tmats_ptr, rows, cols, rhs_idx, mode, cap_rows, cap_out_rows, outs_ptr,
                         out_rows_ptr, out_ok_ptr, out_steps_ptr, out_kind_ptr, out_det_ptr, out_mult_ptr):
    """xpg_lineq_transform_levels_batch_rat32_dev: the limits of transformed loop nests on device arrays in one launch, enqueue
    only. outs is [nb][rhs_idx][cap_out_rows][cols] (level 0 the transformed nest), out_rows [nb][rhs_idx], ok / steps / kind
    [nb], det [nb] (mode 0), mult [nb][rhs_idx][rhs_idx]. Both capacities are the caller's: none is defaulted."""
    ctx.check(lib().xpg_lineq_transform_levels_batch_rat32_dev(
        ctx._h, C.c_int(nb), C.c_void_p(nests_ptr), C.c_int(int(shared_nest)), C.c_void_p(tmats_ptr), C.c_int(rows), C.c_int(cols),
        C.c_int(rhs_idx), C.c_int(mode), C.c_int(cap_rows), C.c_int(cap_out_rows), C.c_void_p(outs_ptr), C.c_void_p(out_rows_ptr),
        C.c_void_p(out_ok_ptr), C.c_void_p(out_steps_ptr), C.c_void_p(out_kind_ptr), C.c_void_p(out_det_ptr), C.c_void_p(out_mult_ptr)),
        "xpg_lineq_transform_levels_batch_rat32_dev")


def bounds_dev(ctx, nb, mats_ptr, rows, cols, rhs_idx, cap_rows, cap_out_rows, outs_ptr, out_rows_ptr, out_ok_ptr, out_chain_ptr,
               out_steps_ptr):
    """xpg_lineq_bounds_batch_rat32_dev: Lineq::calcBound on device arrays in one launch, enqueue only. outs is
    [nb][rhs_idx][cap_out_rows][cols] (cap_out_rows <= 0: cap_rows), out_rows [nb][rhs_idx], the other three [nb]."""
    ctx.check(lib().xpg_lineq_bounds_batch_rat32_dev(ctx._h, C.c_int(nb), C.c_void_p(mats_ptr), C.c_int(rows), C.c_int(cols),
                                                     C.c_int(rhs_idx), C.c_int(cap_rows), C.c_int(cap_out_rows), C.c_void_p(outs_ptr),
                                                     C.c_void_p(out_rows_ptr), C.c_void_p(out_ok_ptr), C.c_void_p(out_chain_ptr),
                                                     C.c_void_p(out_steps_ptr)),
              "xpg_lineq_bounds_batch_rat32_dev")


def rank_dev(ctx, nb, mats_ptr, rows, cols, out_rank_ptr):
    """xpg_rat_rank_batch_dev: Matrix<Rational>::rank on device arrays, enqueue only."""
    ctx.check(lib().xpg_rat_rank_batch_dev(ctx._h, C.c_int(nb), C.c_void_p(mats_ptr), C.c_int(rows), C.c_int(cols),
                                           C.c_void_p(out_rank_ptr)), "xpg_rat_rank_batch_dev")
