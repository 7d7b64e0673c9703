"""What tests/test_lineq_ragged_host.py and tests/test_gpu_lineq_ragged.py share: a restatement of the plan of a ragged
projection / levels call (lineq_host.hip.h ragged_chain_plan: every list under project_check's rules, then the ENVELOPE -- the
widest system's columns, the capacities of the system with the most rows -- under the uniform plans' rules as
tests/lineq_project_cases.py restates them, the output slots following each system's own columns), the mixed batches of the
GPU tests, and the stepped checkers of the uniform tests applied per system with its own list."""
import numpy as np

import lineq_project_cases as pc
from lineq_levels_cases import stepped_levels                                        # noqa: F401 (re-exported)
from lineq_project_cases import XPG_ERR_SHAPE, XPG_ERR_UNSUPPORTED, CHAIN_MAX, rows_equal, stepped   # noqa: F401 (re-exported)

PLAN_KEYS = ("launches", "grid", "groups", "sys_lds", "cap_lds", "seat_bytes", "out_bytes", "cap", "cap_out", "cols", "rows")
ROUTE_KEYS = PLAN_KEYS[:7]
# (rows, nv, list): the four shape classes of the base batch, and the class whose steps have both homes
SHAPES = [(4, 2, [1]), (5, 3, [2, 1]), (6, 4, [3, 2]), (9, 4, [3, 2, 1])]
HOMES = (12, 6, [5, 4], 8)


def check(cols, rhs, elim):
    """project_check: 0 or the error code of one system's list."""
    if cols <= 1 or rhs < 1 or rhs >= cols or elim is None or len(elim) <= 0:
        return XPG_ERR_SHAPE
    if any(u < 0 or u >= rhs for u in elim):
        return XPG_ERR_SHAPE
    return XPG_ERR_UNSUPPORTED if len(elim) > CHAIN_MAX else 0


def plan(rows, cols, rhs, elims, levels, cap_rows=0, cap_out_rows=0):
    """The eleven figures of xpg_test_lineq_ragged_plan, or the error code. rhs None: the last column of each system."""
    nb = len(rows)
    if nb <= 0:
        return XPG_ERR_SHAPE
    too_long = False
    for b in range(nb):
        if rows[b] <= 0:
            return XPG_ERR_SHAPE
        rc = check(cols[b], cols[b] - 1 if rhs is None else rhs[b], elims[b])
        if rc == XPG_ERR_SHAPE:
            return rc
        too_long |= rc != 0
    if too_long:
        return XPG_ERR_UNSUPPORTED
    ecols, erows = max(cols), max(rows)
    if erows > 32767:
        return XPG_ERR_UNSUPPORTED
    cap = erows * erows // 4 + erows + 1 if cap_rows <= 0 else cap_rows
    cap = max(cap, erows)
    if cap_out_rows <= 0:
        cap_out = min(cap, 4 * erows + 16) if levels else cap
    else:
        cap_out = min(cap_out_rows, cap)
    if cap > 32767:
        return XPG_ERR_UNSUPPORTED
    cap_lds, lds = pc.fme_lds(cap, cap, ecols)
    if lds > 160 * 1024:
        return XPG_ERR_UNSUPPORTED
    sys_lds = (lds + 15) & ~15
    grid = min(nb, 4096)                                     # fme takes the whole wave: one system per workgroup
    cells = sum((len(elims[b]) if levels else 1) * cols[b] for b in range(nb))
    return dict(zip(PLAN_KEYS, (1, grid, 1, sys_lds, cap_lds, grid * 2 * cap * ecols * 8, cells * cap_out * 8, cap, cap_out, ecols, erows)))


def _args(rows, cols, rhs, elims):
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    eoff = np.zeros(len(rows) + 1, dtype=np.int32)
    eoff[1:] = np.cumsum([len(e) for e in elims])
    flat = [u for e in elims for u in e]
    return i32(rows), i32(cols), None if rhs is None else i32(rhs), i32(flat) if flat else None, eoff


def plan_view(rows, cols, rhs, elims, levels, cap_rows=0, cap_out_rows=0, nb=None, eoff=None):
    """xpg_test_lineq_ragged_plan (host only): the same dict, or the error code."""
    import ctypes as C
    from xpoly_amd._capi import lib
    r, c, h, el, eo = _args(rows, cols, rhs, elims)
    if eoff is not None:
        eo = np.ascontiguousarray(eoff, dtype=np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    out = np.zeros(11, dtype=np.int64)
    rc = lib().xpg_test_lineq_ragged_plan(C.c_int(len(rows) if nb is None else nb), vp(r), vp(c), vp(h), vp(el), vp(eo), C.c_int(int(levels)),
                                          C.c_int(cap_rows), C.c_int(cap_out_rows), vp(out), C.c_int(11))
    return rc if rc != 0 else dict(zip(PLAN_KEYS, (int(x) for x in out)))


def class_batch(rows, nv, nb, seed=None):
    """tests/test_gpu_lineq_project.py's generator: nb systems of one shape."""
    from tools import gen
    rng = np.random.default_rng(rows * 100 + nv if seed is None else seed)
    return np.stack([gen.random_system(rng, rows, nv) for _ in range(nb)])


def base_batch(per=12):
    """The four classes interleaved, 4 * per systems: (mats, nv, elims), system 4 * i + c the i-th of class c."""
    classes = [class_batch(r, nv, per) for r, nv, _ in SHAPES]
    mats, nvs, elims = [], [], []
    for i in range(per):
        for c, (_, nv, el) in enumerate(SHAPES):
            mats.append(classes[c][i]); nvs.append(nv); elims.append(list(el))
    return mats, nvs, elims


def want_project(port, mats, nvs, elims, dark=False, cap_rows=None, cap_out_rows=None):
    return [stepped(port, mats[b], nvs[b], elims[b], dark, cap_rows=cap_rows, cap_out_rows=cap_out_rows) for b in range(len(mats))]


def want_levels(port, mats, nvs, elims, dark=False, cap_rows=None, cap_out_rows=None):
    return [stepped_levels(port, mats[b], nvs[b], elims[b], dark, cap_rows=cap_rows, cap_out_rows=cap_out_rows) for b in range(len(mats))]


NEST_CLASSES = ((3, (4, 6, 13), 4), (4, (5, 8, 10), 4), (6, (5, 8, 12), 6))


def adapter_nests(port, seed=77):
    """Nests of depth 3, 4 and 6 with three row classes each, generated as tests/test_gpu_lineq_levels.py's adapter test
    generates them: at depth 4 and 6 a system that does not fit its own default capacities is drawn again, at depth 3 it is
    kept -- and depth 3 holds the class with the most rows, so that class alone can exceed the ENVELOPE's defaults. Returns
    [(nv, integer matrix)], grouped by depth."""
    from tools import gen
    rng = np.random.default_rng(seed)
    out = []
    for nv, row_classes, per in NEST_CLASSES:
        elim = list(range(nv - 1, 0, -1))
        for _ in range(per):
            for rows in row_classes:
                cap = rows * rows // 4 + rows + 1
                while True:
                    m = rng.integers(-3, 4, size=(rows, nv + 1)) * (rng.random((rows, nv + 1)) < 0.7)
                    m[:, nv] = rng.integers(-2, 9, size=rows)
                    if nv == 3 or stepped_levels(port, gen.to_rat(m), nv, elim, cap_rows=cap, cap_out_rows=min(cap, 4 * rows + 16))[0] >= 0:
                        break
                out.append((nv, m.astype(np.int32)))
    return out


def adapter_calls(port, nests):
    """The calls xpoly_amd::levels_nests makes for these nests, replayed on the CPU with the checker: (calls, the (nv, rows)
    classes that were short at some call). The capacities start at the envelope's defaults and are raised as the adapter
    raises them."""
    from tools import gen
    most = max(m.shape[0] for _, m in nests)
    cap = most * most // 4 + most + 1
    cap_out = min(cap, 4 * most + 16)
    short = set()
    for call in range(1, 9):
        need_cap = need_out = 0
        for nv, m in nests:
            ok = stepped_levels(port, gen.to_rat(m), nv, list(range(nv - 1, 0, -1)), cap_rows=cap, cap_out_rows=cap_out)[0]
            if ok < 0:
                short.add((nv, m.shape[0]))
                if -ok > cap:
                    need_cap = max(need_cap, -ok)
                else:
                    need_out = max(need_out, -ok)
        if not need_cap and not need_out:
            return call, short
        cap = need_cap or cap
        cap_out = need_out or cap_out
    return 9, short
