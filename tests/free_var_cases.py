"""Inputs of the free-variable tests (tests/test_free_vars_host.py, tests/test_gpu_mip_free_vars.py): integer programs and
dependence polyhedra whose variable constraints are a SIGN PATTERN -- diagonal -1 (x_j >= 0) or 0 (x_j free), the vc
Lineq::initVarConstraint builds (src/com/linsys.cpp:803-819) -- and the checker's answers for them.

The real reference is undefined with a free variable (SIX::normalize fills its vcmap through the stack-walking sete(),
src/com/lpsol.h:1376-1378), so the checker is the CPU restatement in NON-STRICT mode, which follows the intent
v = v' - v'': every oracle call here runs between orc_set_strict(0) and orc_set_strict(1)."""
import contextlib
import hashlib

import numpy as np

from tools import gen

F64, RAT = 0, 1
SHAPES = ((3, 4, 1), (4, 5, 2), (3, 6, 3), (2, 3, 3))           # (coupling rows, variables, free variables)
PER_SHAPE = 256


@contextlib.contextmanager
def non_strict(port):
    port.lib.orc_set_strict(0)
    try:
        yield
    finally:
        port.lib.orc_set_strict(1)


def as_f64(a):
    return None if a is None else np.ascontiguousarray(a[..., 0].astype(np.float64))


def free_var_mip(rng, m, nv, nfree):
    """One integer program: the free set first, then x_j <= hi per variable, -x_j <= -lo per FREE variable (so the LP
    is bounded below there and optima go negative), m coupling rows, the objective. Integer arrays."""
    free = tuple(sorted(int(j) for j in rng.choice(nv, nfree, replace=False)))
    hi = rng.integers(1, 7, size=nv)
    lo = rng.integers(-6, 0, size=nfree)
    A = rng.integers(-3, 4, size=(m, nv))
    b = rng.integers(-2, 9, size=m)
    c = rng.integers(-4, 9, size=nv)
    leq = np.zeros((nv + nfree + m, nv + 1), dtype=np.int32)
    for j in range(nv):
        leq[j, j] = 1; leq[j, nv] = hi[j]
    for k, j in enumerate(free):
        leq[nv + k, j] = -1; leq[nv + k, nv] = -lo[k]
    leq[nv + nfree:, :nv] = A; leq[nv + nfree:, nv] = b
    tgtf = np.concatenate([c, [0]]).astype(np.int32)
    return dict(free=free, leq=leq, tgtf=tgtf)


def shape_problems(shape, count=PER_SHAPE):
    m, nv, nfree = shape
    rng = np.random.default_rng(1000 + 10 * nv + nfree)
    return [free_var_mip(rng, m, nv, nfree) for _ in range(count)]


def groups_by_free_set(probs):
    """vc is shared by a batch: the problems' indices grouped by their free set, in order of first appearance."""
    out = {}
    for i, p in enumerate(probs):
        out.setdefault(p["free"], []).append(i)
    return list(out.items())


def batch_arrays(probs, idx, kind):
    """(tgtf [nb, cols(,2)], vc, leq [nb, rows, cols(,2)]) of the problems idx, which share a free set."""
    nv = probs[idx[0]]["leq"].shape[1] - 1
    tg = gen.to_rat(np.stack([probs[i]["tgtf"] for i in idx]))
    leq = gen.to_rat(np.stack([probs[i]["leq"] for i in idx]))
    vc = gen.to_rat(gen.vc_nonneg(nv, False, probs[idx[0]]["free"]))
    if kind == F64:
        return as_f64(tg), as_f64(vc), as_f64(leq)
    return tg, vc, leq


_oracle_cache = {}


def oracle_answers(port, shape, kind, is_max, count=PER_SHAPE):
    """[(status, v, sol)] of the first `count` problems of the shape from the non-strict CPU restatement."""
    key = (shape, kind, is_max)
    have = _oracle_cache.setdefault(key, [])
    if len(have) < count:
        probs = shape_problems(shape, count)
        with non_strict(port):
            for i in range(len(have), count):
                tg, vc, leq = batch_arrays(probs, [i], kind)
                have.append(port.mip_solve(kind, is_max, False, tg[0], vc, None, leq[0]))
    return have[:count]


def same_answer(got_st, got_v, got_sol, want):
    """Exact: status, the optimum's bits, and on success the solution's bits."""
    if int(got_st) != int(want[0]):
        return False
    if np.asarray(got_v).tobytes() != np.asarray(want[1]).tobytes():
        return False
    return int(want[0]) != 0 or np.asarray(got_sol).tobytes() == np.asarray(want[2]).tobytes()


def batch_digests(ctx):
    """One line per (shape, kind, direction, free set): sha256 over status + v + sol, the node count and the route.
    Run in-process (the device tree walk) and in a child started with XPG_MIP_DEVICE=0 (the host controller)."""
    from xpoly_amd.six import mip_batch_vc, mip_last_route
    lines = []
    for shape in SHAPES:
        probs = shape_problems(shape)
        for kind in (RAT, F64):
            for is_max in (True, False):
                for free, idx in groups_by_free_set(probs):
                    tg, vc, leq = batch_arrays(probs, idx, kind)
                    st, v, sol, nodes = mip_batch_vc(ctx, is_max, False, tg, vc, leq, kind=kind)
                    r = mip_last_route()
                    h = hashlib.sha256(st.tobytes() + v.tobytes() + sol.tobytes()).hexdigest()
                    lines.append(("%s %d %d %s %s %d" % (shape, kind, is_max, free, h, nodes), r, len(idx)))
    return lines


def general_vcs(nv):
    """Two vc that are NOT sign patterns: a diagonal of -2, a nonzero constant."""
    a = gen.vc_nonneg(nv, False); a[0, 0] = -2
    b = gen.vc_nonneg(nv, False); b[1, nv] = -1
    return a, b


def wide_lp_f64(count=16, nv=20, nfree=16, rows=50, seed=7777):
    """fp64 programs whose node LPs fit the tree walk's LDS budget without the twins of their free variables and not with
    them: nv variables, the first nfree free, `rows` inequalities -- x_j <= [1,3] per variable, -x_j <= [1,3] per free
    one, the rest sparse couplings with a constant in [3,11]. Returns (tgtf [count, cols], vc, leq [count, rows, cols])."""
    rng = np.random.default_rng(seed)
    ncoup = rows - nv - nfree
    leq = np.zeros((count, rows, nv + 1))
    tg = np.zeros((count, nv + 1))
    for b in range(count):
        for j in range(nv):
            leq[b, j, j] = 1; leq[b, j, nv] = rng.integers(1, 4)
        for j in range(nfree):
            leq[b, nv + j, j] = -1; leq[b, nv + j, nv] = rng.integers(1, 4)
        A = rng.integers(-2, 3, size=(ncoup, nv)) * (rng.random((ncoup, nv)) < 0.25)
        leq[b, nv + nfree:, :nv] = A
        leq[b, nv + nfree:, nv] = rng.integers(3, 12, size=ncoup)
        tg[b, :nv] = rng.integers(-3, 6, size=nv)
    vc = gen.vc_nonneg(nv, True, tuple(range(nfree)))
    return tg, vc, leq


def free_var_eq_problems(kind, count=240):
    """tests/mip_eq_cases.py's random MIPs with equalities at the root (shapes and is_bin drawn as mip_eq_cases.run draws
    them), each with one or two of its variables made free."""
    import mip_eq_cases
    rng = np.random.default_rng(5150 + kind)
    out = []
    for _ in range(count):
        m_leq, m_eq, nv = int(rng.integers(0, 6)), int(rng.integers(1, 4)), int(rng.integers(2, 7))
        is_bin = bool(rng.integers(0, 2))
        p = mip_eq_cases.random_mip_eq(rng, m_leq, m_eq, nv, is_bin)
        nfree = int(rng.integers(1, 3))
        free = tuple(int(j) for j in rng.choice(nv, min(nfree, nv), replace=False))
        p["vc"] = gen.to_rat(gen.vc_nonneg(nv, False, free))
        if kind == F64:
            p = {k: (as_f64(v) if k != "ind" else v) for k, v in p.items()}
        out.append((p, is_bin))
    return out


DEP_SHAPES = ((3, 2, 9), (4, 1, 12), (3, 3, 10))                 # (variables, constant symbols, rows)


def dep_systems(count=4096):
    """Integer dependence polyhedra with constant symbols, `count` per shape of DEP_SHAPES, from one generator."""
    rng = np.random.default_rng(4242)
    out = []
    for nv, ns, rows in DEP_SHAPES:
        mats = np.stack([gen.random_system(rng, rows, nv + ns) for _ in range(count)])
        mats[..., 1] = 1
        out.append(((nv, ns, rows), mats))
    return out


def dep_wide_vc(nv, ns, vc=None):
    """The caller's vc [nv][nv + 1] (None: x >= 0) widened by all-zero rows / columns for the symbols."""
    wide = np.zeros((nv + ns, nv + ns + 1), dtype=np.int32)
    if vc is None:
        wide[np.arange(nv), np.arange(nv)] = -1
    else:
        wide[:nv, :nv] = vc[:, :nv, 0]; wide[:nv, nv + ns] = vc[:, nv, 0]
    return gen.to_rat(wide)


def dep_oracle(port, mat, nv, ns, wide):
    """(what Lineq::reduce alone decides or None, the symbols-as-variables verdict) of one polyhedron: move2var, reduce at
    the last column, has_solution(int, unique) on the widened vc. Call inside non_strict()."""
    moved = port.move2var(mat, nv, nv + 1, nv + ns) if ns else mat
    ok, res = port.reduce(moved, nv + ns, True)
    if not ok:
        return 1, 1
    if res.shape[0] == 0:
        return 0, 0
    h = port.has_solution(res, None, wide, nv + ns, True, True)
    return None, (-7 if h == -7 else (0 if h == 1 else 1))
