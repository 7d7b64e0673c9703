"""What tests/test_lineq_rescue_host.py, tests/test_gpu_lineq_rescue.py and tools/gen_golden_lineq_rescue.py share: loop nests
whose coefficients are tile sizes, strides and array extents -- large enough that the Rational leaves int32 inside the
elimination chain and takes the float32 `appro` rescue (scalar.hip.h on the device, counted by appro_count() of
oracle/checker.py on the host) -- and the expected answers of every fused row-elimination entry point on them. The answers come
from the checkers' existing compositions only (lineq_project_cases.stepped, lineq_levels_cases.stepped_levels,
lineq_bounds_cases.chains, which the host test holds against checker.calc_bound, lineq_transform_cases.transformed,
lineq_hull_cases.hull / project_union), each with the appro_count() delta of its system next to it. Everything is drawn from
fixed seeds and importable without a GPU."""
import numpy as np

import lineq_bounds_cases as bc
import lineq_hull_cases as hc
import lineq_levels_cases as lc
import lineq_project_cases as pc
import lineq_transform_cases as tc
from lineq_project_cases import rows_equal   # noqa: F401 (re-exported)

K, W, LATE = (1000, 5000), (30000, 70000), (30, 130)     # the coefficient ranges: tile sizes, extents, and the late starter
PER = 16                                                 # systems per family
GOLDEN_PER = 2                                           # of which the fixture of real reference outputs holds the first
SKEW = 75000                                             # 30 000 * SKEW is past 2^31 already


# ---- the nests --------------------------------------------------------------------------------------------------------------------
def tiled_nest(rng, n, lo, hi, consts=1, inner=1):
    """A triangular nest of depth n as A * i <= C, [2 * (n - 1 + inner), n + consts, 2]: per level k a lower bound
    -s i_k + a i_(k-1) <= c and an upper bound s i_k - a i_(k-1) - a' i_(k-2) <= c, the innermost level `inner` of each (a
    min / max of several tile edges), every s, a, a', c drawn from lo .. hi. consts == 2 adds a symbolic extent N behind the
    constant (lineq_transform_cases.nest has one): the upper bounds of every level but 1 carry a coefficient of N, so
    rhs_idx < cols - 1."""
    draw = lambda: int(rng.integers(lo, hi + 1))
    rows = []
    for k in range(n):
        for _ in range(inner if k == n - 1 else 1):
            low = [0] * (n + consts); low[k] = -draw(); low[n] = draw()
            up = [0] * (n + consts); up[k] = draw(); up[n] = draw()
            if k:
                low[k - 1] = draw(); up[k - 1] = -draw()
            if k > 1:
                up[k - 2] = -draw()
            if consts == 2 and k != 1:
                up[n + 1] = draw()
            rows += [low, up]
    return tc.to_rat(rows)


def tiled_empty_nest(rng, n, lo, hi, at=1):
    """The tiled nest of depth n >= 2 with level `at` replaced by s i_at - a i_(at-1) <= -c against -s i_at + a i_(at-1) <= -c'
    (one s, one a): no point, and fme finds it when variable `at` goes -- with at == 1 at the chain's last step, after the
    steps that rescue."""
    a = tiled_nest(rng, n, lo, hi)[..., 0].tolist()
    s, f = int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))
    low = [0] * (n + 1); low[at] = -s; low[at - 1] = f; low[n] = -int(rng.integers(lo, hi + 1))
    up = [0] * (n + 1); up[at] = s; up[at - 1] = -f; up[n] = -int(rng.integers(lo, hi + 1))
    return tc.to_rat(a[:2 * at] + [low, up] + a[2 * at + 2:])


def predivided(mat):
    """Every row divided by the magnitude of its first nonzero coefficient and LEFT UNREDUCED: cell x/1 becomes x/|s|, the
    leading cell s/|s|. The cells enter the chain with denominators other than 1 and not in canonical form."""
    out = np.array(mat, dtype=np.int32, copy=True)
    for i in range(out.shape[0]):
        lead = [int(v) for v in out[i, :, 0] if v != 0]
        if lead:
            out[i, :, 1] = abs(lead[0])
    return out


# name: (depth, range, consts, kind). rhs_idx is the depth; the list of a chain is depth-1 .. 1
FAMILIES = {
    "d3_k": (3, K, 1, "nest"), "d4_k": (4, K, 2, "nest"), "d5_k": (5, K, 2, "nest"),
    "d3_w": (3, W, 1, "nest"), "d4_w": (4, W, 1, "nest"), "d5_w": (5, W, 1, "nest"),
    "d5_late": (5, LATE, 1, "nest"),
    "d4_empty": (4, W, 1, "empty"),
    "d4_prediv": (4, W, 1, "prediv"),
    # three lower and three upper bounds at the innermost level, 14 x 7: the first step needs 17 rows, more than the LDS result
    # area holds once the layout is past 12 KB, so its result is built in the seat's device slots
    "d5_wide": (5, K, 2, "wide"),
}
WIDE_NB, WIDE_CAP = 8, 768                               # d5_wide: its first systems, and a cap_rows that holds all their steps
TILED = [f for f, v in FAMILIES.items() if v[3] in ("nest", "wide")]
SMALL = [f for f in FAMILIES if f != "d5_wide"]          # the families that run at the default capacities too


def family(name, nb=PER):
    """[nb, rows, cols, 2] int32 of one family, system b the same whatever nb is."""
    n, (lo, hi), consts, kind = FAMILIES[name]
    out = []
    for b in range(nb):
        rng = np.random.default_rng([17, n, lo, consts, len(kind), b])
        if kind == "empty":
            out.append(tiled_empty_nest(rng, n, lo, hi, 1))
        elif kind == "prediv":
            out.append(predivided(tiled_nest(rng, n, lo, hi, consts)))
        else:
            out.append(tiled_nest(rng, n, lo, hi, consts, 3 if kind == "wide" else 1))
    return np.stack(out)


def depth(name):
    return FAMILIES[name][0]


def elim_of(n):
    return list(range(n - 1, 0, -1))


# ---- expected answers, each with the appro_count() delta of its system -----------------------------------------------------------
def counted(chk, fn, *args, **kw):
    """(fn(*args), the rescues the checker counted while it ran)."""
    a0 = chk.appro_count()
    out = fn(*args, **kw)
    return out, chk.appro_count() - a0


def want_project(chk, mats, n, cap_rows=None, cap_out_rows=None):
    """([lineq_project_cases.stepped per system], [rescues per system])."""
    got = [counted(chk, pc.stepped, chk, m, n, elim_of(n), False, cap_rows, cap_out_rows) for m in mats]
    return [g for g, _ in got], [r for _, r in got]


def want_levels(chk, mats, n, cap_rows=None, cap_out_rows=None):
    got = [counted(chk, lc.stepped_levels, chk, m, n, elim_of(n), False, cap_rows, cap_out_rows) for m in mats]
    return [g for g, _ in got], [r for _, r in got]


def want_bounds(chk, mats, n, cap_rows=None, cap_out_rows=None):
    got = [counted(chk, bc.chains, chk, m, n, cap_rows, cap_out_rows) for m in mats]
    return [g for g, _ in got], [r for _, r in got]


def rescues_by_step(chk, mat, n):
    """[rescues of step k] of the chain n-1 .. 1, as far as it runs: the checker's fme replayed on the levels stepped_levels
    returned (a chain that ends 0 or short has no levels: it is walked here until it stops)."""
    cur, out = np.asarray(mat), []
    for u in elim_of(n):
        if cur.shape[0] == 0:
            break
        (ok, res), r = counted(chk, chk.fme, cur, n, u, False)
        out.append(r)
        if not ok:
            break
        cur = res
    return out


def first_rescue_step(chk, mat, n):
    """The first step of the chain that rescues, or None."""
    return next((k for k, r in enumerate(rescues_by_step(chk, mat, n)) if r), None)


# ---- the transformations ----------------------------------------------------------------------------------------------------------
def skews(n, s=SKEW):
    """{name: T [n, n, 2]}: unimodular, the off-diagonal entry s -- [[1, s], [0, 1]] and its transpose, at depth 3 and 4
    extended by an interchange of the last two loops and a reversal of the last. T^-1 carries -s: against a nest of 30 000 ..
    70 000 the product loop tmp + a(i,k) * m(k,j) leaves int32."""
    e = np.eye(n, dtype=np.int64)
    up = e.copy(); up[0, 1] = s
    low = e.copy(); low[1, 0] = s
    out = {"skew_upper": up, "skew_lower": low}
    if n >= 3:
        ic = e.copy(); ic[[n - 2, n - 1]] = ic[[n - 1, n - 2]]
        rev = e.copy(); rev[n - 1, n - 1] = -1
        far = e.copy(); far[0, n - 1] = -s
        out.update(skew_interchange=ic @ up, skew_reversal=up @ rev, skew_both=rev @ ic @ low)
        if n == 3:
            out.update(skew_far=far @ ic)
    return {k: tc.to_rat(v) for k, v in out.items()}


def det_rescued(n):
    """A T [n, n, 2] whose determinant the Rational cannot compute exactly: 2 x 2 minors near 2.5e9. Whatever kind the
    checker then reports is the expected kind."""
    base = np.array([[50021, 40003, 7, 11], [40007, 50023, 13, 5], [3, 9, 46021, 17], [2, 6, 19, 44987]], dtype=np.int64)
    return tc.to_rat(base[:n, :n])


def tmats(n):
    """The transformations of depth n >= 2: the large skews, the identity (the nest's own levels), and the T whose determinant
    approximates."""
    out = dict(skews(n))
    out["identity"] = tc.to_rat(np.eye(n, dtype=np.int64))
    out["det_rescued"] = det_rescued(n)
    return out


TRANSFORM_NESTS = {2: "t2_w", 3: "d3_w", 4: "d4_w"}          # the nests the transformations meet: 30 000 .. 70 000


def transform_nests(n, nb):
    """[nb, 2n, n + 1, 2]: the (30 000, 70 000) nests of depth n."""
    if n == 2:
        return np.stack([tiled_nest(np.random.default_rng([17, 2, W[0], 1, 4, b]), 2, *W) for b in range(nb)])
    return family(TRANSFORM_NESTS[n], nb)


def want_transformed(chk, pairs, mode=0, cap_rows=None, cap_out_rows=None):
    """([lineq_transform_cases.transformed per (nest, T)], [rescues per pair])."""
    got = [counted(chk, tc.transformed, chk, a, t, mode, cap_rows, cap_out_rows) for a, t in pairs]
    return [g for g, _ in got], [r for _, r in got]


# ---- the mixed list of the ragged entries, and the groups of the hulls ------------------------------------------------------------
MIXED_FAMILIES = ("d3_k", "d4_k", "d5_k", "d3_w", "d4_w", "d5_w")
MIXED_PER = 3
MIXED_EXACT = ((6, 3), (9, 4), (5, 2))                       # (rows, nv) of the gen.random_system members


def mixed_list():
    """(mats, nvs, elims, names): depths 3, 4 and 5 and both coefficient ranges interleaved, 18 nests, and three
    gen.random_system systems among them (entries within [-3, 3]: exact) -- exact and rescued systems share one envelope."""
    from tools import gen
    fams = {f: family(f, MIXED_PER) for f in MIXED_FAMILIES}
    mats, nvs, names = [], [], []
    for i in range(MIXED_PER):
        for f in MIXED_FAMILIES:
            mats.append(fams[f][i]); nvs.append(depth(f)); names.append(f)
        rows, nv = MIXED_EXACT[i]
        mats.append(gen.random_system(np.random.default_rng(1700 + i), rows, nv)); nvs.append(nv); names.append("exact")
    return mats, nvs, [elim_of(nv) for nv in nvs], names


def groups():
    """(groups, rhss, names) for hull_ragged / project_union_ragged: groups of 1, 2 and 5 members of one depth taken from the
    mixed list (the 5 from more systems of its two depth-4 families), and a group of 3 whose middle member is an empty nest."""
    d4 = list(family("d4_w", 3)) + list(family("d4_prediv", 2))
    d5 = family("d5_k", 2)
    d3 = family("d3_w", 1)
    holed = [family("d4_w", 4)[3], family("d4_empty", 1)[0], family("d4_prediv", 3)[2]]
    return [[d3[0]], [d5[0], d5[1]], d4, holed], [3, 5, 4, 4], ["one", "two", "five", "with empty"]


def want_hulls(chk, is_intersect, **caps):
    g, rhss, _ = groups()
    got = [counted(chk, hc.hull, chk, m, r, is_intersect, **caps) for m, r in zip(g, rhss)]
    return [x for x, _ in got], [r for _, r in got]


def want_unions(chk, is_intersect, **caps):
    g, rhss, _ = groups()
    got = [counted(chk, hc.project_union, chk, m, r, [elim_of(r)] * len(m), is_intersect, False, **caps) for m, r in zip(g, rhss)]
    return [x for x, _ in got], [r for _, r in got]
