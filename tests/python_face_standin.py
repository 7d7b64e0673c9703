"""A scripted stand-in for libxpoly_amd.so, for tests/test_python_face_host.py: what xpoly_amd/six.py and xpoly_amd/lineq.py pass
DOWN to the C ABI and hand UP to their callers, seen without the library and without a device.

The library takes no argtypes, so each wrapper of the face chooses the ctypes kind of every scalar and the array behind every
pointer. TABLE states, per entry point under test and in the order of include/xpoly_amd.h, what the header expects: a scalar, or
a pointer with its element type and its length as an expression over the call's scalars and arrays. With it the stand-in reads
every input (and refuses, before touching it, a buffer shorter than the header says), writes the scripted answers into the
outputs -- offsets, counts, verdicts, a buffer of its own behind the view pointer -- and records one line per call: every scalar as
name=kind:value (i c_int, which is left out, u c_uint, l c_longlong, z c_size_t), every pointer as NULL or as type[length]:contents (a run of k equal values as v*k, an xpg_rat32 as num/den or, over 1, num).
The handle is not recorded: every call that takes one is held to pass the one xpg_create gave out.

Spec tokens: `name` a scalar; `name:T[expr]` a host pointer to expr elements of T (i int32, q long long, d double, b uint8,
r xpg_rat32 = two int32); `name:D` a device pointer, recorded by value and never read; `name:V` the `const xpg_rat32 **` view;
`name:N` a `long long *` to one value; `ctx` the handle xpg_create gave out."""
import ctypes as C

import numpy as np

HANDLE = 0x51DE
DT = {"i": np.int32, "q": np.int64, "d": np.float64, "b": np.uint8, "r": np.int32}
KINDS = {"c_int": "i", "c_uint": "u", "c_long": "l", "c_ulong": "z", "c_longlong": "l", "c_ulonglong": "z", "c_double": "f"}

TABLE = {}

PACKED_TAIL = "outs:r[outs_cap_rows*cols] outs_cap_rows out_view:V "
RAGGED_IN = "mats:r[offsets[NB]] rows:i[NB] cols:i[NB] offsets:q[NB+1] rhs_idx:i[NB] "
RAGGED_TAIL = "outs:r[outs_cap_cells] outs_cap_cells out_view:V out_cell_offsets:q[NRES+1] out_rows:i[NRES] "
CHAIN_LIST = "elim:i[elim_offsets[NB]] elim_offsets:i[NB+1] "
NRES_BOUNDS = "variables(rhs_idx,cols)"                     # a length expression holds no blank


def _add(name, spec, **sub):
    for k, v in sub.items():
        spec = spec.replace(k, v)
    TABLE[name] = [(t.split(":", 1) + [None])[:2] for t in spec.split()]


def _add_kinds(name, spec, **sub):
    for k, x in (("f64", "d"), ("rat32", "r")):
        _add(name.replace("KIND", k), spec.replace(":x", ":" + x), **sub)


_add("xpg_lineq_reduce_batch_packed_rat32", "ctx nb mats:r[nb*rows*cols] rows cols rhs_idx is_intersect " + PACKED_TAIL +
     "row_offsets:q[nb+1] out_rows:i[nb] out_ok:i[nb]")
_add("xpg_lineq_fme_batch_packed_rat32", "ctx nb mats:r[nb*rows*cols] rows cols rhs_idx u darkshadow cap_rows " + PACKED_TAIL +
     "row_offsets:q[nb+1] out_ok:i[nb]")
_add("xpg_lineq_fme_batch_rat32", "ctx nb mats:r[nb*rows*cols] rows cols rhs_idx u darkshadow outs:r[nb*cap_rows*cols] cap_rows "
     "out_rows:i[nb] out_ok:i[nb]")
_add("xpg_lineq_calc_bound_batch_packed_rat32", "ctx nb mats:r[nb*rows*cols] rows cols rhs_idx cap_rows " + PACKED_TAIL +
     "row_offsets:q[nb*rhs_idx+1] out_ok:i[nb]")
for _n, _k in (("project", "nb"), ("levels", "nb*n_elim")):
    _add("xpg_lineq_%s_batch_packed_rat32" % _n, "ctx nb mats:r[nb*rows*cols] rows cols rhs_idx elim:i[n_elim] n_elim darkshadow "
         "cap_rows cap_out_rows " + PACKED_TAIL + "row_offsets:q[%s+1] out_ok:i[nb] out_steps:i[nb]" % _k)
_add("xpg_lineq_bounds_batch_packed_rat32", "ctx nb mats:r[nb*rows*cols] rows cols rhs_idx cap_rows cap_out_rows " + PACKED_TAIL +
     "row_offsets:q[nb*rhs_idx+1] out_ok:i[nb] out_chain:i[nb] out_steps:i[nb]")
for _n, _k in (("project", "nb"), ("levels", "int(elim_offsets[nb])")):
    _add("xpg_lineq_%s_batch_ragged_rat32" % _n, "ctx nb " + RAGGED_IN + CHAIN_LIST + "darkshadow cap_rows cap_out_rows " + RAGGED_TAIL +
         "out_ok:i[nb] out_steps:i[nb]", NB="nb", NRES=_k)
_add("xpg_lineq_bounds_batch_ragged_rat32", "ctx nb " + RAGGED_IN + "cap_rows cap_out_rows " + RAGGED_TAIL +
     "out_ok:i[nb] out_chain:i[nb] out_steps:i[nb]", NB="nb", NRES=NRES_BOUNDS)
HULL_TAIL = "cap_rows cap_out_rows cap_hull_rows " + RAGGED_TAIL + "out_ok:i[NRES] out_member:i[NRES] out_chain:i[NRES] out_steps:i[NRES]"
_add("xpg_lineq_hull_batch_ragged_rat32", "ctx n_groups group_offsets:i[NRES+1] n_members " + RAGGED_IN + "is_intersect " + HULL_TAIL,
     NB="n_members", NRES="n_groups")
_add("xpg_lineq_project_union_batch_ragged_rat32", "ctx n_groups group_offsets:i[NRES+1] n_members " + RAGGED_IN + CHAIN_LIST +
     "darkshadow is_intersect " + HULL_TAIL, NB="n_members", NRES="n_groups")
_add("xpg_lineq_reduce_batch_ragged_rat32", "ctx nb " + RAGGED_IN + "is_intersect out_rows:i[nb] out_ok:i[nb]", NB="nb")
_add("xpg_lineq_fme_batch_ragged_rat32", "ctx nb " + RAGGED_IN + "u:i[nb] darkshadow outs:r[outs_cap_cells] outs_cap_cells "
     "out_cell_offsets:q[nb+1] out_rows:i[nb] out_ok:i[nb]", NB="nb")

for _n in ("lineq_project", "lineq_levels", "lineq_ragged", "lineq_bounds", "lineq_bounds_ragged", "lineq_hull", "mip", "mip_hbm",
           "six_batch", "six_batch_hbm", "six_batch_vc_hbm", "has_solution_batch", "has_solution_batch_ragged", "has_solution_int_batch"):
    _add("xpg_%s_last_route" % _n, "out:q[n] n")
_add("xpg_six_last_profile", "out:d[n] n")
_add("xpg_test_vc_pattern", "kind vc:k[vc_rows*cols] vc_rows cols out_free:b[cols-1]")
_add("xpg_test_mip_hbm_plan", "kind pattern leq_rows eq_rows cols is_bin is_max extra nb num_cus out:q[n] n")
_add("xpg_test_batch_hbm_geometry", "kind R V nb num_cus out:q[n] n")
_add("xpg_test_six_batch_vc_hbm_plan", "kind vc:k[vc_rows*cols] vc_rows leq_rows eq_rows cols is_max nb num_cus out:q[n] n")
_add("xpg_test_has_solution_batch_plan", "vc:r[vc_rows*cols] vc_rows leq_rows eq_rows cols nb num_cus out:q[n] n")
_add("xpg_test_has_solution_batch_ragged_plan", "vc:r[vc_rows*cols] vc_rows cols nb leq_rows:i[nb] eq_rows:i[nb] num_cus out_route:i[nb] out:q[n] n")
_add("xpg_test_has_solution_int_plan", "vc:r[vc_rows*cols] vc_rows leq_rows eq_rows cols nb num_cus out:q[n] n")

HS_IN = "ctx nb leq:r[nb*leq_rows*cols] leq_rows eq:r[nb*eq_rows*cols] eq_rows vc:r[vc_rows*cols] vc_rows cols rhs_idx "
HS_RAGGED_IN = ("ctx nb leq:r[leq_offsets[nb]] leq_rows:i[nb] leq_offsets:q[nb+1] eq:r[eq_offsets[nb]] eq_rows:i[nb] eq_offsets:q[nb+1] "
                "vc:r[vc_rows*cols] vc_rows cols rhs_idx ")
HS_OUT = "out_has:i[nb] out_status:i[2*nb]"
_add("xpg_has_solution_batch_rat32", HS_IN + "is_int_sol is_unique_sol max_iter " + HS_OUT)
_add("xpg_has_solution_int_batch_rat32", HS_IN + "is_unique_sol " + HS_OUT)
_add("xpg_has_solution_batch_ragged_rat32", HS_RAGGED_IN + "is_int_sol is_unique_sol max_iter " + HS_OUT)
_add("xpg_has_solution_int_batch_ragged_rat32", HS_RAGGED_IN + "is_unique_sol " + HS_OUT)
_add("xpg_has_solution_batch_rat32_dev", "ctx nb leq:D leq_rows eq:D eq_rows vc:D vc_rows cols rhs_idx is_int_sol is_unique_sol max_iter "
     "out_has:D out_status:D")

SOLVED = "out_status:i[nb] out_v:x[nb] out_sol:x[nb*cols]"
VC_IN = "tgtf:x[nb*cols] vc:x[(cols-1)*cols] eq:x[nb*eq_rows*cols] eq_rows leq:x[nb*leq_rows*cols] leq_rows cols "
VC_DEV = "ctx is_max nb tgtf:D vc:D eq:D eq_rows leq:D leq_rows cols max_iter out_status:D out_v:D out_sol:D"
for _h in ("", "_hbm"):
    _add_kinds("xpg_six_batch%s_KIND" % _h, "ctx is_max nb tgtf:x[nb*cols] leq:x[nb*m*cols] m cols max_iter " + SOLVED)
    _add_kinds("xpg_six_batch%s_KIND_dev" % _h, "ctx is_max nb tgtf:D leq:D m cols max_iter out_status:D out_v:D out_sol:D out_pivots:D")
    _add_kinds("xpg_six_batch_vc%s_KIND" % _h, "ctx is_max nb " + VC_IN + "max_iter " + SOLVED)
    _add_kinds("xpg_mip_batch_vc%s_KIND" % _h, "ctx nb is_max is_bin " + VC_IN + "rational_indicator:b[cols] " + SOLVED + " out_nodes:N")
_add_kinds("xpg_six_batch_vc_KIND_dev", VC_DEV)
_add_kinds("xpg_six_batch_vc_hbm_KIND_dev", VC_DEV + " out_pivots:D")
ONE_IN = "ctx tgtf:x[cols] vc:x[vc_rows*cols] vc_rows eq:x[eq_rows*cols] eq_rows leq:x[leq_rows*cols] leq_rows cols "
for _m in ("maxm", "minm"):
    _add_kinds("xpg_six_%s_KIND" % _m, ONE_IN + "max_iter out_v:x[1] out_sol:x[cols]")
    _add_kinds("xpg_mip_%s_KIND" % _m, ONE_IN + "is_bin rational_indicator:b[cols] out_v:x[1] out_sol:x[cols]")


def fmt(values, cells=False):
    """1,1,1,1,2 -> 1*4,2; cells: (num, den) pairs as num/den, a den of 1 left out"""
    vals = ["%g" % v for v in np.asarray(values).reshape(-1).tolist()]
    if cells:
        vals = [n if d == "1" else n + "/" + d for n, d in zip(vals[0::2], vals[1::2])]
    out, k = [], 0
    while k < len(vals):
        j = k
        while j < len(vals) and vals[j] == vals[k]:
            j += 1
        out += [vals[k]] * (j - k) if j - k < 3 else ["%s*%d" % (vals[k], j - k)]
        k = j
    return ",".join(out)


def _room(arg):
    """bytes behind a pointer argument where the argument itself tells: numpy's data_as keeps its array, a ctypes array knows its size"""
    if isinstance(arg, C.Array):
        return C.sizeof(arg)
    arr = getattr(arg, "_arr", None)
    return None if arr is None else int(arr.nbytes)


def _address(arg):
    if arg is None:
        return None
    if isinstance(arg, C.Array):
        return C.addressof(arg)
    if isinstance(arg, C.c_void_p):
        return arg.value
    raise AssertionError("not a pointer argument: %r" % (arg,))


class Call:
    def __init__(self, name):
        self.name, self.s, self.a, self.out = name, {}, {}, {}


class StandIn:
    """What _capi._lib holds during a scenario. `answers` is the script: one entry per call of a TABLE entry point, in order --
    a dict {output name: values written to its front, "view": int32 values behind the view pointer, "nodes": the long long,
    "rc": the return code} or a function of the Call that returns the code. A call past the script's end answers 0."""

    def __init__(self):
        self.lines, self.answers, self.pinned = [], [], []

    def __getattr__(self, name):
        if name == "xpg_create":
            return self._create
        if name == "xpg_destroy":
            return lambda h: None
        if name == "xpg_last_error":
            return lambda h: b"scripted"
        if name in TABLE:
            return lambda *args: self._call(name, args)
        raise AttributeError("the stand-in has no %s" % name)

    @staticmethod
    def _create(out, device):
        out._obj.value = HANDLE
        return 0

    def views(self, x):
        return isinstance(x, np.ndarray) and any(np.shares_memory(x, p) for p in self.pinned)

    def _call(self, name, args):
        spec = TABLE[name]
        assert len(args) == len(spec), "%s takes %d arguments, got %d" % (name, len(spec), len(args))
        call, words = Call(name), [None] * len(spec)
        for k, ((pname, code), arg) in enumerate(zip(spec, args)):
            if pname == "ctx":
                assert isinstance(arg, C.c_void_p) and arg.value == HANDLE, "ctx is not the handle xpg_create gave out"
                words[k] = ""
            elif code is None:
                kind = KINDS.get(type(arg).__name__, type(arg).__name__)
                call.s[pname] = arg.value if hasattr(arg, "value") else arg
                words[k] = "%s=%s%s" % (pname, "" if kind == "i" else kind + ":", call.s[pname])
        env = dict(call.s)
        todo = [k for k in range(len(spec)) if words[k] is None]
        while todo:
            left = []
            for k in todo:
                (pname, code), arg = spec[k], args[k]
                if code == "V" or code == "N":
                    call.out[pname] = arg._obj
                    words[k] = "%s=%s" % (pname, {"V": "view", "N": "&" + KINDS.get(type(arg._obj).__name__, "?")}[code])
                    continue
                addr = _address(arg)
                if not addr:
                    env[pname] = None
                    words[k] = "%s=NULL" % pname
                    continue
                if code == "D":
                    words[k] = "%s=dev:%d" % (pname, addr)
                    continue
                t, expr = code[0], code[2:-1]
                if t == "k":
                    t = "dr"[call.s["kind"]]
                try:
                    n = int(eval(expr, {"int": int, "variables": lambda rhs, cols: (cols - 1 if rhs is None else rhs).sum()}, env))
                except (NameError, TypeError):
                    left.append(k)
                    continue
                n = max(n, 0)
                per = 2 if t == "r" else 1
                need = n * per * np.dtype(DT[t]).itemsize
                room = _room(arg)
                assert room is None or need <= room, "%s: %s is %d bytes, the header reads %d" % (name, pname, room, need)
                arr = np.frombuffer((C.c_byte * need).from_address(addr), dtype=DT[t]) if need else np.zeros(0, dtype=DT[t])
                env[pname] = call.a[pname] = arr
                words[k] = "%s=%s[%d]%s" % (pname, t, n, ":" + fmt(arr, t == "r") if n else "")
                if room is not None and room > need:     # more room than the header reads: recorded, in the header's element type
                    whole = np.frombuffer((C.c_byte * room).from_address(addr), dtype=np.uint8)
                    words[k] += " (room %d bytes:%s)" % (room, fmt(whole.view(DT[t]), t == "r") if room % np.dtype(DT[t]).itemsize == 0 else "?")
            assert len(left) < len(todo), "%s: lengths that never resolve: %s" % (name, [spec[k][0] for k in left])
            todo = left
        answer = self.answers.pop(0) if self.answers else {}
        if callable(answer):
            rc = answer(call)
        else:
            rc = answer.get("rc", 0)
            for pname, values in answer.items():
                if pname == "rc":
                    continue
                if pname == "view":
                    self.view(call, values)
                elif pname == "nodes":
                    call.out["out_nodes"].value = values
                else:
                    v = np.asarray(values).reshape(-1)
                    assert v.size <= call.a[pname].size, "%s: the script writes %d values into %s[%d]" % (name, v.size, pname, call.a[pname].size)
                    call.a[pname][: v.size] = v
        self.lines.append("  call %s(%s) -> %d" % (name[4:], " ".join(w for w in words if w), rc))
        return rc

    def view(self, call, n):
        """n int32 values 1 .. n in a buffer of the stand-in's own behind the call's view pointer"""
        buf = np.arange(1, n + 1, dtype=np.int32)
        self.pinned.append(buf)
        call.out["out_view"].value = buf.ctypes.data

    def show(self, x):
        if isinstance(x, np.ndarray):
            return "%s[%s]%s:%s" % ({"int32": "i32", "int64": "i64", "float64": "f64"}.get(str(x.dtype), x.dtype), ",".join(map(str, x.shape)), "view" if self.views(x) else "", fmt(x))
        if isinstance(x, (tuple, list)):
            return "%s%s%s" % ("([" [isinstance(x, list)], "; ".join(self.show(e) for e in x), ")]"[isinstance(x, list)])
        if isinstance(x, dict):
            return "{%s}" % " ".join("%s=%s" % (k, self.show(v)) for k, v in x.items())
        if isinstance(x, (np.generic, int, float)) and not isinstance(x, bool):
            return "%s:%g" % (type(x).__name__, x)
        return repr(x)

    def scenario(self, title, fn, answers=()):
        self.lines.append("== " + title)
        self.answers = list(answers)
        try:
            self.lines.append("  returns " + self.show(fn()))
        except Exception as e:                                  # noqa: BLE001 -- the type and the text are what is recorded
            self.lines.append("  raises %s: %s" % (type(e).__name__, e))
        assert not self.answers, "%s: %d scripted answers were never asked for" % (title, len(self.answers))
