"""The argument-rule table of the host-pointer analysis and map entry points (include/tgms.h), for
tests/test_capi_errors_host.py and tests/golden/make_capi_errors.py.

Every case is one call on a host handle (tgms_create_host, no GPU): the smallest valid arguments
(B = 1, M = 1, a 2 x 2 x 2 grid, one face, one obstacle) with a few of them replaced, so that one
rule of the call's check_* function, or one generic rule (offsets, a NULL input, every output
NULL, a NULL handle), decides.  run_all() returns {case id: [status, last_error]}; for
tgms_field_edt_work_size the "status" is the size it returns.
"""
import ctypes

import numpy as np

from trajectory_generator_ros2_amd import _lib

NAN, INF, I32_MAX = float("nan"), float("inf"), 2 ** 31 - 1


def i32(x):
    return np.array(x, dtype=np.int32)


def f64(x):
    return np.array(x, dtype=np.float64)


def fld(n=(2, 2, 2), origin=(0.0, 0.0, 0.0), h=1.0):
    return _lib.Field(origin, h, n)


def base():
    """The valid arguments, by name; x(t) = t on one segment of one second."""
    C = np.zeros((1, 3, 8))
    C[0, 0, 1] = 1.0
    occ = np.zeros(8, dtype=np.uint8)
    occ[0] = 1
    return dict(B=1, so=i32([0, 1]), W=f64([[0, 0, 0], [1, 0, 0]]), T=f64([1.0]), ED=None, C=C, dt=0.1, limits=None,
                tlimits=None, g=9.8, omega=INF, s_lo=1.0, s_hi=10.0, F=1, faces=f64([[1, 0, 0, 10]]),
                fo=np.array([0, 1], dtype=np.int64), r=0.0, seg_rec=f64([[-1.0, 0.5]]), seg_face=i32([0]), mode=0,
                min_frac=0.1, t_cut=f64([0.5]), t0=None, P=1, pairs=i32([[0, 0]]), scale=None, r_min=1.0, K=1,
                obstacles=f64([[5, 5, 5, 6, 6, 6]]), field=fld(), values=np.ones(8, dtype=np.float32), lip=1.0, tol=1e-3,
                max_evals=100, r_free=0.5, max_grow=1, max_depth=1, occ=occ, max_dist=2.0, edt_mode=0)


# entry point -> its arguments after the handle, in order; "name>k": an output of element kind k
# (d fp64, f fp32, i int32, q int64), by default a zeroed buffer
SPEC = {
    "tgms_extrema_batch": "B so W T ED C dt limits ext>d flags>i",
    "tgms_bounds_batch": "B so T C limits ext>d flags>i",
    "tgms_thrust_batch": "B so T C g tlimits rec>d flags>i",
    "tgms_rate_batch": "B so T C g omega rec>d seg_rec_out>d flags>i",
    "tgms_dilate_batch": "B so T C g limits tlimits s_lo s_hi scale_out>d active>i flags>i T_out>d C_out>d",
    "tgms_corridor_batch": "B so T C F faces fo r rec>d where>i seg_rec_out>d seg_face_out>i flags>i",
    "tgms_corridor_split_batch": "B so W T C F faces fo seg_rec seg_face r mode min_frac so_out>i W_out>d T_out>d "
                                 "faces_out>d fo_out>q parent>i totals>q flags>i",
    "tgms_cut_batch": "B so W T ED C t_cut min_frac so_out>i W_out>d T_out>d ED_out>d C_out>d parent>i t0_out>d "
                      "totals>q flags>i",
    "tgms_separation_batch": "B so T C t0 P pairs scale r_min sep>d flags>i",
    "tgms_neighbors_batch": "B so T C t0 scale r_min near>d nbr>i count>i tested>i flags>i",
    "tgms_clearance_batch": "B so T C K obstacles scale r_min near>d obs>i count>i tested>i flags>i",
    "tgms_field_clearance_batch": "B so T C field values lip r_min tol max_evals near>d evals>i flags>i",
    "tgms_corridor_inflate_batch": "B so W field values r_free max_grow box>i faces_out>d fo_out>q seg_flags>i flags>i",
    "tgms_corridor_subdivide_batch": "B so W T field values r_free max_depth so_out>i W_out>d T_out>d parent>i "
                                     "seg_flags>i totals>q flags>i",
    "tgms_field_edt": "field occ max_dist edt_mode values_out>f d2>i",
}
SPEC = {k: v.split() for k, v in SPEC.items()}
KIND = {"d": np.float64, "f": np.float32, "i": np.int32, "q": np.int64}
# the inputs whose absence is "NULL pointer" (after every other rule, with B > 0)
INPUTS = {
    "tgms_extrema_batch": "W T C", "tgms_bounds_batch": "T C", "tgms_thrust_batch": "T C", "tgms_rate_batch": "T C",
    "tgms_dilate_batch": "T C", "tgms_corridor_batch": "T C", "tgms_corridor_split_batch": "W T C seg_rec seg_face",
    "tgms_cut_batch": "W T C t_cut", "tgms_separation_batch": "T C", "tgms_neighbors_batch": "T C",
    "tgms_clearance_batch": "T C obstacles", "tgms_field_clearance_batch": "T C", "tgms_corridor_inflate_batch": "W",
    "tgms_corridor_subdivide_batch": "W", "tgms_field_edt": "",
}
GRID = {"tgms_field_clearance_batch": "nodes", "tgms_corridor_inflate_batch": "table",
        "tgms_corridor_subdivide_batch": "table", "tgms_field_edt": "edt"}


def grid_cases(kind):
    """(label, field) of every refused grid: per axis n < 2, a non-finite origin and the count
    overflow (the node count cannot overflow on axis 0: n[0] alone fits), the spacing, and pairs of
    violations that pin which rule fires first."""
    out = []
    for a in range(3):
        n, o = [2, 2, 2], [0.0, 0.0, 0.0]
        n[a] = 1
        out.append((f"n[{a}]=1", fld(n)))
        o[a] = NAN
        out.append((f"origin[{a}]=nan", fld(origin=o)))
    out.append(("origin[1]=inf", fld(origin=(0.0, -INF, 0.0))))
    out.append(("n[2]=1 after origin[0]=nan", fld((2, 2, 1), (NAN, 0.0, 0.0))))
    out.append(("n[0]=1 before origin[0]=nan", fld((1, 2, 2), (NAN, 0.0, 0.0))))
    if kind == "nodes":
        big = [("axis1", (65536, 65536, 2)), ("axis2", (2048, 2048, 1024))]
        out.append(("count axis1 before origin[2]=nan", fld((65536, 65536, 2), (0.0, 0.0, NAN))))
    elif kind == "table":
        big = [("axis0", (I32_MAX, 2, 2)), ("axis1", (65535, 65535, 2)), ("axis2", (2047, 2047, 1023))]
        out.append(("count axis1 before origin[2]=nan", fld((65535, 65535, 2), (0.0, 0.0, NAN))))
        out.append(("count axis0 before n[1]=1", fld((I32_MAX, 1, 2))))
    else:
        big = [("axis0", (8, 16384, 16384)), ("axis1", (16384, 8, 16384)), ("axis2", (16384, 16384, 8))]
        out += [(f"n[{a}]=16385", fld([16385 if b == a else 2 for b in range(3)])) for a in range(3)]
        out.append(("origin[2]=nan before count", fld((16384, 16384, 8), (0.0, 0.0, NAN))))
    out += [(f"count {lab}", fld(n)) for lab, n in big]
    out.append(("count before h=0", fld(big[-1][1], h=0.0)))
    out += [(f"h={h}", fld(h=h)) for h in (0.0, -1.0, NAN, INF)]
    return out


def cases():
    """[(entry point, label, replaced arguments)]"""
    L, TL = _lib.Limits, _lib.ThrustLimits
    out = []

    def add(entry, label, **kw):
        out.append((entry, label, kw))

    for e, spec in SPEC.items():
        add(e, "ok")
        add(e, "handle NULL", handle=None)
        add(e, "every output NULL", **{a.split(">")[0]: None for a in spec if ">" in a})
        if "so" in spec:
            add(e, "B<0", B=-1)
            add(e, "so NULL", so=None)
            add(e, "so[0]!=0", so=i32([1, 2]))
            add(e, "M=0", so=i32([0, 0]))
            add(e, "M=17", so=i32([0, 17]))
            add(e, "empty batch", B=0, so=i32([0]))
        for name in INPUTS[e].split():
            add(e, f"{name} NULL", **{name: None})
        if e in GRID:
            add(e, "field NULL", field=None)
            for label, f in grid_cases(GRID[e]):
                add(e, label, field=f)

    for e in ("tgms_extrema_batch", "tgms_bounds_batch"):
        add(e, "limit nan", limits=L(v_max=NAN))
        add(e, "a_max nan", limits=L(a_max=NAN))
        add(e, "j_max nan", limits=L(j_max=NAN))
        add(e, "pmin>pmax", limits=L(pmin=(0, 1, 0), pmax=(1, 0, 1)))
        add(e, "pmin nan", limits=L(pmin=(NAN, 0, 0), pmax=(1, 1, 1)))
        add(e, "limits ok", limits=L(pmin=(-1, -1, -1), pmax=(2, 2, 2), v_max=5.0))
        add(e, "flags only ok", ext=None)
    for dt in (0.0, -1.0, NAN, INF):
        add("tgms_extrema_batch", f"dt={dt}", dt=dt)
    for e in ("tgms_thrust_batch", "tgms_rate_batch", "tgms_dilate_batch"):
        for g in (-1.0, NAN, INF):
            add(e, f"g={g}", g=g)
    for e in ("tgms_thrust_batch", "tgms_dilate_batch"):
        add(e, "f_min nan", tlimits=TL(f_min=NAN))
        add(e, "f_max nan", tlimits=TL(f_max=NAN))
        add(e, "tilt_max nan", tlimits=TL(tilt_max=NAN))
        add(e, "tlimits infinite ok", tlimits=TL(f_min=-INF, f_max=-INF, tilt_max=-INF))
    add("tgms_rate_batch", "omega nan", omega=NAN)
    add("tgms_rate_batch", "omega -inf ok", omega=-INF)
    add("tgms_rate_batch", "omega nan before outputs", omega=NAN, rec=None, seg_rec_out=None, flags=None)
    e = "tgms_dilate_batch"
    add(e, "s_lo=0", s_lo=0.0)
    add(e, "s_lo nan", s_lo=NAN)
    add(e, "s_lo>s_hi", s_lo=2.0, s_hi=1.0)
    add(e, "s_hi inf", s_hi=INF)
    add(e, "scale interval before limits", s_lo=0.0, limits=L(v_max=NAN))
    for k in ("v_max", "a_max", "j_max"):
        add(e, f"{k} nan", limits=L(**{k: NAN}))
    add(e, "tilt_max=pi/2", tlimits=TL(tilt_max=1.5707963267948966))
    add(e, "tilt_max just below pi/2 ok", tlimits=TL(tilt_max=1.5707963267948963))
    add(e, "limits before tlimits", limits=L(v_max=NAN), tlimits=TL(tilt_max=2.0))
    for e in ("tgms_corridor_batch", "tgms_corridor_split_batch"):
        add(e, "F<0", F=-1)
        add(e, "F>int32", F=2 ** 31)
        for r in (NAN, INF):
            add(e, f"r={r}", r=r)
        add(e, "faces NULL", faces=None)
        add(e, "F=0 faces NULL ok", F=0, faces=None, fo=np.array([0, 0], dtype=np.int64))
        add(e, "shared F>256", F=257, fo=None, faces_out=None, fo_out=None)
    add("tgms_corridor_batch", "shared ok", fo=None)
    add("tgms_corridor_batch", "r before outputs", r=NAN, rec=None, where=None, seg_rec_out=None, seg_face_out=None,
        flags=None)
    e = "tgms_corridor_split_batch"
    add(e, "mode=2", mode=2)
    add(e, "mode=-1", mode=-1)
    for mf in (NAN, 0.0, 0.6, INF):
        add(e, f"min_frac={mf}", min_frac=mf)
    add(e, "min_frac=0.5 ok", min_frac=0.5)
    for name in ("so_out", "totals", "W_out", "T_out", "fo_out", "faces_out"):
        add(e, f"{name} NULL", **{name: None})
    add(e, "shared ok", fo=None, faces_out=None, fo_out=None)
    add(e, "shared with faces_out", fo=None, fo_out=None)
    add(e, "shared with fo_out", fo=None, faces_out=None)
    add(e, "F=0 faces_out NULL ok", F=0, faces=None, faces_out=None, fo=np.array([0, 0], dtype=np.int64))
    add(e, "empty batch shared", B=0, so=i32([0]), fo=None, faces_out=None, fo_out=None)
    add(e, "empty batch W_out NULL ok", B=0, so=i32([0]), W_out=None, T_out=None)
    add(e, "mode before min_frac", mode=7, min_frac=NAN)
    e = "tgms_cut_batch"
    for mf in (NAN, -0.1, 1.0, INF):
        add(e, f"min_frac={mf}", min_frac=mf)
    add(e, "min_frac=0 ok", min_frac=0.0)
    for name in ("so_out", "totals", "W_out", "T_out", "ED_out"):
        add(e, f"{name} NULL", **{name: None})
    add(e, "optional outputs NULL ok", C_out=None, parent=None, t0_out=None, flags=None)
    add(e, "empty batch W_out NULL ok", B=0, so=i32([0]), W_out=None, T_out=None, ED_out=None)
    e = "tgms_separation_batch"
    add(e, "P<0", P=-1)
    add(e, "all pairs P!=B(B-1)/2", pairs=None)
    add(e, "all pairs P=0 ok", pairs=None, P=0)
    add(e, "P=0 ok before pointers", P=0, T=None, C=None)
    add(e, "r_min nan", r_min=NAN)
    add(e, "r_min=-inf ok", r_min=-INF)
    add(e, "pair out of range ok", pairs=i32([[0, 5]]))
    for e in ("tgms_separation_batch", "tgms_neighbors_batch", "tgms_clearance_batch"):
        for lab, sc in (("0", (1, 0, 1)), ("<0", (-1, 1, 1)), ("nan", (1, 1, NAN)), ("inf", (INF, 1, 1))):
            add(e, f"scale {lab}", scale=f64(sc))
        add(e, "scale ok", scale=f64((1, 2, 3)))
    for e in ("tgms_neighbors_batch", "tgms_clearance_batch"):
        for rm in (0.0, -1.0, NAN, INF):
            add(e, f"r_min={rm}", r_min=rm)
        add(e, "tested alone is no output", near=None, count=None, flags=None,
            **{"nbr" if "neighbors" in e else "obs": None})
        add(e, "flags only ok", near=None, count=None, tested=None, **{"nbr" if "neighbors" in e else "obs": None})
        add(e, "scale before r_min", scale=f64((0, 1, 1)), r_min=0.0)
    e = "tgms_clearance_batch"
    add(e, "K<0", K=-1)
    add(e, "K=0 obstacles NULL ok", K=0, obstacles=None)
    e = "tgms_field_clearance_batch"
    add(e, "values NULL", values=None)
    for tol in (0.0, NAN, INF):
        add(e, f"tol={tol}", tol=tol)
    for rm in (0.0, -1.0, NAN):
        add(e, f"r_min={rm}", r_min=rm)
    add(e, "r_min=inf ok", r_min=INF)
    for lip in (-1.0, NAN, INF):
        add(e, f"lip={lip}", lip=lip)
    add(e, "lip=0 ok", lip=0.0)
    add(e, "max_evals=0", max_evals=0)
    add(e, "h before tol", field=fld(h=0.0), tol=0.0)
    add(e, "tol before r_min before lip", tol=0.0, r_min=0.0, lip=-1.0)
    add(e, "r_min before lip", r_min=0.0, lip=-1.0)
    for e in ("tgms_corridor_inflate_batch", "tgms_corridor_subdivide_batch"):
        add(e, "values NULL", values=None)
        for rf in (NAN, INF):
            add(e, f"r_free={rf}", r_free=rf)
        add(e, "grid before values", field=fld(h=0.0), values=None)
    e = "tgms_corridor_inflate_batch"
    add(e, "max_grow<0", max_grow=-1)
    add(e, "max_grow=0 ok", max_grow=0)
    add(e, "outputs before r_free", r_free=NAN, box=None, faces_out=None, fo_out=None, seg_flags=None, flags=None)
    e = "tgms_corridor_subdivide_batch"
    for d in (-1, 5):
        add(e, f"max_depth={d}", max_depth=d)
    add(e, "max_depth=0 ok", max_depth=0)
    add(e, "T without T_out", T_out=None)
    add(e, "T_out without T", T=None)
    add(e, "no times ok", T=None, T_out=None)
    for name in ("so_out", "totals", "W_out"):
        add(e, f"{name} NULL", **{name: None})
    add(e, "empty batch W_out NULL ok", B=0, so=i32([0]), W_out=None)
    add(e, "totals before r_free", totals=None, r_free=NAN)
    e = "tgms_field_edt"
    for m in (2, 3, -1):
        add(e, f"mode={m}", edt_mode=m)
    add(e, "signed ok", edt_mode=1)
    for md in (0.0, -1.0, NAN, INF):
        add(e, f"max_dist={md}", max_dist=md)
    add(e, "occ NULL", occ=None)
    add(e, "values only ok", d2=None)
    add(e, "d2 only ok", values_out=None)
    add(e, "mode before max_dist", edt_mode=2, max_dist=0.0)
    add(e, "grid before mode", field=fld(h=NAN), edt_mode=2)
    add(e, "max_dist before occ", max_dist=0.0, occ=None)
    return out


def case_id(c):
    return f"{c[0]}: {c[1]}"


def _arg(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if isinstance(v, ctypes.Structure):
        return ctypes.byref(v)
    return v


def run_case(L, h, case):
    """(status, last_error) of one case on the handle h (a ctypes.c_void_p)."""
    entry, _, kw = case
    a = base()
    for name in SPEC[entry]:
        if ">" in name:
            a[name.split(">")[0]] = np.zeros(256, dtype=KIND[name.split(">")[1]])
    a.update(kw)
    hh = a.get("handle", h)
    st = getattr(L, entry)(hh, *[_arg(a[name.split(">")[0]]) for name in SPEC[entry]])
    return [int(st), L.tgms_last_error(hh).decode()]


def gpu_only_entries():
    """The entry points a host handle refuses at the door (enter)."""
    return [e for e in _lib.EXPORTS if e.endswith("_device")] + ["tgms_refine_batch", "tgms_solve_batch_multi"]


def run_gpu_only(L, h, entry):
    fn = getattr(L, entry)
    zero = [0.0 if t is ctypes.c_double else 0 if t in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64) else None
            for t in fn.argtypes[1:]]
    return [int(fn(h, *zero)), L.tgms_last_error(h).decode()]


def run_all(L):
    h = ctypes.c_void_p()
    assert L.tgms_create_host(ctypes.byref(h)) == _lib.OK
    try:
        table = cases()
        got = {case_id(c): run_case(L, h, c) for c in table}
        assert len(got) == len(table), "case ids must be unique"
        for e in gpu_only_entries():
            got[f"{e}: host handle"] = run_gpu_only(L, h, e)
        for signed in (0, 1):
            got[f"tgms_field_edt_work_size: ok mode={signed}"] = [int(L.tgms_field_edt_work_size(ctypes.byref(fld()), signed)), ""]
        got["tgms_field_edt_work_size: ok 5x4x3"] = [int(L.tgms_field_edt_work_size(ctypes.byref(fld((5, 4, 3))), 0)), ""]
        got["tgms_field_edt_work_size: field NULL"] = [int(L.tgms_field_edt_work_size(None, 0)), ""]
        got["tgms_field_edt_work_size: mode=2"] = [int(L.tgms_field_edt_work_size(ctypes.byref(fld()), 2)), ""]
        for label, f in grid_cases("edt"):
            got[f"tgms_field_edt_work_size: {label}"] = [int(L.tgms_field_edt_work_size(ctypes.byref(f), 0)), ""]
    finally:
        L.tgms_destroy(h)
    return got


def pack(got):
    """The fixture's form of run_all()'s result: every distinct message once, and per entry point
    {label: [status, index of the message]}."""
    msgs = sorted({m for _, m in got.values()})
    cases = {}
    for k, (st, m) in got.items():
        entry, label = k.split(": ", 1)
        cases.setdefault(entry, {})[label] = [st, msgs.index(m)]
    return {"messages": msgs, "cases": cases}


def unpack(fixture):
    return {f"{e}: {label}": [st, fixture["messages"][i]] for e, c in fixture["cases"].items() for label, (st, i) in c.items()}
