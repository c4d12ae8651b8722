"""How a row of tests/golden/fb_refusals.json becomes a call of a floating-base entry point
(include/blf/blf_c.h sections 8 to 12d), shared by tests/test_fb_refusals.py and the table's generator
tests/golden/make_fb_refusals.py.

Every call starts from the entry point's accepted empty-batch call: a fake non-null handle, a 3-joint
model whose arrays are fake non-null pointers, empty state and contact structs, batch = 0.  A row's
`args` override that: "batch": 2 sets an argument, "model.ndof": 49 a struct member, "model": null passes
a null struct pointer, "state.*": "ptr" sets every pointer member of a struct.  Values: numbers, null,
"ptr" (a fake non-null pointer) and "nan" / "inf" / "-inf".  No pointer is ever dereferenced, because no row
passes the argument checks with a batch above zero; nothing here needs a device."""
import ctypes

from blf import native

FAKE_HANDLE = 1
FAKE_ARRAY = 8
MODEL_ARRAYS = ("parent", "joint_origin", "joint_rot", "joint_axis", "link_mass", "link_com", "link_inertia")

P, I32, I64, F64 = "ptr", "i32", "i64", "f64"
_SCALARS = {ctypes.c_void_p: P, ctypes.c_int32: I32, ctypes.c_int64: I64, ctypes.c_double: F64}

# argument names and kinds (a scalar kind, or the struct class a pointer argument points to) of the
# floating-base entry points, those that take a blf_fb_model, from the binding's table of the C declarations
SIGNATURES = {entry: tuple((name, _SCALARS.get(t) or t._type_) for name, t in args)
              for entry, (_, args) in native.SIGNATURES.items()
              if ("model", ctypes.POINTER(native.FbModel)) in args}
ENTRY_POINTS = tuple(SIGNATURES)

# the accepted call: scalar arguments and struct members that are not zero / null
_DEFAULT_ARGS = {"handle": FAKE_HANDLE, "initial_time": 0.0, "final_time": 0.019, "steps": 1}
_DEFAULT_DT = {True: 0.001, False: 0.01}   # with / without the integration interval
_LAW = {"ndof": 3, "slices": 2, "steps_per_slice": 5, "kp": P, "kd": P}
_DEFAULT_MEMBERS = {
    "model": dict({k: P for k in MODEL_ARRAYS}, ndof=3),
    "impedance": _LAW,
    "law": _LAW,
    "tasks": {"joint_weight": P, "joint_kp": P},
    "schedule": {"steps": 1},
}
ABSENT = ("hard", "limits")   # optional structs: null unless a row names them


def _value(v):
    if v == P:
        return FAKE_ARRAY
    if isinstance(v, str):
        return float(v)   # "nan", "inf", "-inf"
    return v


def _set(struct, member, v):
    fields = dict(struct._fields_)
    if member == "*":
        for k, t in struct._fields_:
            if t is ctypes.c_void_p:
                setattr(struct, k, _value(v))
        return
    if member not in fields:
        raise KeyError(f"{type(struct).__name__} has no member {member}")
    setattr(struct, member, _value(v))


def invoke(entry, args):
    """Calls `entry` with the accepted empty-batch arguments overridden by `args`; returns
    (status, blf_last_error() or None when the call was accepted)."""
    sig = SIGNATURES[entry]
    timed = any(k == "initial_time" for k, _ in sig)
    for key in args:
        if key.split(".")[0] not in dict(sig):
            raise KeyError(f"{entry} has no argument {key.split('.')[0]}")
    actual, keep = [], []
    for name, kind in sig:
        if isinstance(kind, str):
            v = args.get(name, _DEFAULT_DT[timed] if name == "dT" else _DEFAULT_ARGS.get(name, 0 if kind != P else None))
            v = _value(v)
            actual.append(ctypes.c_void_p(v) if kind == P else float(v) if kind == F64 else int(v))
            continue
        members = {k.split(".", 1)[1]: v for k, v in args.items() if k.startswith(name + ".")}
        if name in args or (name in ABSENT and not members):
            assert args.get(name) is None and not members, (entry, name)
            actual.append(None)
            continue
        s = kind()
        for k, v in _DEFAULT_MEMBERS.get(name, {}).items():
            if not (name in ("impedance", "law") and k not in dict(kind._fields_)):
                _set(s, k, v)
        for k, v in sorted(members.items(), key=lambda kv: kv[0] != "*"):   # "*" first, then single members
            _set(s, k, v)
        keep.append(s)
        actual.append(ctypes.byref(s))
    status = getattr(native.lib(), entry)(*actual)
    return status, (native.last_error() if status != 0 else None)
