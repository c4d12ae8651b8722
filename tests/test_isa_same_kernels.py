"""tools/isa_same_kernels.py's pairing and classification on two small synthetic listings: no compiler
runs, the tool's compare() takes the listings as text."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_same_kernels", os.path.join(ROOT, "tools", "isa_same_kernels.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


def listing(*funcs):
    """A listing in the compiler's layout: (function index, mangled name, body lines) each."""
    out = ["\t.text", "\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\""]
    for idx, name, body in funcs:
        out += [f"\t.globl\t{name}", f"{name}: ; @{name}", "; %bb.0:"]
        out += ["\t" + ln.replace("@", str(idx)) for ln in body]
        out += [f".Lfunc_end{idx}:", f"\t.size\t{name}, .Lfunc_end{idx}-{name}", "\t.section\t.rodata"]
    return "\n".join(out) + "\n"


BODY = ["s_load_dwordx2 s[4:5], s[0:1], 0x8",
        "s_load_dword s2, s[0:1], 0xe0          ; nsteps",
        "s_waitcnt lgkmcnt(0)",
        "s_cmp_lt_i32 s2, 1",
        "s_cbranch_scc1 .LBB@_2",
        ".LBB@_1:",
        "v_add_f64 v[0:1], v[0:1], v[2:3]",
        "s_add_i32 s2, s2, -1",
        "s_cmp_lg_u32 s2, 0",
        "s_cbranch_scc1 .LBB@_1",
        ".LBB@_2:",
        "s_endpgm"]


def changed(old, new):
    return [ln.replace(old, new) for ln in BODY]


OLD = listing((0, "_Z4keepILi32EEvPd", BODY), (1, "_Z9traj_kernILi32EEvPd", BODY), (2, "_Z8ctq_kernILi32EEvPd", BODY),
              (3, "_Z4regsILi32EEvPd", BODY), (4, "_Z4goneILi32EEvPd", BODY))
# a kernel added in front renumbers every block label; the two renamed kernels follow it
NEW = listing((0, "_Z5addedILi32EEvPd", BODY), (1, "_Z4keepILi32EEvPd", BODY),
              (2, "_Z4kernILi32E4TrajEvPd", BODY),
              (3, "_Z4kernILi32E3CtqEvPd", changed("s[0:1], 0xe0", "s[0:1], 0xe4")),
              (4, "_Z4regsILi32EEvPd", changed("v[2:3]", "v[4:5]")))
RENAMES = [(r"_Z9traj_kernILi32EE", "_Z4kernILi32E4TrajE"), (r"_Z8ctq_kernILi32EE", "_Z4kernILi32E3CtqE")]


def test_pairing_and_verdicts():
    res, nold, nnew = tool.compare(OLD, NEW, RENAMES)
    assert (nold, nnew) == (5, 5)
    verdict = {k: v[0] for k, v in res.items()}
    assert verdict == {"_Z4keepILi32EEvPd": "identical",             # a renumbered block label is no difference
                       "_Z9traj_kernILi32EEvPd": "identical",        # paired through its rename
                       "_Z8ctq_kernILi32EEvPd": "kernarg-offset",    # one kernarg load's offset moved
                       "_Z4regsILi32EEvPd": "differs",               # a register changed
                       "_Z4goneILi32EEvPd": "missing"}
    assert len(res["_Z8ctq_kernILi32EEvPd"][1]) == 1
    a, b = res["_Z8ctq_kernILi32EEvPd"][1][0]
    assert a.endswith("0xe0") and b.endswith("0xe4")


def test_without_the_rename_the_function_is_missing():
    res, _, _ = tool.compare(OLD, NEW)
    assert res["_Z9traj_kernILi32EEvPd"][0] == "missing" and res["_Z8ctq_kernILi32EEvPd"][0] == "missing"
    assert res["_Z4keepILi32EEvPd"][0] == "identical"


def test_kernarg_class_needs_the_same_opcode_registers_and_line_count():
    body = lambda s: listing((0, "_Z1kv", s))
    verdict = lambda s: tool.compare(body(BODY), body(s))[0]["_Z1kv"][0]
    assert verdict(changed("s_load_dword s2, s[0:1], 0xe0", "s_load_dword s3, s[0:1], 0xe4")) == "differs"
    assert verdict(changed("s_load_dword s2, s[0:1], 0xe0", "s_load_dwordx2 s[2:3], s[0:1], 0xe4")) == "differs"
    assert verdict(changed("s[0:1], 0xe0", "s[6:7], 0xe4")) == "differs"       # not the kernarg pointer
    assert verdict(changed("s[0:1], 0xe0", "s[0:1], 0xe4") + ["s_nop 0"]) == "differs"
    # the offset of a branch target or of a vector instruction is not a kernarg load's
    assert verdict(changed("s_add_i32 s2, s2, -1", "s_add_i32 s2, s2, -2")) == "differs"
