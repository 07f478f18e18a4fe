"""msgm_forward_paths through the layers (no GPU needed): declared in include/msgm_hip.h, present in _lib.SIGNATURES with
the declared arguments, exported by the library, wrapped in ops and sde_scheme."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "msgm_forward_paths"


def _declaration():
    txt = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    found = re.findall(r"\b" + NAME + r"\s*\(([^)]*)\)\s*;", txt)
    assert len(found) == 1, found
    return [a.strip() for a in found[0].split(",") if a.strip()]


def _ctype(arg):
    if "*" in arg or arg.startswith("msgm_stream_t"):
        return "ptr"
    return {"int64_t": C.c_int64, "int32_t": C.c_int32, "float": C.c_float}[arg.split()[0]]


def test_declaration_and_binding_agree():
    from sdeflow_light_amd import _lib
    args = _declaration()
    assert [a.split()[-1].lstrip("*") for a in args] == ["x0", "y_all", "B", "n", "sde", "nsf", "first_keep", "ts", "delta",
                                                        "sqrt_delta", "t_half", "t_full", "z_main", "rng", "stream"]
    res, bound = _lib.SIGNATURES[NAME]
    assert res is C.c_int and len(bound) == len(args)
    for a, b in zip(args, bound):
        want = _ctype(a)
        if want == "ptr":
            assert b is C.c_void_p or (isinstance(b, type) and issubclass(b, C._Pointer)), (a, b)
        else:
            assert b is want, (a, b)


def test_header_cites_the_reference_lines():
    txt = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    block = txt[txt.index("int " + NAME) - 2000: txt.index("int " + NAME)]
    assert "SDEs.py:648-706" in block and "SDEs.py:124-132" in block


def test_library_exports_and_refuses_null_arguments():
    import __graft_entry__ as g
    g.build()
    from sdeflow_light_amd import _lib
    L = _lib.lib()
    assert hasattr(L, NAME)
    # null pointers are refused before anything is launched (MSGM_E_BADARG = -1)
    assert L.msgm_forward_paths(None, None, 2, 8, None, 4, 0, None, 0.25, 0.5, 0.125, 0.25, None, None, None) == -1


def test_wrappers_exist():
    from sdeflow_light_amd import ops, sde_scheme
    assert list(inspect.signature(ops.forward_paths).parameters) == ["x0", "sde", "nsf", "first_keep", "ts", "delta", "z_main", "rng"]
    assert list(inspect.signature(sde_scheme.msgm_forward_paths).parameters) == ["base", "y0", "first_keep", "noise"]
    assert list(inspect.signature(sde_scheme.msgm_forward_paths_composed).parameters) == ["base", "y0", "first_keep", "noise"]
