"""The ctypes binding is computed from include/msgm_hip.h (sdeflow_light_amd/_abi.py); no GPU needed.  The struct layouts are
checked against the compiler, the reader must refuse what it does not understand, a struct pointer must not take an int,
and the header's constants must equal the values the Python names have always had."""
import ctypes
import os
import re
import subprocess

import pytest

from sdeflow_light_amd import _abi, _lib, ops
from sdeflow_light_amd.build import _hipcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"SdeT": 40, "MlpParamsT": 72, "ConvGeomT": 52, "ConvFuseT": 88, "ReduceJobT": 88, "PackJobT": 72, "DropoutT": 24,
         "EmbJobT": 64}


def test_struct_layouts_match_the_compiler(tmp_path):
    abi = _abi.load()
    assert {c.__name__: ctypes.sizeof(c) for c in abi.classes.values() if c.__name__ in SIZES} == SIZES
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "msgm_hip.h"', "int main() {"]
    for s, fields in abi.structs.items():
        lines.append(f'  std::printf("{s} - %zu %zu\\n", (size_t)0, sizeof({s}));')
        lines += [f'  std::printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for f, _ in fields]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}"]) + "\n")
    subprocess.run([_hipcc(), "-x", "c++", "-std=c++17", "-O0", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    compiled = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    derived = []
    for s, fields in abi.structs.items():
        cls = abi.classes[s]
        assert [f for f, _ in cls._fields_] == [f for f, _ in fields]
        derived.append(f"{s} - 0 {ctypes.sizeof(cls)}")
        derived += [f"{s} {f} {getattr(cls, f).offset} {getattr(cls, f).size}" for f, _ in fields]
    assert compiled == derived
    assert len(abi.structs) == 10 and {getattr(_lib, c.__name__) for c in abi.classes.values()} == set(abi.classes.values())


OK_HEADER = "typedef struct { int32_t a, b[4]; const float* p; } msgm_s_t;\nint msgm_f(const msgm_s_t* s, int64_t n);\n"


@pytest.mark.parametrize("text, line", [
    ("int msgm_f(int32_t a);\nint msgm_g(long x);\n", 2),                                  # an unknown type
    ("\n\nint msgm_f(int32_t a, float);\n", 3),                                            # a parameter without a name
    ("int msgm_f(int32_t);\n", 1),
    ("int msgm_f(int32_t a);\nint msgm_f(int32_t a);\n", 2),                               # a duplicate prototype
    ("int msgm_f(const msgm_x_t* x);\n", 1),                                               # a pointer to an undeclared struct
    ("int msgm_f(const msgm_x_t* x_dev);\n", 1),
    ("int msgm_f(msgm_stream_t a, msgm_stream_t a);\n", 1),                                # a duplicate parameter
    ("typedef struct { int32_t a; long b; } msgm_s_t;\n", 1),                              # unknown field type
    ("typedef struct { int32_t a, a; } msgm_s_t;\n", 1),                                   # duplicate field
    ("typedef struct { float* p, q; } msgm_s_t;\n", 1),                                    # pointer with several declarators
    ("typedef struct { int32_t a; } msgm_s_t;\ntypedef struct { float b; } msgm_s_t;\n", 2),
    ("enum { MSGM_A = 0, MSGM_A = 1 };\n", 1),
    ("enum { MSGM_A = 1 << 2 };\n", 1),                                                    # not a plain integer
    ("#define MSGM_A (1)\n", 1),
    ("/* c */\nint msgm_f(int32_t a, float** b);\n", 2),                                   # an unparsable declarator
    ("int msgm_f(int32_t a[4]);\n", 1),
    ("float* msgm_f(int32_t a);\n", 1),                                                    # a pointer result other than const char*
    ("int other_f(int32_t a);\n", 1),                                                      # not an msgm_* prototype
    ("int msgm_f(int32_t a)\n", 1),                                                        # no semicolon
    (OK_HEADER + "}\n", 3),                                                                # a stray brace
])
def test_reader_refuses_what_it_does_not_understand(text, line):
    with pytest.raises(_lib.MsgmError, match=rf"msgm_hip\.h:{line}:"):
        _abi.parse(text)


def test_reader_accepts_the_small_header():
    abi = _abi.parse(OK_HEADER)
    S = abi.classes["msgm_s_t"]
    assert S.__name__ == "ST" and abi.structs["msgm_s_t"] == [("a", ctypes.c_int32), ("b", ctypes.c_int32 * 4), ("p", ctypes.c_void_p)]
    assert abi.functions == {"msgm_f": (ctypes.c_int, [("s", ctypes.POINTER(S)), ("n", ctypes.c_int64)])}
    assert _abi.parse("enum { MSGM_A, MSGM_B = -2, MSGM_C };\n#define MSGM_D 0x10\n#define MSGM_GUARD_H\n").constants == {
        "MSGM_A": 0, "MSGM_B": -2, "MSGM_C": -1, "MSGM_D": 16}


def test_struct_pointer_takes_the_struct_and_refuses_an_int():
    abi = _abi.load()
    assert _abi.load() is abi and _lib._ABI is abi                    # the header is read once per process
    hdr = re.sub(r"/\*.*?\*/", "", open(_abi.HEADER_PATH).read(), flags=re.S)
    names = re.findall(r"\bmsgm_\w+_t\s*\*\s*(\w+)\s*[,)]", hdr)         # every struct-pointer parameter of the header
    by_ref, tables = 0, 0
    for fn, (res, params) in abi.functions.items():
        assert _lib.SIGNATURES[fn] == (res, [t for _, t in params])
        for name, t in params:
            if isinstance(t, type) and issubclass(t, ctypes._Pointer):
                cls = t._type_
                assert issubclass(cls, ctypes.Structure) and t is ctypes.POINTER(cls) and not name.endswith("_dev"), (fn, name)
                t.from_param(cls())                                    # ctypes passes the instance by reference
                t.from_param(ctypes.byref(cls()))
                t.from_param(None)
                for bad in (0, 1 << 40, 1.0):
                    with pytest.raises(TypeError):                     # in a call: ctypes.ArgumentError
                        t.from_param(bad)
                by_ref += 1
            elif name.endswith("_dev") and name in names:
                assert t is ctypes.c_void_p, (fn, name)
                tables += 1
    assert by_ref == sum(not n.endswith("_dev") for n in names) and by_ref > 40
    assert by_ref + tables == len(names)


def test_header_constants_equal_the_python_names():
    want = dict(MSGM_OK=0, MSGM_E_UNSUPPORTED=-2, SDE_SGM=0, SDE_MSGM_SPARSE=1, SDE_MSGM_DENSE=2, PROC_REVERSE=0, PROC_FORWARD=1,
                METHOD_EM=0, METHOD_HEUN=1, METHOD_RK4=2, DATA_SWISS=0, DATA_GAUSSIAN=1, DATA_CAUCHY=2, DATA_GAUSSIAN_CAUCHY=3,
                RNG_STREAM_T=0, RNG_STREAM_EPS=1, RNG_STREAM_V=2, RNG_STREAM_DW=3, RNG_STREAM_ROWS=4, RNG_STREAM_USER=16,
                RNG_STREAM_DATA=5, RNG_STREAM_DATA_ELEM=6, RNG_STREAM_DATA_CALL=7, RNG_STREAM_DROPOUT=64)
    assert {k: getattr(_lib, k) for k in want} == want
    want = dict(DECAY_NONE=0, DECAY_L2=1, DECAY_DECOUPLED=2, _OPTIM_CLIP=1, _OPTIM_EMA_WARMUP=2)
    assert {k: getattr(ops, k) for k in want} == want
    assert _lib.CONSTANTS == dict(
        MSGM_OK=0, MSGM_E_BADARG=-1, MSGM_E_UNSUPPORTED=-2, MSGM_E_WORKSPACE=-3, MSGM_E_LAUNCH=-4, MSGM_SDE_SGM=0,
        MSGM_SDE_MSGM_SPARSE=1, MSGM_SDE_MSGM_DENSE=2, MSGM_PROC_REVERSE=0, MSGM_PROC_FORWARD=1, MSGM_DATA_SWISS=0,
        MSGM_DATA_GAUSSIAN=1, MSGM_DATA_CAUCHY=2, MSGM_DATA_GAUSSIAN_CAUCHY=3, MSGM_METHOD_EM=0, MSGM_METHOD_HEUN=1,
        MSGM_METHOD_RK4=2, MSGM_DECAY_NONE=0, MSGM_DECAY_L2=1, MSGM_DECAY_DECOUPLED=2, MSGM_OPTIM_CLIP=1, MSGM_OPTIM_EMA_WARMUP=2)
