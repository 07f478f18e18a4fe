"""The T = 16 attention entries through the layers (no GPU needed): declared in include/msgm_hip.h, present in
_lib.SIGNATURES with the declared number of arguments, exported by the library, wrapped in ops."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("msgm_attention_small_supported", "msgm_attention_small_forward", "msgm_attention_small_dual_forward",
           "msgm_attention_small_dual_backward")


def _declared_arity():
    txt = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(msgm_attention_small_[a-z_]+)\s*\(([^)]*)\)\s*;", txt):
        out[name] = len([a for a in args.split(",") if a.strip()])
    return out


def test_entries_declared_with_matching_signatures():
    from sdeflow_light_amd import _lib
    decl = _declared_arity()
    assert set(decl) == set(ENTRIES), decl
    for n in ENTRIES:
        assert n in _lib.SIGNATURES, n
        assert len(_lib.SIGNATURES[n][1]) == decl[n], (n, decl[n], _lib.SIGNATURES[n][1])


def test_header_cites_the_reference_and_has_no_workspace_argument():
    txt = open(os.path.join(ROOT, "include", "msgm_hip.h")).read()
    block = txt[txt.index("int msgm_attention_small_supported") - 2000: txt.index("msgm_attention_small_dual_backward") + 400]
    assert block.count("model/unet.py:220-250") >= 4
    decl = re.sub(r"/\*.*?\*/", "", block[block.index("int msgm_attention_small_supported"):], flags=re.S)
    assert "workspace" not in decl


def test_library_exports_and_host_predicate():
    import __graft_entry__ as g
    g.build()
    from sdeflow_light_amd import _lib
    L = _lib.lib()
    for n in ENTRIES:
        assert hasattr(L, n), n
    ok = L.msgm_attention_small_supported                     # a pure host query: callable without a GPU
    assert all(ok(16, h, D) for h in (1, 4, 64) for D in (16, 32, 64, 128))
    assert not any(ok(t, 1, 64) for t in (4, 9, 32, 36, 64))
    assert not any(ok(16, 1, D) for D in (8, 48, 256)) and not ok(16, 0, 64) and not ok(16, 65, 64)
    assert not L.msgm_attention_supported(16, 64) and not L.msgm_attention_mh_supported(16, 2, 64)
    # null pointers are refused before anything is launched (MSGM_E_BADARG = -1)
    assert L.msgm_attention_small_forward(None, None, 1, 16, 1, 64, 0.125, None) == -1
    assert L.msgm_attention_small_dual_forward(None, None, 1, 16, 1, 64, 0.125, None) == -1
    assert L.msgm_attention_small_dual_backward(None, None, None, 1, 16, 1, 64, 0.125, None) == -1


def test_ops_wrappers_exist():
    from sdeflow_light_amd import ops
    want = {"attention_small_supported": ["T", "heads", "D"],
            "attention_small_forward": ["qkv", "out", "N", "T", "heads", "D", "scale"],
            "attention_small_dual_forward": ["qkv", "Bp", "T", "heads", "D", "scale"],
            "attention_small_dual_backward": ["qkv", "datt", "Bp", "T", "heads", "D", "scale"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(ops, name)).parameters) == params, name
