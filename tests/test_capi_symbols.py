"""The C-ABI library builds for gfx950, loads, and exports exactly the symbols that
include/gnntrk.h declares; the ctypes table repeats the header's argument lists (no
compute calls: these tests need no GPU)."""

import ctypes
import pathlib
import re
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib_path():
    from gnn_tracking_amd import _build

    return _build.build_lib()


def test_header_symbols_are_exported(lib_path):
    from gnn_tracking_amd import _capi

    hdr = (ROOT / "include" / "gnntrk.h").read_text()
    declared = set(re.findall(r"\b(gnntrk_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations found"
    lib = ctypes.CDLL(str(lib_path))
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in gnntrk.h but not exported"
    assert declared == set(_capi.EXPORTED_SYMBOLS), "ctypes table out of sync with gnntrk.h"
    # and the other way round: every gnntrk_* function the library defines is one the header declares
    nm = subprocess.run(["nm", "-D", "--defined-only", str(lib_path)], check=True, capture_output=True, text=True).stdout
    defined = {f[2] for f in map(str.split, nm.splitlines()) if len(f) == 3 and f[1] in "TtWw"}
    exported = {n for n in defined if re.fullmatch(r"gnntrk_[a-z0-9_]+", n)}
    assert exported, "nm found no gnntrk_* function"
    assert exported <= declared, f"exported but not declared in gnntrk.h: {sorted(exported - declared)}"


_SCALARS = {"int": ctypes.c_int32, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t,
            "float": ctypes.c_float, "double": ctypes.c_double}
# further scalar types that appear only behind pointers
_POINTEES = {**_SCALARS, "uint8_t": ctypes.c_uint8, "uint16_t": ctypes.c_uint16, "uint32_t": ctypes.c_uint32,
             "uint64_t": ctypes.c_uint64}
_STRUCTS = {"gnntrk_seg": "Seg", "gnntrk_mlp": "Mlp", "gnntrk_mlp_fwd_args": "MlpFwdArgs",
            "gnntrk_mlp_bwd_args": "MlpBwdArgs", "gnntrk_head_bce": "HeadBce", "gnntrk_graph_index": "GraphIndex",
            "gnntrk_graph_index_carry": "GraphIndexCarry", "gnntrk_oc_args": "OcArgs", "gnntrk_resfcnn": "ResFcnn",
            "gnntrk_resfcnn_grads": "ResFcnnGrads", "gnntrk_efmlp": "EfMlp", "gnntrk_efmlp_grads": "EfMlpGrads",
            "gnntrk_edge_rows": "EdgeRows", "gnntrk_hinge_args": "HingeArgs"}


def _header_prototypes():
    """{name: (return type, [parameter type, ...])} of include/gnntrk.h; a type is the C spelling without
    `const` and the parameter's name, with one trailing `*` per pointer level."""
    hdr = (ROOT / "include" / "gnntrk.h").read_text()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)

    def ctype(decl, named):
        words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
        stars = words.count("*")
        words = [w for w in words if w != "*"]
        if named and len(words) > 1:
            words = words[:-1]          # the parameter's name
        return " ".join(words) + "*" * stars

    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_][\w \t]*?[\s*]+)(gnntrk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        args = " ".join(args.split())
        params = [] if args in ("", "void") else [ctype(a, True) for a in args.split(",")]
        assert name not in protos, f"{name} declared twice"
        protos[name] = (ctype(ret, False), params)
    return protos


def _ctypes_ok(c_type, ct, capi):
    """whether the ctypes type `ct` is an allowed binding of the C type `c_type`"""
    if not c_type.endswith("*"):
        return ct is _SCALARS.get(c_type)
    if ct is ctypes.c_void_p:
        return True
    pointee = c_type[:-1]
    if pointee == "char":
        return ct is ctypes.c_char_p
    if pointee in _POINTEES:
        return ct is ctypes.POINTER(_POINTEES[pointee])
    if pointee in _STRUCTS:
        return ct is ctypes.POINTER(getattr(capi, _STRUCTS[pointee]))
    return False


def test_ctypes_signatures_match_header():
    """Every row of _capi._SIGNATURES against its prototype: the return type, the number of parameters and each
    parameter.  A scalar maps to exactly one ctypes type; a pointer to c_void_p, c_char_p (char * only) or
    POINTER of the pointee's ctypes mirror."""
    from gnn_tracking_amd import _capi

    protos = _header_prototypes()
    assert protos and set(protos) == set(_capi._SIGNATURES)
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        res, args = _capi._SIGNATURES[name]
        if not _ctypes_ok(ret, res, _capi):
            bad.append(f"{name}: returns {ret}, bound as {res.__name__}")
        if len(args) != len(params):
            bad.append(f"{name}: {len(params)} parameters, {len(args)} bound")
            continue
        for i, (c_type, ct) in enumerate(zip(params, args)):
            if not _ctypes_ok(c_type, ct, _capi):
                bad.append(f"{name}: parameter {i} is {c_type}, bound as {ct.__name__}")
    assert not bad, "\n".join(bad)


def test_version_and_error_channel(lib_path):
    from gnn_tracking_amd import _capi

    lib = _capi.bind(ctypes.CDLL(str(lib_path)))
    assert lib.gnntrk_version() == 600
    # argument validation happens on the host, before any launch
    rc = lib.gnntrk_mlp_forward(None, None)
    assert rc == 1 and b"NULL" in lib.gnntrk_last_error()


def test_round5_entry_points_validate_on_the_host(lib_path):
    """gnntrk_node_order / gnntrk_graph_index_place refuse bad arguments before any launch (include/gnntrk.h)."""
    from gnn_tracking_amd import _capi

    lib = _capi.bind(ctypes.CDLL(str(lib_path)))
    assert lib.gnntrk_node_order_workspace_bytes(1000) >= 1000 * 24
    assert lib.gnntrk_node_order_workspace_bytes(300) < (1 << 20)   # (a small event does not pay for the largest table)
    assert lib.gnntrk_node_order(None, 1, None, 0, 0, None, None, None, 0, None) == 0      # nothing to order
    assert lib.gnntrk_node_order(None, 1, None, 0, 10, None, None, None, 0, None) == 1 and b"NULL" in lib.gnntrk_last_error()
    buf = (ctypes.c_float * 16)()
    out = (ctypes.c_int32 * 16)()
    rc = lib.gnntrk_node_order(buf, 1, None, 0, 16, out, out, buf, 8, None)
    assert rc == 1 and b"workspace" in lib.gnntrk_last_error()
    assert lib.gnntrk_node_order(buf, 1, None, 0, 1 << 32, out, out, buf, 8, None) == 4   # GNNTRK_EUNSUPPORTED: sizes must fit int32
    assert lib.gnntrk_graph_index_place(None, 0, 0, None, *([None] * 8), None) == 1
    part, batch = _capi.GraphIndex(), _capi.GraphIndex()
    part.n_nodes, part.n_edges, batch.n_nodes, batch.n_edges = 10, 20, 15, 30
    rc = lib.gnntrk_graph_index_place(ctypes.byref(part), 6, 0, ctypes.byref(batch), *([None] * 8), None)
    assert rc == 1 and b"does not fit" in lib.gnntrk_last_error()
    rc = lib.gnntrk_graph_index_place(ctypes.byref(part), 0, 0, ctypes.byref(batch), out, None, *([None] * 6), None)
    assert rc == 1 and b"pairs" in lib.gnntrk_last_error()


def test_struct_layout_matches_header():
    from gnn_tracking_amd import _capi

    assert ctypes.sizeof(_capi.Seg) == 32
    assert ctypes.sizeof(_capi.Mlp) == 64
    assert ctypes.sizeof(_capi.MlpFwdArgs) == 448
    assert _capi.MlpFwdArgs.n_rows.offset == 392
    assert ctypes.sizeof(_capi.GraphIndex) == 72
    assert ctypes.sizeof(_capi.GraphIndexCarry) == 48
    assert ctypes.sizeof(_capi.MlpBwdArgs) == 808 and ctypes.sizeof(_capi.GFold) == 24
    assert ctypes.sizeof(_capi.ResFcnn) == 8 * (5 + 2 * _capi.RESFCNN_MAX_HIDDEN) + 32
    assert ctypes.sizeof(_capi.ResFcnnGrads) == 8 * (5 + 2 * _capi.RESFCNN_MAX_HIDDEN)
    assert ctypes.sizeof(_capi.HingeArgs) == 56 and _capi.HingeArgs.r_emb.offset == 40


def test_product_path_refuses_cpu_tensors():
    import torch

    import gnn_tracking_amd as G

    with pytest.raises(RuntimeError, match="no CPU implementation"):
        G.MLP(4, 2, 8)(torch.zeros(3, 4))
