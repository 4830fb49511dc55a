"""Host side of the one-launch route for dense-coded graphs of 129 to 448 nodes (csrc/mid_graph.hip): the entry points are exported,
declared and bound; the route query proves the LDS budget over the WHOLE admitted domain; what the kernels do not cover is
refused before any HIP call, with the offending value named; the Python predicate's edges.  No GPU."""
import ctypes
import os
import re
import types

import pytest
import torch

from gnan_amd import HopGraph, _lib
from gnan_amd import small_graph as sg
from gnan_amd.functional import StackedMLP
from conftest import ROOT

SYMBOLS = ("gnan_mid_graph_fwd", "gnan_mid_graph_bwd", "gnan_mid_graph_workspace_bytes", "gnan_mid_graph_bwd_workspace_bytes",
           "gnan_mid_graph_describe")
STRUCTS = (("gnan_mid_graph_args", "MidGraphArgs"), ("gnan_mid_graph_bwd_args", "MidGraphBwdArgs"),
           ("gnan_mid_graph_info", "MidGraphInfo"))
LDS_PER_CU = 160 * 1024


def header():
    with open(os.path.join(ROOT, "include", "gnan_hip.h")) as f:
        return f.read()


def test_symbols_are_exported_declared_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    # the entry points were ADDED (no struct of the ABI changed): the library, the header and the binding agree on the number
    number = int(re.search(r"^#define GNAN_ABI_VERSION (\d+)$", header(), re.M).group(1))
    assert _lib.lib().gnan_abi_version() == _lib.ABI_VERSION == number


def test_struct_layouts_match_the_header():
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "gnan_small_mlp": _lib.SmallMlp,
               "gnan_small_mlp_grads": _lib.SmallMlpGrads}
    for struct, cls_name in STRUCTS:
        cls = getattr(_lib, cls_name)
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            words = decl.replace("const ", "").split(None, 1)
            for name in words[1].split(","):
                name = name.strip()
                pointer = name.startswith("*") or words[0].endswith("*")
                fields.append((name.lstrip("*").strip(), ctypes.c_void_p if pointer else c_types[words[0]]))
        assert fields == list(cls._fields_), struct


def test_lds_budget_over_the_whole_domain():
    """Every admitted (n, D, C): ceil(n / 64) row tiles, both kernels inside one compute unit's LDS, and the workspace sizes the
    query reports are the ones the *_workspace_bytes calls return."""
    lib = _lib.lib()
    info = _lib.MidGraphInfo()
    F = 15
    worst = 0
    for n in range(129, 449):
        for D in (2, 17, 64):
            for C in (1, 8):
                assert lib.gnan_mid_graph_describe(n, F, D, C, info) == 0, (n, D, C, lib.gnan_last_error())
                assert info.row_tiles == -(-n // 64), (n, info.as_dict())
                assert 1 <= info.rho_groups <= n and info.fwd_grid == F + 1 and info.bwd_grid == F + info.rho_groups
                assert 0 < info.fwd_lds_bytes <= LDS_PER_CU and 0 < info.bwd_lds_bytes <= LDS_PER_CU, (n, D, C, info.as_dict())
                assert info.fwd_workspace_bytes == lib.gnan_mid_graph_workspace_bytes(n, F, C)
                assert info.bwd_workspace_bytes == lib.gnan_mid_graph_bwd_workspace_bytes(n, D)
                worst = max(worst, info.fwd_lds_bytes, info.bwd_lds_bytes)
    assert worst <= 96 * 1024, worst          # the design's aim: two workgroups per compute unit


def _mlp(L=3, H=64, C=1, bias=True, base=0x1000):
    """A gnan_small_mlp of made-up (never dereferenced) addresses."""
    return _lib.SmallMlp(L=L, H=H, C=C, w_first=base, b_first=base + 0x100 if bias else None, w_mid=base + 0x200 if L == 3 else None,
                         b_mid=base + 0x300 if (L == 3 and bias) else None, w_last=base + 0x400, b_last=base + 0x500 if bias else None)


def _grads(m, base=0x9000):
    return _lib.SmallMlpGrads(w_first=base, b_first=base + 0x100 if m.b_first else None, w_mid=base + 0x200 if m.L == 3 else None,
                              b_mid=base + 0x300 if m.b_mid else None, w_last=base + 0x400, b_last=base + 0x500 if m.b_last else None)


def _fwd_args(n=200, F=15, D=12, f=None, rho=None, **over):
    f = f or _mlp()
    rho = rho or _mlp(bias=False, base=0x2000)
    need = _lib.lib().gnan_mid_graph_workspace_bytes(n, F, f.C)
    kw = dict(x=0x100000, x_stride=F, n=n, F=F, f=f, rho=rho, code=0x200000, D=D, reserved=0, cnt=0x300000, cnt_stride=D, S=0x400000,
              lut=0x500000, Y=None, Ysum=0x600000, workspace=0x700000, workspace_bytes=need)
    kw.update(over)
    return _lib.MidGraphArgs(**kw)


def _bwd_args(n=200, F=15, D=12, f=None, rho=None, **over):
    f = f or _mlp()
    rho = rho or _mlp(bias=False, base=0x2000)
    need = _lib.lib().gnan_mid_graph_bwd_workspace_bytes(n, D)
    kw = dict(x=0x100000, x_stride=F, n=n, F=F, f=f, rho=rho, code=0x200000, D=D, reserved=0, cnt=0x300000, cnt_stride=D, S=0x400000,
              lut=0x500000, dY=None, dYsum=0x600000, df=_grads(f), drho=_grads(rho, 0xA000), workspace=0x700000, workspace_bytes=need)
    kw.update(over)
    return _lib.MidGraphBwdArgs(**kw)


@pytest.mark.parametrize("what,kw,named", [
    ("n", dict(n=449), b"n=449"), ("D", dict(D=65), b"D=65"), ("C", dict(f=_mlp(C=9)), b"C=9"), ("H", dict(f=_mlp(H=65)), b"H=65"),
    ("L", dict(f=_mlp(L=4)), b"L=4"), ("rho.C", dict(rho=_mlp(C=2, bias=False, base=0x2000)), b"rho.C=2")])
def test_shapes_outside_the_cover_are_refused_by_name(what, kw, named):
    lib = _lib.lib()
    for call, args in ((lib.gnan_mid_graph_fwd, _fwd_args(**kw)), (lib.gnan_mid_graph_bwd, _bwd_args(**kw))):
        assert call(args, None) == _lib.ERR_UNSUPPORTED, what
        assert named in lib.gnan_last_error(), (what, lib.gnan_last_error())
    if what in ("n", "D", "C"):
        info = _lib.MidGraphInfo()
        shape = dict(n=200, F=15, D=12, C=1)
        shape.update({"n": kw.get("n", 200), "D": kw.get("D", 12), "C": kw["f"].C if "f" in kw else 1})
        assert lib.gnan_mid_graph_describe(shape["n"], shape["F"], shape["D"], shape["C"], info) == _lib.ERR_UNSUPPORTED
        assert named in lib.gnan_last_error()


def test_bad_arguments_are_refused_before_any_hip_call():
    """A null stream and made-up addresses on a machine without a GPU: every refusal comes from the host-side checks."""
    lib = _lib.lib()
    need = lib.gnan_mid_graph_workspace_bytes(200, 15, 1)
    assert need == 16 + 15 * 200 * 4
    assert lib.gnan_mid_graph_fwd(_fwd_args(workspace_bytes=need - 1), None) == _lib.ERR_WORKSPACE
    assert str(need).encode() in lib.gnan_last_error() and str(need - 1).encode() in lib.gnan_last_error()
    need_b = lib.gnan_mid_graph_bwd_workspace_bytes(200, 12)
    assert lib.gnan_mid_graph_bwd(_bwd_args(workspace_bytes=need_b - 1), None) == _lib.ERR_WORKSPACE
    assert str(need_b).encode() in lib.gnan_last_error()
    for call, make in ((lib.gnan_mid_graph_fwd, _fwd_args), (lib.gnan_mid_graph_bwd, _bwd_args)):
        assert call(make(code=None), None) == _lib.ERR_BAD_ARG and b"null code" in lib.gnan_last_error()
        assert call(make(x_stride=14), None) == _lib.ERR_BAD_ARG
        assert b"x_stride=14" in lib.gnan_last_error() and b"F=15" in lib.gnan_last_error()
        assert call(make(cnt_stride=11), None) == _lib.ERR_BAD_ARG and b"cnt_stride=11" in lib.gnan_last_error()
        assert call(make(code=0x200001), None) == _lib.ERR_BAD_ARG and b"aligned" in lib.gnan_last_error()
        assert call(make(n=0), None) == _lib.ERR_BAD_ARG and b"n=0" in lib.gnan_last_error()
    # a bias gradient exactly where there is a bias: one missing, one too many
    f = _mlp()
    missing = _grads(f)
    missing.b_first = None
    assert lib.gnan_mid_graph_bwd(_bwd_args(df=missing), None) == _lib.ERR_BAD_ARG and b"bias" in lib.gnan_last_error()
    rho = _mlp(bias=False, base=0x2000)
    extra = _grads(rho, 0xA000)
    extra.b_last = 0xA500
    assert lib.gnan_mid_graph_bwd(_bwd_args(drho=extra), None) == _lib.ERR_BAD_ARG and b"bias" in lib.gnan_last_error()
    assert lib.gnan_mid_graph_bwd(_bwd_args(dYsum=None), None) == _lib.ERR_BAD_ARG
    # gnan_small_graph_fwd keeps refusing what is now this route's
    small = _lib.SmallGraphArgs(x=0x100000, x_stride=15, n=129, F=15, f=_mlp(), rho=_mlp(bias=False, base=0x2000), code=0x200000, D=12,
                                pre_rho=0, cnt=None, cnt_stride=0, S=0x400000, lut=0x500000, Y=None, Ysum=0x600000,
                                workspace=0x700000, workspace_bytes=1 << 20)
    assert lib.gnan_small_graph_fwd(small, None) == _lib.ERR_UNSUPPORTED


class _FakeCuda:
    """What the predicate reads of a device tensor, on a machine without a device."""
    is_cuda, dtype, requires_grad = True, torch.float32, False

    def __init__(self, n, F, requires_grad=False):
        self.shape, self.requires_grad = (n, F), requires_grad


def test_the_predicate():
    F = 5
    t = lambda *s: torch.zeros(*s)        # noqa: E731
    f = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 1, 8), t(F, 1), 3, 8, 1, F)
    rho = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 1, 8), None, 3, 8, 1, 1)
    rho2 = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 2, 8), None, 3, 8, 2, 1)
    assert sg.MID_GRAPH is True and sg.SMALL_GRAPH_MAX_NODES == 128 and sg.SLOT_MAX_NODES == 128
    assert sg.MID_GRAPH_MAX_NODES <= 448

    def dense(n):             # (what the predicate reads of a dense-coded graph: building one takes a device)
        return types.SimpleNamespace(is_dense=True, n_rows=n, n_cols=n, n_codes=2, cnt=torch.ones(n, 2, dtype=torch.int32))
    graphs = {n: dense(n) for n in (128, 129, sg.MID_GRAPH_MAX_NODES, 449)}
    assert not sg.mid_graph_applies(torch.zeros(129, F), graphs[129], f, rho)                 # CPU tensors
    assert sg.mid_graph_applies(_FakeCuda(129, F), graphs[129], f, rho)                       # ... the same on a device
    assert sg.mid_graph_applies(_FakeCuda(sg.MID_GRAPH_MAX_NODES, F), graphs[sg.MID_GRAPH_MAX_NODES], f, rho)
    assert not sg.mid_graph_applies(_FakeCuda(128, F), graphs[128], f, rho)
    assert not sg.mid_graph_applies(_FakeCuda(449, F), graphs[449], f, rho)
    assert not sg.mid_graph_applies(_FakeCuda(129, F, requires_grad=True), graphs[129], f, rho)
    assert not sg.mid_graph_applies(_FakeCuda(129, F), graphs[129], f, rho, use_cnt="pre")
    assert not sg.mid_graph_applies(_FakeCuda(129, F), graphs[129], f, rho2)                  # a rho channel per output channel
    assert not sg.mid_graph_applies(_FakeCuda(129, F + 1), graphs[129], f, rho)
    n = 129
    csr = HopGraph.from_csr(torch.arange(n + 1), torch.arange(n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8), n_cols=n,
                            n_codes=2)
    assert not sg.mid_graph_applies(_FakeCuda(n, F), csr, f, rho)
    old = sg.MID_GRAPH
    sg.MID_GRAPH = False
    try:
        assert not sg.mid_graph_applies(_FakeCuda(129, F), graphs[129], f, rho)
    finally:
        sg.MID_GRAPH = old
