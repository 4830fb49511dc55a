"""Host side of the NAM read-out for dense-coded graphs of 129 to 448 nodes (csrc/mid_graph_nam.hip: gnan_mid_graph_nam_*): the entry
points are exported, declared and bound; the records are the small-graph NAM records plus ``colw``; the route query over the WHOLE admitted
domain; what the kernels do not cover is refused before any HIP call with the offending value named; the Python predicate's edges.
No GPU."""
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

SYMBOLS = ("gnan_mid_graph_nam_fwd", "gnan_mid_graph_nam_bwd", "gnan_mid_graph_nam_workspace_bytes", "gnan_mid_graph_nam_describe")
STRUCTS = (("gnan_mid_graph_nam_args", "MidGraphNamArgs"), ("gnan_mid_graph_nam_bwd_args", "MidGraphNamBwdArgs"),
           ("gnan_mid_graph_nam_info", "MidGraphNamInfo"))
LDS_BUDGET = 96 * 1024


def header():
    with open(os.path.join(ROOT, "include", "gnan_hip.h")) as f:
        return f.read()


def test_symbols_are_exported_declared_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS + ("gnan_mid_graph_nam_args", "gnan_mid_graph_nam_bwd_args"):
        assert re.search(r"\b%s\b" % name, text), f"{name} not declared"
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    # the entry points were ADDED (no struct of the ABI changed): the library, the header and the binding agree on the number, still 51
    number = int(re.search(r"^#define GNAN_ABI_VERSION (\d+)$", header(), re.M).group(1))
    assert _lib.lib().gnan_abi_version() == _lib.ABI_VERSION == number == 51


def _fields_of(struct):
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "gnan_small_mlp": _lib.SmallMlp,
               "gnan_small_mlp_grads": _lib.SmallMlpGrads}
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
    return fields


def test_struct_layouts_match_the_header():
    for struct, cls_name in STRUCTS:
        assert _fields_of(struct) == list(getattr(_lib, cls_name)._fields_), struct
    # the small-graph NAM records plus colw: nothing else added, nothing moved
    for mid, one in (("gnan_mid_graph_nam_args", "gnan_small_graph_nam_args"),
                     ("gnan_mid_graph_nam_bwd_args", "gnan_small_graph_nam_bwd_args")):
        assert [(n, t) for n, t in _fields_of(mid) if n != "colw"] == _fields_of(one), mid
        assert ("colw", ctypes.c_void_p) in _fields_of(mid)


def test_the_route_query_over_the_whole_domain():
    """Every n in 1 .. 448 x D x C x F: the tiles, the groups, the three grids, both LDS figures inside the two-per-compute-unit budget,
    and ONE workspace size for both directions — the *_workspace_bytes call's."""
    lib = _lib.lib()
    info = _lib.MidGraphNamInfo()
    for F in (1, 15, 200):
        for n in range(1, 449):
            for D in (2, 17, 64):
                for C in (1, 8):
                    assert lib.gnan_mid_graph_nam_describe(n, F, D, C, info) == 0, (n, F, D, C, lib.gnan_last_error())
                    assert info.row_tiles == -(-n // 64) and info.rho_groups == -(-n // 32), (n, info.as_dict())
                    assert info.fwd_grid == F and info.bwd_feature_grid == F and info.bwd_rho_grid == info.rho_groups
                    assert 0 < info.fwd_lds_bytes <= LDS_BUDGET and 0 < info.bwd_lds_bytes <= LDS_BUDGET, (n, D, C, info.as_dict())
                    need = lib.gnan_mid_graph_nam_workspace_bytes(n, F, D, C)
                    assert info.fwd_workspace_bytes == info.bwd_workspace_bytes == need
                    # counter line | the larger of the forward's parts [F, C] and the backward's float64 partials + d hidden [F]
                    assert need == 16 + max(F * C * 4, -(-n // 32) * 64 * 8 + F * 4)
    assert lib.gnan_mid_graph_nam_describe(200, 15, 12, 1, None) == _lib.ERR_BAD_ARG
    assert lib.gnan_mid_graph_nam_describe(200, 0, 12, 1, info) == _lib.ERR_BAD_ARG
    assert lib.gnan_mid_graph_nam_describe(200, 15, 1, 1, info) == _lib.ERR_UNSUPPORTED and b"D=1" in lib.gnan_last_error()


def _mlp(L=3, H=64, C=1, bias=True, base=0x1000):
    """A gnan_small_mlp of made-up (never dereferenced) addresses."""
    return _lib.SmallMlp(L=L, H=H, C=C, w_first=base, b_first=base + 0x100 if bias else None, w_mid=base + 0x200 if L == 3 else None,
                         b_mid=base + 0x300 if (L == 3 and bias) else None, w_last=base + 0x400, b_last=base + 0x500 if bias else None)


def _grads(m, base=0x9000):
    return _lib.SmallMlpGrads(w_first=base, b_first=base + 0x100 if m.b_first else None, w_mid=base + 0x200 if m.L == 3 else None,
                              b_mid=base + 0x300 if m.b_mid else None, w_last=base + 0x400, b_last=base + 0x500 if m.b_last else None)


def _nam(L=2, H=64, C=3, bias=True, base=0x3000):
    """The read-out's stack; ``L == 1``: a Linear(1, C) per feature, only its last layer exists."""
    if L == 1:
        return _lib.SmallMlp(L=1, H=0, C=C, w_first=None, b_first=None, w_mid=None, b_mid=None, w_last=base + 0x400,
                             b_last=base + 0x500 if bias else None)
    return _mlp(L=L, H=H, C=C, bias=bias, base=base)


def _nam_grads(m, base=0xB000):
    if m.L == 1:
        return _lib.SmallMlpGrads(w_first=None, b_first=None, w_mid=None, b_mid=None, w_last=base + 0x400,
                                  b_last=base + 0x500 if m.b_last else None)
    return _grads(m, base)


def _common(n, F, D, f, rho, nam):
    f = f or _mlp()
    rho = rho or _mlp(bias=False, base=0x2000)
    nam = nam or _nam()
    need = _lib.lib().gnan_mid_graph_nam_workspace_bytes(n, F, D, nam.C)
    return dict(x=0x100000, x_stride=F, n=n, F=F, f=f, rho=rho, nam=nam, code=0x200000, D=D, reserved=0, cnt=0x300000, cnt_stride=D,
                fx=0x400000, lut=0x500000, hidden=0x510000, colw=0x520000, workspace=0x700000, workspace_bytes=need)


def _fwd_args(n=200, F=15, D=12, f=None, rho=None, nam=None, **over):
    kw = _common(n, F, D, f, rho, nam)
    kw["out"] = 0x600000
    kw.update(over)
    return _lib.MidGraphNamArgs(**kw)


def _bwd_args(n=200, F=15, D=12, f=None, rho=None, nam=None, **over):
    kw = _common(n, F, D, f, rho, nam)
    kw.update(d_out=0x600000, df=_grads(kw["f"]), drho=_grads(kw["rho"], 0xA000), dnam=_nam_grads(kw["nam"]))
    kw.update(over)
    return _lib.MidGraphNamBwdArgs(**kw)


def _calls():
    lib = _lib.lib()
    return ((lib.gnan_mid_graph_nam_fwd, _fwd_args), (lib.gnan_mid_graph_nam_bwd, _bwd_args))


UNSUPPORTED = [
    ("n=449", dict(n=449), b"n=449"), ("D=65", dict(D=65, cnt_stride=65), b"D=65"), ("f.C=2", dict(f=_mlp(C=2)), b"f.C=2"),
    ("rho.C=2", dict(rho=_mlp(C=2, bias=False, base=0x2000)), b"rho.C=2"), ("H=65", dict(f=_mlp(H=65)), b"H=65"),
    ("rho H=65", dict(rho=_mlp(H=65, bias=False, base=0x2000)), b"rho.H=65"), ("L=4", dict(f=_mlp(L=4)), b"L=4"),
    ("nam.C=9", dict(nam=_nam(C=9)), b"nam.C=9"), ("nam.L=4", dict(nam=_nam(L=4)), b"nam.L=4"),
    ("nam.H=65", dict(nam=_nam(H=65)), b"nam.H=65")]


@pytest.mark.parametrize("what,kw,named", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_what_lies_outside_the_cover_is_refused_by_name(what, kw, named):
    """A null stream and made-up addresses on a machine without a GPU: every refusal comes from the host-side checks."""
    lib = _lib.lib()
    for call, make in _calls():
        assert call(make(**kw), None) == _lib.ERR_UNSUPPORTED, what
        assert named in lib.gnan_last_error(), (what, lib.gnan_last_error())
    if what in ("n=449", "D=65", "nam.C=9"):
        info = _lib.MidGraphNamInfo()
        shape = (kw.get("n", 200), 15, kw.get("D", 12), kw["nam"].C if "nam" in kw else 3)
        assert lib.gnan_mid_graph_nam_describe(*shape, info) == _lib.ERR_UNSUPPORTED
        assert named in lib.gnan_last_error()


def test_any_number_of_features_passes_the_shape_check():
    """F = 200 (the waiting kernel of the small route stops at 127): accepted as a shape, so the call goes on to the pointers."""
    lib = _lib.lib()
    for call, make in _calls():
        assert call(make(F=200, x_stride=200, x=None), None) == _lib.ERR_BAD_ARG, lib.gnan_last_error()
        assert b"null x" in lib.gnan_last_error()
    info = _lib.MidGraphNamInfo()
    assert lib.gnan_mid_graph_nam_describe(448, 200, 64, 8, info) == 0 and info.fwd_grid == info.bwd_feature_grid == 200


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _lib.lib()
    need = lib.gnan_mid_graph_nam_workspace_bytes(200, 15, 12, 3)
    assert need == 16 + 7 * 64 * 8 + 15 * 4
    null_w = _mlp()
    null_w.w_last = None
    null_nam = _nam(L=1)
    null_nam.w_last = None
    for call, make in _calls():
        assert call(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
        assert call(make(code=None), None) == _lib.ERR_BAD_ARG and b"null code" in lib.gnan_last_error()
        assert call(make(colw=None), None) == _lib.ERR_BAD_ARG and b"null colw" in lib.gnan_last_error()
        for stack in (dict(f=null_w), dict(nam=null_nam)):
            assert call(make(**stack), None) == _lib.ERR_BAD_ARG and b"null weights" in lib.gnan_last_error()
        for field in ("x", "fx", "lut", "hidden"):
            assert call(make(**{field: None}), None) == _lib.ERR_BAD_ARG, field
            assert b"null" in lib.gnan_last_error(), field
        assert call(make(x_stride=14), None) == _lib.ERR_BAD_ARG
        assert b"x_stride=14" in lib.gnan_last_error() and b"F=15" in lib.gnan_last_error()
        assert call(make(cnt_stride=11), None) == _lib.ERR_BAD_ARG
        assert b"cnt_stride=11" in lib.gnan_last_error() and b"D=12" in lib.gnan_last_error()
        assert call(make(code=0x200001), None) == _lib.ERR_BAD_ARG and b"aligned" in lib.gnan_last_error()
        assert call(make(n=0), None) == _lib.ERR_BAD_ARG and b"n=0" in lib.gnan_last_error()
        assert call(make(workspace_bytes=need - 1), None) == _lib.ERR_WORKSPACE
        assert str(need).encode() in lib.gnan_last_error() and str(need - 1).encode() in lib.gnan_last_error()
        assert call(make(workspace=None), None) == _lib.ERR_WORKSPACE
    assert lib.gnan_mid_graph_nam_fwd(_fwd_args(out=None), None) == _lib.ERR_BAD_ARG and b"null out" in lib.gnan_last_error()
    assert lib.gnan_mid_graph_nam_bwd(_bwd_args(d_out=None), None) == _lib.ERR_BAD_ARG and b"null d_out" in lib.gnan_last_error()
    # a bias gradient exactly where there is a bias: one missing, one too many — f, rho and a two-layer read-out
    f, rho, nam = _mlp(), _mlp(bias=False, base=0x2000), _nam(L=2)
    for field, stack, base in (("df", f, 0x9000), ("dnam", nam, 0xB000)):
        missing = _grads(stack, base)
        missing.b_first = None
        assert lib.gnan_mid_graph_nam_bwd(_bwd_args(**{field: missing}), None) == _lib.ERR_BAD_ARG, field
        assert b"bias" in lib.gnan_last_error(), field
    for field, stack, base in (("drho", rho, 0xA000), ("dnam", _nam(L=2, bias=False), 0xB000)):
        extra = _grads(stack, base)
        extra.b_last = base + 0x500
        over = {field: extra}
        if field == "dnam":
            over["nam"] = stack
        assert lib.gnan_mid_graph_nam_bwd(_bwd_args(**over), None) == _lib.ERR_BAD_ARG, field
        assert b"bias" in lib.gnan_last_error(), field
    extra_f = _grads(_mlp(bias=False))
    extra_f.b_first = 0x9100
    assert lib.gnan_mid_graph_nam_bwd(_bwd_args(f=_mlp(bias=False), df=extra_f), None) == _lib.ERR_BAD_ARG
    missing_r = _grads(_mlp(base=0x2000), 0xA000)
    missing_r.b_last = None
    assert lib.gnan_mid_graph_nam_bwd(_bwd_args(rho=_mlp(base=0x2000), drho=missing_r), None) == _lib.ERR_BAD_ARG
    # the one-layer read-out: its last layer's weight gradient, and its bias gradient exactly where there is a bias
    one = _nam(L=1)
    no_grad = _nam_grads(one)
    no_grad.w_last = None
    assert lib.gnan_mid_graph_nam_bwd(_bwd_args(nam=one, dnam=no_grad), None) == _lib.ERR_BAD_ARG
    assert b"one-layer read-out" in lib.gnan_last_error()
    no_bias = _nam_grads(one)
    no_bias.b_last = None
    assert lib.gnan_mid_graph_nam_bwd(_bwd_args(nam=one, dnam=no_bias), None) == _lib.ERR_BAD_ARG
    assert b"one-layer read-out" in lib.gnan_last_error()
    bare = _nam(L=1, bias=False)
    too_many = _nam_grads(bare)
    too_many.b_last = 0xB500
    assert lib.gnan_mid_graph_nam_bwd(_bwd_args(nam=bare, dnam=too_many), None) == _lib.ERR_BAD_ARG
    assert b"one-layer read-out" in lib.gnan_last_error()
    # gnan_small_graph_nam_fwd keeps refusing what is now this route's
    small = _lib.SmallGraphNamArgs(**{k: v for k, v in _common(129, 15, 12, None, None, None).items() if k != "colw"}, out=0x600000)
    assert lib.gnan_small_graph_nam_fwd(small, None) == _lib.ERR_UNSUPPORTED and b"n=129" in lib.gnan_last_error()


class _FakeCuda:
    """What the predicate reads of a device tensor, on a machine without a device."""
    is_cuda, dtype, requires_grad = True, torch.float32, False

    def __init__(self, n, F, requires_grad=False):
        self.shape, self.requires_grad = (n, F), requires_grad


def test_the_predicate(monkeypatch):
    F = 5
    t = lambda *s: torch.zeros(*s)        # noqa: E731
    f = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 1, 8), t(F, 1), 3, 8, 1, F)
    f2 = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 2, 8), t(F, 2), 3, 8, 2, F)
    rho = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 1, 8), None, 3, 8, 1, 1)
    rho2 = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 2, 8), None, 3, 8, 2, 1)
    nam = StackedMLP(t(F, 8), t(F, 8), None, None, t(F, 3, 8), t(F, 3), 2, 8, 3, F)
    nam_other = StackedMLP(t(F + 1, 8), t(F + 1, 8), None, None, t(F + 1, 3, 8), t(F + 1, 3), 2, 8, 3, F + 1)
    nam4 = StackedMLP(t(F, 8), t(F, 8), t(2, F, 8, 8), t(2, F, 8), t(F, 3, 8), t(F, 3), 4, 8, 3, F)
    monkeypatch.setattr(sg, "MID_GRAPH_NAM", True)

    def dense(n, n_codes=2):             # (what the predicate reads of a dense-coded graph: building one takes a device)
        return types.SimpleNamespace(is_dense=True, n_rows=n, n_cols=n, n_codes=n_codes, cnt=torch.ones(n, n_codes, dtype=torch.int32))
    ok = sg.mid_graph_nam_applies
    assert not ok(_FakeCuda(128, F), dense(128), f, rho, nam)
    assert ok(_FakeCuda(129, F), dense(129), f, rho, nam)
    assert ok(_FakeCuda(448, F), dense(448), f, rho, nam)
    assert not ok(_FakeCuda(449, F), dense(449), f, rho, nam)
    assert not ok(_FakeCuda(129, F, requires_grad=True), dense(129), f, rho, nam)
    n = 129
    csr = HopGraph.from_csr(torch.arange(n + 1), torch.arange(n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8), n_cols=n,
                            n_codes=2)
    assert not ok(_FakeCuda(n, F), csr, f, rho, nam)
    assert ok(_FakeCuda(129, F), dense(129, 64), f, rho, nam) and not ok(_FakeCuda(129, F), dense(129, 65), f, rho, nam)
    assert not ok(_FakeCuda(129, F), dense(129), f2, rho, nam)                    # f.C = 2
    assert not ok(_FakeCuda(129, F), dense(129), f, rho2, nam)                    # rho.C = 2
    assert not ok(_FakeCuda(129, F), dense(129), f, rho, nam_other)               # nam.F != f.F
    assert not ok(_FakeCuda(129, F), dense(129), f, rho, nam4)                    # nam.L = 4
    assert not ok(torch.zeros(129, F), dense(129), f, rho, nam)                   # CPU tensors
    # shell normalisation without shell sizes does not apply; without normalisation the sizes are not needed
    bare = dense(129)
    bare.cnt = None
    assert not ok(_FakeCuda(129, F), bare, f, rho, nam) and ok(_FakeCuda(129, F), bare, f, rho, nam, False)
    monkeypatch.setattr(sg, "MID_GRAPH_NAM", False)                               # the switch is read at every call
    assert not ok(_FakeCuda(129, F), dense(129), f, rho, nam)
    monkeypatch.setattr(sg, "MID_GRAPH_NAM", True)
    assert ok(_FakeCuda(129, F), dense(129), f, rho, nam)
    # the small route's predicate keeps its cover
    assert sg.small_graph_nam_applies(_FakeCuda(128, F), dense(128), f, rho, nam)
    assert not sg.small_graph_nam_applies(_FakeCuda(129, F), dense(129), f, rho, nam)
