"""Host side of the NAM read-out on graph slots (csrc/small_graph_nam.hip: gnan_small_slot_nam_*): the entry points are exported,
declared and bound; the structs are the header's; the route query over the whole admitted domain; what the kernels do not cover is
refused before any HIP call, with the code and the offending value; ``small_graph.slot_mode`` behind ``SLOT_NAM_READOUT``.  No GPU."""
import ctypes
import re

import pytest

from gnan_amd import _lib
from gnan_amd import small_graph as sg
from test_mid_graph_host import _grads, _mlp, header

SYMBOLS = ("gnan_small_slot_nam_fwd", "gnan_small_slot_nam_bwd", "gnan_small_slot_nam_workspace_bytes", "gnan_small_slot_nam_describe")
STRUCTS = (("gnan_small_slot_nam_args", "SmallSlotNamArgs"), ("gnan_small_slot_nam_bwd_args", "SmallSlotNamBwdArgs"),
           ("gnan_small_slot_nam_info", "SmallSlotNamInfo"))
LDS_PER_CU = 160 * 1024


def test_symbols_are_exported_declared_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    # entry points were ADDED (no struct of the ABI changed): the number did not move
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
    # the one-graph records with n replaced by max_nodes, and node_off / fx_stride added: nothing else moved
    for slot, one in (("gnan_small_slot_nam_args", "gnan_small_graph_nam_args"),
                      ("gnan_small_slot_nam_bwd_args", "gnan_small_graph_nam_bwd_args")):
        kept = [(("n" if n == "max_nodes" else n), t) for n, t in _fields_of(slot) if n not in ("node_off", "fx_stride")]
        assert kept == _fields_of(one), slot


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


def _common(max_nodes, F, D, f, rho, nam, over):
    f = f or _mlp()
    rho = rho or _mlp(bias=False, base=0x2000)
    nam = nam or _nam()
    need = _lib.lib().gnan_small_slot_nam_workspace_bytes(F, nam.C)
    kw = dict(x=0x100000, x_stride=F, max_nodes=max_nodes, F=F, f=f, rho=rho, nam=nam, code=0x200000, D=D, reserved=0, cnt=0x300000,
              cnt_stride=D, node_off=0x210000, fx=0x400000, fx_stride=max_nodes, lut=0x500000, hidden=0x510000, workspace=0x700000,
              workspace_bytes=need)
    kw.update(over)
    return kw


def _fwd_args(max_nodes=64, F=15, D=16, f=None, rho=None, nam=None, **over):
    kw = _common(max_nodes, F, D, f, rho, nam, {})
    kw["out"] = 0x600000
    kw.update(over)
    return _lib.SmallSlotNamArgs(**kw)


def _bwd_args(max_nodes=64, F=15, D=16, f=None, rho=None, nam=None, **over):
    kw = _common(max_nodes, F, D, f, rho, nam, {})
    kw.update(d_out=0x600000, df=_grads(kw["f"]), drho=_grads(kw["rho"], 0xA000), dnam=_nam_grads(kw["nam"]))
    kw.update(over)
    return _lib.SmallSlotNamBwdArgs(**kw)


def _calls():
    lib = _lib.lib()
    return ((lib.gnan_small_slot_nam_fwd, _fwd_args), (lib.gnan_small_slot_nam_bwd, _bwd_args))


UNSUPPORTED = [
    ("max_nodes=100", dict(max_nodes=100), b"max_nodes=100"), ("max_nodes=129", dict(max_nodes=129), b"max_nodes=129"),
    ("max_nodes=32", dict(max_nodes=32), b"max_nodes=32"), ("D", dict(D=65, cnt_stride=65), b"D=65"),
    ("D=1", dict(D=1), b"D=1"), ("f.C", dict(f=_mlp(C=2)), b"C=2"), ("rho.C", dict(rho=_mlp(C=2, bias=False, base=0x2000)), b"rho.C=2"),
    ("nam.L", dict(nam=_nam(L=4)), b"L=4"), ("nam.C", dict(nam=_nam(C=9)), b"C=9"), ("f.H", dict(f=_mlp(H=65)), b"H=65"),
    ("rho.H", dict(rho=_mlp(H=65, bias=False, base=0x2000)), b"H=65"), ("nam.H", dict(nam=_nam(H=65)), b"H=65"),
    ("f.L", dict(f=_mlp(L=4)), b"L=4")]


@pytest.mark.parametrize("what,kw,named", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_what_lies_outside_the_cover_is_refused_by_name(what, kw, named):
    """A null stream and made-up addresses on a machine without a GPU: every refusal comes from the host-side checks."""
    lib = _lib.lib()
    for call, make in _calls():
        assert call(make(**kw), None) == _lib.ERR_UNSUPPORTED, what
        assert named in lib.gnan_last_error(), (what, lib.gnan_last_error())
    assert b"{64, 128}" in lib.gnan_last_error() or not what.startswith("max_nodes")      # the limit is named with the value


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _lib.lib()
    need = lib.gnan_small_slot_nam_workspace_bytes(15, 3)
    assert need == 16 + 15 * 3 * 4 == lib.gnan_small_graph_nam_workspace_bytes(15, 3)
    assert lib.gnan_small_slot_nam_workspace_bytes(70, 1) == 16 + 70 * 4
    null_w = _mlp()
    null_w.w_last = None
    null_nam = _nam(L=1)
    null_nam.w_last = None
    for call, make in _calls():
        assert call(None, None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
        assert call(make(node_off=None), None) == _lib.ERR_BAD_ARG and b"null node_off" in lib.gnan_last_error()
        for stack in (dict(f=null_w), dict(nam=null_nam)):
            assert call(make(**stack), None) == _lib.ERR_BAD_ARG and b"null weights" in lib.gnan_last_error()
        for field in ("x", "code", "fx", "lut", "hidden"):
            assert call(make(**{field: None}), None) == _lib.ERR_BAD_ARG, field
            assert b"null" in lib.gnan_last_error(), field
        assert call(make(workspace_bytes=need - 1), None) == _lib.ERR_WORKSPACE
        assert str(need).encode() in lib.gnan_last_error() and str(need - 1).encode() in lib.gnan_last_error()
        assert call(make(workspace=None), None) == _lib.ERR_WORKSPACE
        assert call(make(x_stride=14), None) == _lib.ERR_BAD_ARG
        assert b"x_stride=14" in lib.gnan_last_error() and b"F=15" in lib.gnan_last_error()
        assert call(make(cnt_stride=15), None) == _lib.ERR_BAD_ARG and b"cnt_stride=15" in lib.gnan_last_error()
        assert call(make(fx_stride=63), None) == _lib.ERR_BAD_ARG
        assert b"fx_stride=63" in lib.gnan_last_error() and b"max_nodes=64" in lib.gnan_last_error()
        assert call(make(code=0x200002), None) == _lib.ERR_BAD_ARG and b"aligned" in lib.gnan_last_error()
        assert call(make(F=0), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_small_slot_nam_fwd(_fwd_args(out=None), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_small_slot_nam_bwd(_bwd_args(d_out=None), None) == _lib.ERR_BAD_ARG
    missing = _grads(_mlp())
    missing.b_first = None
    assert lib.gnan_small_slot_nam_bwd(_bwd_args(df=missing), None) == _lib.ERR_BAD_ARG and b"bias" in lib.gnan_last_error()
    one = _nam(L=1)
    no_grad = _nam_grads(one)
    no_grad.w_last = None
    assert lib.gnan_small_slot_nam_bwd(_bwd_args(nam=one, dnam=no_grad), None) == _lib.ERR_BAD_ARG
    assert b"one-layer read-out" in lib.gnan_last_error()


def test_the_route_query_over_the_whole_domain():
    """Both capacities x F x every D x every C: F workgroups either way (no workgroup of rho's own, no limit on F), both launches
    inside one compute unit's LDS, and the workspace shares are the ones the byte query takes the larger of."""
    lib = _lib.lib()
    info = _lib.SmallSlotNamInfo()
    for cap in (64, 128):
        for F in (1, 15, 127, 200):
            for D in range(2, 65):
                for C in range(1, 9):
                    assert lib.gnan_small_slot_nam_describe(cap, F, D, C, info) == 0, (cap, F, D, C, lib.gnan_last_error())
                    assert info.fwd_grid == F and info.bwd_grid == F, info.as_dict()
                    assert 0 < info.fwd_lds_bytes <= LDS_PER_CU and 0 < info.bwd_lds_bytes <= LDS_PER_CU, info.as_dict()
                    assert info.fwd_workspace_bytes == 16 + F * C * 4 and info.bwd_workspace_bytes == 16 + F * 4
                    assert lib.gnan_small_slot_nam_workspace_bytes(F, C) == max(info.fwd_workspace_bytes, info.bwd_workspace_bytes)
    assert max(info.fwd_lds_bytes, info.bwd_lds_bytes) <= LDS_PER_CU // 2          # two workgroups per compute unit
    for bad, named in (((100, 15, 16, 1), b"max_nodes=100"), ((64, 15, 65, 1), b"D=65"), ((64, 15, 16, 9), b"C=9"), ((64, 15, 1, 1), b"D=1")):
        assert lib.gnan_small_slot_nam_describe(*bad, info) == _lib.ERR_UNSUPPORTED and named in lib.gnan_last_error(), bad
    assert lib.gnan_small_slot_nam_describe(64, 15, 16, 1, None) == _lib.ERR_BAD_ARG
    assert lib.gnan_small_slot_nam_describe(64, 0, 16, 1, info) == _lib.ERR_BAD_ARG


def _readout_model(**kw):
    import torch
    from gnan_amd import models
    torch.manual_seed(0)
    return models.TensorGNAN(15, kw.pop("out_channels", 3), 3, hidden_channels=kw.pop("hidden_channels", 32), is_graph_task=True,
                             readout_n_layers=kw.pop("readout_n_layers", 1), **kw)


def test_slot_mode_behind_the_switch(monkeypatch):
    m = _readout_model()
    assert m.readout_n_layers == 1 and m.aggregation_order == "sum_first"
    monkeypatch.setattr(sg, "SLOT_NAM_READOUT", False)
    assert sg.slot_mode(m) is None
    monkeypatch.setattr(sg, "SLOT_NAM_READOUT", True)
    mode = sg.slot_mode(m)
    assert isinstance(mode, sg.SlotNamMode) and mode.use_cnt is True and bool(mode) is True          # (the answer off was not frozen)
    assert mode != "pre" and mode is not True and mode == sg.SlotNamMode(True) != sg.SlotNamMode(False)
    monkeypatch.setattr(sg, "SLOT_NAM_READOUT", False)
    assert sg.slot_mode(m) is None                                    # ... nor is the one with it on
    monkeypatch.setattr(sg, "SLOT_NAM_READOUT", True)
    with monkeypatch.context() as mp:                                 # the route's backward is the one launch or nothing
        mp.setattr(sg, "SMALL_GRAPH_BACKWARD", False)
        assert sg.slot_mode(m) is None
    plain = sg.slot_mode(_readout_model(normalize_rho=False))
    assert isinstance(plain, sg.SlotNamMode) and plain.use_cnt is False and not plain and plain is not None      # no cnt laid out
    for layers in (2, 3):
        assert isinstance(sg.slot_mode(_readout_model(readout_n_layers=layers)), sg.SlotNamMode)
    # the order: asked at every call
    m.aggregation_order = "reference"
    assert sg.slot_mode(m) is None
    m.aggregation_order = "sum_first"
    assert isinstance(sg.slot_mode(m), sg.SlotNamMode)
    # outside the cover: a hidden width of 65, nine read-out channels, a four-layer read-out
    assert sg.slot_mode(_readout_model(hidden_channels=65)) is None
    assert sg.slot_mode(_readout_model(out_channels=9)) is None
    assert sg.slot_mode(_readout_model(readout_n_layers=4)) is None
    # the other classes' answers do not depend on this switch
    from gnan_amd import models
    for on in (False, True):
        monkeypatch.setattr(sg, "SLOT_NAM_READOUT", on)
        assert sg.slot_mode(models.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=True, readout_n_layers=0)) is True
        assert sg.slot_mode(models.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=False, readout_n_layers=1)) is None


def test_the_mode_lays_out_cnt_by_its_truth():
    """``SlotGraph(use_cnt=mode)`` and the harness read a mode's truth: shell sizes exactly under ``normalize_rho``."""
    import types
    assert bool(sg.SlotNamMode(True)) and not bool(sg.SlotNamMode(False))
    assert len({sg.SlotNamMode(True), sg.SlotNamMode(True), sg.SlotNamMode(False)}) == 2
    assert "use_cnt=True" in repr(sg.SlotNamMode(True))
    import torch
    from gnan_amd.functional import StackedMLP
    F = 5
    t = lambda *s: torch.zeros(*s)        # noqa: E731
    f = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 1, 8), t(F, 1), 3, 8, 1, F)
    f2 = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 2, 8), t(F, 2), 3, 8, 2, F)
    rho = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 1, 8), None, 3, 8, 1, 1)
    nam1 = StackedMLP(None, None, None, None, t(F, 3), t(F, 3), 1, 0, 3, F)
    nam200 = StackedMLP(None, None, None, None, t(200, 3), t(200, 3), 1, 0, 3, 200)
    slot = types.SimpleNamespace(F=F)
    assert sg.slot_nam_applies(slot, f, rho, nam1) and not sg.slot_nam_applies(slot, f2, rho, nam1)
    assert not sg.slot_nam_applies(slot, f, rho, nam200)              # the read-out's features are the slots'
