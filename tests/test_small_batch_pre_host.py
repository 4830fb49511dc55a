"""Host side of pre-rho normalisation on the batched / slot kernels (csrc/small_graph.hip: gnan_small_batch_pre_*): the entry points
are exported, declared and bound; the route query over the whole admitted domain; what the kernels do not cover is refused before
any HIP call, with the code and the offending value; ``small_graph.slot_mode`` behind ``SLOT_PRE_RHO``.  No GPU."""
import ctypes
import re

import pytest
import torch

from gnan_amd import _lib
from gnan_amd import small_graph as sg
from test_mid_graph_host import _FakeCuda, _grads, _mlp, header

SYMBOLS = ("gnan_small_batch_pre_fwd", "gnan_small_batch_pre_bwd", "gnan_small_batch_pre_fwd_drop_dev",
           "gnan_small_batch_pre_bwd_drop_dev", "gnan_small_batch_pre_workspace_bytes", "gnan_small_batch_pre_bwd_workspace_bytes",
           "gnan_small_batch_pre_describe")
LDS_PER_CU = 160 * 1024
RHO_GROUPS_MAX, RHO_SLOT = 12, 64 * 64 + 5 * 64          # csrc/small_graph.hip, csrc/small_graph_body.hpp


def test_symbols_are_exported_declared_and_bound():
    handle = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert len(SYMBOLS) == 7
    for name in SYMBOLS:
        assert hasattr(handle, name), f"{name} not exported"
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} not declared"
        assert name in _lib.SYMBOLS, f"{name} not bound"
        assert getattr(_lib.lib(), name).argtypes == _lib.SYMBOLS[name][1]
    # entry points were ADDED (no struct of the ABI changed): the number did not move
    number = int(re.search(r"^#define GNAN_ABI_VERSION (\d+)$", header(), re.M).group(1))
    assert _lib.lib().gnan_abi_version() == _lib.ABI_VERSION == number == 51


def test_the_info_struct_matches_the_header():
    c_types = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64}
    body = re.search(r"typedef struct gnan_small_batch_pre_info \{(.*?)\} gnan_small_batch_pre_info;", header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(d.split()[1], c_types[d.split()[0]]) for d in (s.strip() for s in body.split(";")) if d]
    assert fields == list(_lib.SmallBatchPreInfo._fields_)


def _fwd_args(sizes=(30, 64, 5), F=15, D=12, f=None, rho=None, **over):
    f = f or _mlp()
    rho = rho or _mlp(bias=False, base=0x2000)
    G, N = len(sizes), sum(sizes)
    need = _lib.lib().gnan_small_batch_pre_workspace_bytes(G, N, F, f.C)
    kw = dict(x=0x100000, x_stride=F, total_nodes=N, F=F, n_graphs=G, max_nodes=max(sizes), f=f, rho=rho, code=0x200000,
              node_off=0x210000, code_off=0x220000, D=D, rho_raw_hops=0, rest_zero=0, S=0x400000, lut=0x500000, Y=None, Ysum=0x600000,
              workspace=0x700000, workspace_bytes=need, cnt=0x300000, cnt_stride=D)
    kw.update(over)
    return _lib.SmallBatchArgs(**kw)


def _bwd_args(sizes=(30, 64, 5), F=15, D=12, f=None, rho=None, **over):
    f = f or _mlp()
    rho = rho or _mlp(bias=False, base=0x2000)
    G, N = len(sizes), sum(sizes)
    kw = dict(x=0x100000, x_stride=F, total_nodes=N, F=F, n_graphs=G, max_nodes=max(sizes), f=f, rho=rho, code=0x200000,
              node_off=0x210000, code_off=0x220000, D=D, rho_raw_hops=0, rest_zero=0, S=0x400000, lut=0x500000, dY=None,
              dYsum=0x600000, df=_grads(f), drho=_grads(rho, 0xA000), workspace=0x700000, workspace_bytes=0, cnt=0x300000, cnt_stride=D)
    kw.update(over)
    a = _lib.SmallBatchBwdArgs(**kw)
    if "workspace_bytes" not in over:
        a.workspace_bytes = _lib.lib().gnan_small_batch_pre_bwd_workspace_bytes(a)
    return a


def test_the_route_query_over_the_whole_domain():
    """Every max_nodes 1 .. 128 x D x C: the grids, both launches inside one compute unit's LDS, and the workspace formulas the
    query reports are the ones the two byte queries return."""
    lib = _lib.lib()
    info = _lib.SmallBatchPreInfo()
    F, G = 15, 3
    for n in range(1, 129):
        for D in (1, 2, 16, 63, 64):
            for C in range(1, 9):
                assert lib.gnan_small_batch_pre_describe(n, F, D, C, info) == 0, (n, D, C, lib.gnan_last_error())
                assert info.node_blocks == (1 if n <= 64 else 2)
                assert info.rho_workgroups == -(-n * D // 64) and info.fwd_grid == F + -(-n * D // 64), (n, D, info.as_dict())
                assert info.rho_groups == min(D, 12) and info.bwd_grid == F + min(D, 12), (n, D, info.as_dict())
                assert 0 < info.fwd_lds_bytes <= LDS_PER_CU and 0 < info.bwd_lds_bytes <= LDS_PER_CU, (n, D, C, info.as_dict())
                if D in (1, 64) and n in (1, 64, 65, 128):
                    N = G * n - 2 if n > 1 else G
                    assert lib.gnan_small_batch_pre_workspace_bytes(G, N, F, C) == G * info.fwd_graph_bytes + N * info.fwd_node_bytes
                    f = _mlp(C=C)
                    a = _bwd_args(sizes=(n,) * G, F=F, D=D, f=f)
                    slabs = lib.gnan_small_batch_bwd_workspace_bytes(a)              # the slabs of gnan_small_batch_bwd
                    assert slabs % G == 0
                    assert a.workspace_bytes == -(-slabs // 128) * 128 + G * info.bwd_graph_bytes, (n, D, C)
    assert info.fwd_graph_bytes == 128 and info.bwd_graph_bytes == 128 + RHO_GROUPS_MAX * RHO_SLOT * 4
    for bad, named in (((129, F, 2, 1), b"n=129"), ((64, F, 65, 1), b"D=65"), ((64, F, 2, 9), b"C=9")):
        assert lib.gnan_small_batch_pre_describe(*bad, info) == _lib.ERR_UNSUPPORTED and named in lib.gnan_last_error()
    assert lib.gnan_small_batch_pre_describe(64, F, 2, 1, None) == _lib.ERR_BAD_ARG


UNSUPPORTED = [
    ("cnt", dict(cnt=None, cnt_stride=0), b"cnt="), ("rho.C", dict(rho=_mlp(C=2, bias=False, base=0x2000)), b"rho.C=2"),
    ("D", dict(D=65, cnt_stride=65), b"D=65"), ("rho_raw_hops", dict(rho_raw_hops=1), b"rho_raw_hops=1"),
    ("rest_zero", dict(rest_zero=1), b"rest_zero=1"), ("max_nodes", dict(max_nodes=129), b"n=129"),
    ("n_graphs", dict(n_graphs=65536), b"n_graphs=65536"), ("H", dict(f=_mlp(H=65)), b"H=65"), ("L", dict(f=_mlp(L=4)), b"L=4"),
    ("C", dict(f=_mlp(C=9)), b"C=9")]


@pytest.mark.parametrize("what,kw,named", UNSUPPORTED, ids=[u[0] for u in UNSUPPORTED])
def test_what_lies_outside_the_cover_is_refused_by_name(what, kw, named):
    """A null stream and made-up addresses on a machine without a GPU: every refusal comes from the host-side checks."""
    lib = _lib.lib()
    cell = _lib.SmallDropoutDev(p=0.5, reserved=0, seed=0x800000)
    for call, args in ((lib.gnan_small_batch_pre_fwd, _fwd_args(**kw)), (lib.gnan_small_batch_pre_bwd, _bwd_args(**kw))):
        assert call(args, None) == _lib.ERR_UNSUPPORTED, what
        assert named in lib.gnan_last_error(), (what, lib.gnan_last_error())
    for call, args in ((lib.gnan_small_batch_pre_fwd_drop_dev, _fwd_args(**kw)), (lib.gnan_small_batch_pre_bwd_drop_dev, _bwd_args(**kw))):
        assert call(args, cell, None) == _lib.ERR_UNSUPPORTED, what
        assert named in lib.gnan_last_error(), (what, lib.gnan_last_error())


def test_bad_arguments_are_refused_before_any_hip_call():
    lib = _lib.lib()
    need = lib.gnan_small_batch_pre_workspace_bytes(3, 99, 15, 1)
    assert need == 3 * 128 + 99 * 15 * 4 == lib.gnan_small_batch_workspace_bytes(3, 99, 15, 1)
    assert lib.gnan_small_batch_pre_fwd(_fwd_args(workspace_bytes=need - 1), None) == _lib.ERR_WORKSPACE
    assert str(need).encode() in lib.gnan_last_error() and str(need - 1).encode() in lib.gnan_last_error()
    full = _bwd_args()
    assert lib.gnan_small_batch_pre_bwd(_bwd_args(workspace_bytes=full.workspace_bytes - 1), None) == _lib.ERR_WORKSPACE
    assert str(full.workspace_bytes).encode() in lib.gnan_last_error()
    assert lib.gnan_small_batch_pre_bwd(_bwd_args(workspace=None), None) == _lib.ERR_WORKSPACE
    assert lib.gnan_small_batch_pre_bwd(_bwd_args(workspace=0x700004), None) == _lib.ERR_BAD_ARG and b"aligned" in lib.gnan_last_error()
    assert lib.gnan_small_batch_pre_bwd_workspace_bytes(None) == 0
    null_w = _mlp()
    null_w.w_last = None
    for call, make in ((lib.gnan_small_batch_pre_fwd, _fwd_args), (lib.gnan_small_batch_pre_bwd, _bwd_args)):
        assert call(None, None) == _lib.ERR_BAD_ARG
        assert call(make(f=null_w), None) == _lib.ERR_BAD_ARG and b"null weights" in lib.gnan_last_error()
        for field in ("x", "code", "node_off", "code_off", "S", "lut"):
            assert call(make(**{field: None}), None) == _lib.ERR_BAD_ARG, field
            assert b"null" in lib.gnan_last_error(), field
        assert call(make(x_stride=14), None) == _lib.ERR_BAD_ARG
        assert b"x_stride=14" in lib.gnan_last_error() and b"F=15" in lib.gnan_last_error()
        assert call(make(cnt_stride=11), None) == _lib.ERR_BAD_ARG and b"cnt_stride=11" in lib.gnan_last_error()
        assert call(make(F=0), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_small_batch_pre_fwd(_fwd_args(Ysum=None), None) == _lib.ERR_BAD_ARG
    assert lib.gnan_small_batch_pre_bwd(_bwd_args(dYsum=None), None) == _lib.ERR_BAD_ARG
    f = _mlp()
    missing = _grads(f)
    missing.b_first = None
    assert lib.gnan_small_batch_pre_bwd(_bwd_args(df=missing), None) == _lib.ERR_BAD_ARG and b"bias" in lib.gnan_last_error()


def test_the_dropout_records_refusal_order():
    """A NULL record, p outside [0, 1) (NaN included), reserved != 0, a NULL cell — in this order, each before anything of the call
    itself (an unsupported shape comes after them); p == 0 goes on to the plain launcher's checks."""
    lib = _lib.lib()
    rec = lambda **kw: _lib.SmallDropoutDev(**{**dict(p=0.5, reserved=0, seed=0x800000), **kw})          # noqa: E731
    bad_shape = dict(D=65, cnt_stride=65)
    for call, make in ((lib.gnan_small_batch_pre_fwd_drop_dev, _fwd_args), (lib.gnan_small_batch_pre_bwd_drop_dev, _bwd_args)):
        assert call(None, rec(), None) == _lib.ERR_BAD_ARG and b"null args" in lib.gnan_last_error()
        assert call(make(**bad_shape), None, None) == _lib.ERR_BAD_ARG and b"null dropout record" in lib.gnan_last_error()
        for p in (-0.1, 1.0, float("nan")):
            assert call(make(**bad_shape), rec(p=p, reserved=3, seed=None), None) == _lib.ERR_BAD_ARG
            assert b"dropout p" in lib.gnan_last_error()
        assert call(make(**bad_shape), rec(reserved=3, seed=None), None) == _lib.ERR_BAD_ARG and b"reserved=3" in lib.gnan_last_error()
        assert call(make(**bad_shape), rec(seed=None), None) == _lib.ERR_BAD_ARG and b"seed cell" in lib.gnan_last_error()
        assert call(make(**bad_shape), rec(), None) == _lib.ERR_UNSUPPORTED and b"D=65" in lib.gnan_last_error()
        assert call(make(**bad_shape), rec(p=0.0), None) == _lib.ERR_UNSUPPORTED and b"D=65" in lib.gnan_last_error()


def _standalone(**kw):
    from gnan_amd import GNAN as standalone
    torch.manual_seed(0)
    return standalone.TensorGNAN(15, kw.pop("out_channels", 1), 3, hidden_channels=32, is_graph_task=kw.pop("is_graph_task", True), **kw)


def test_slot_mode_behind_the_switch(monkeypatch):
    from gnan_amd import models
    m = _standalone()
    assert m.normalize_rho is True                                    # the class's default
    monkeypatch.setattr(sg, "SLOT_PRE_RHO", False)
    assert sg.slot_mode(m) is None
    monkeypatch.setattr(sg, "SLOT_PRE_RHO", True)
    assert sg.slot_mode(m) == "pre"                                   # (the answer with the switch off was not frozen)
    monkeypatch.setattr(sg, "SLOT_PRE_RHO", False)
    assert sg.slot_mode(m) is None                                    # ... nor is the one with it on
    monkeypatch.setattr(sg, "SLOT_PRE_RHO", True)
    with monkeypatch.context() as mp:                                 # a pre-rho forward has no general backward
        mp.setattr(sg, "SMALL_GRAPH_BACKWARD", False)
        assert sg.slot_mode(m) is None
    assert sg.slot_mode(_standalone(is_graph_task=False)) is None
    assert sg.slot_mode(_standalone(out_channels=3)) is None          # rho has out_channels outputs: not one channel
    for on in (False, True):                                          # unchanged whatever the switch says
        monkeypatch.setattr(sg, "SLOT_PRE_RHO", on)
        assert sg.slot_mode(_standalone(normalize_rho=False)) is False
        assert sg.slot_mode(_standalone(normalize_rho=False, out_channels=3)) is None
        assert sg.slot_mode(models.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=True, readout_n_layers=0)) is True
        assert sg.slot_mode(models.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=True, readout_n_layers=0,
                                              normalize_rho=False)) is False
        assert sg.slot_mode(models.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=True, readout_n_layers=2)) is None
        assert sg.slot_mode(models.TensorGNAN(15, 1, 3, hidden_channels=32, is_graph_task=False, readout_n_layers=0)) is None


def test_the_slots_predicate_is_the_stacks_side_only():
    """``slot_graph_applies`` asks a one-channel rho whatever the normalisation: what ``slot_mode`` builds on."""
    import types
    from gnan_amd.functional import StackedMLP
    F = 5
    t = lambda *s: torch.zeros(*s)        # noqa: E731
    f = StackedMLP(t(F, 8), t(F, 8), t(1, F, 8, 8), t(1, F, 8), t(F, 1, 8), t(F, 1), 3, 8, 1, F)
    rho = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 1, 8), None, 3, 8, 1, 1)
    rho2 = StackedMLP(t(1, 8), None, t(1, 1, 8, 8), None, t(1, 2, 8), None, 3, 8, 2, 1)
    slot = types.SimpleNamespace(F=F)
    assert sg.slot_graph_applies(slot, f, rho) and not sg.slot_graph_applies(slot, f, rho2)
    assert _FakeCuda(4, F).is_cuda and sg.SLOT_MAX_NODES == 128 and sg.SLOT_CODES == 64
