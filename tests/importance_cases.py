"""``interpret.importance`` checked on one device — TEST INFRASTRUCTURE shared by tests/test_gpu_importance.py (the HIP path,
``gnan_attr_reduce``) and tests/test_importance_cpu.py (``cpu_route.reduced_attributions``).  The module classes, graphs and inputs
are those of tests/test_gpu_explain.py; the moments are formed here in float64 from (a) the dense float64 restatement of
tests/attr_ref.py, which forms no hop code, and (b) ``interpret.explain`` on the same device."""
import numpy as np
import torch

import attr_ref
from helpers import TWO_FLOORS, assert_rule
from test_gpu_explain import F_RAW, MODULES, build, forward, graph_case, inputs_on

from gnan_amd import interpret


def moments_of(terms, labels):
    """``terms [R, F, D, C]`` float64, ``labels [R]``: ``(group_labels, count, mean, mean_abs, rms, f_mean, f_mean_abs, f_rms)`` with
    the groups in ascending label order."""
    terms = terms.detach().cpu().double()
    labels = torch.as_tensor(labels).long().cpu()
    uniq = torch.unique(labels)
    out = [[] for _ in range(6)]
    count = []
    for lab in uniq.tolist():
        a = terms[labels == lab]
        t = a.sum(2)
        count.append(a.shape[0])
        for slot, v in zip(out, (a.mean(0), a.abs().mean(0), (a * a).mean(0).sqrt(), t.mean(0), t.abs().mean(0), (t * t).mean(0).sqrt())):
            slot.append(v)
    return (uniq, torch.tensor(count, dtype=torch.float64)) + tuple(torch.stack(s) for s in out)


FIELDS = ("mean", "mean_abs", "rms", "feature_mean", "feature_mean_abs", "feature_rms")


def assert_fields(imp, want, what, floor):
    labels, count = want[:2]
    assert imp.group_labels.cpu().tolist() == labels.tolist(), what
    assert imp.count.dtype == torch.float64 and imp.count.cpu().tolist() == count.tolist(), what
    for name, w in zip(FIELDS, want[2:]):
        got = getattr(imp, name)
        assert got.dtype == torch.float64 and tuple(got.shape) == tuple(w.shape), (what, name)
        assert_rule(got, w, what=f"{what}: {name}", floor=floor)


def check_module(name, which, dev, same_device_floor):
    """Every field of ``importance`` for module ``name`` on graph ``which``, grouped by a three-valued label, against the restatement
    and against ``explain`` on ``dev``; the two identities; the ungrouped call."""
    _, kind, node_ids = MODULES[name]
    x, nd, norm, csr, D = graph_case(which)
    m = build(name, dev)
    data = inputs_on(which, dev)
    R = x.shape[0] if node_ids is None else len(node_ids)
    labels = (torch.arange(R) * 7 % 3) * 2 + 1                        # classes 1, 3, 5, interleaved: the front sorts the rows
    imp = interpret.importance(m, data, node_ids=node_ids, groups=labels)
    ids = torch.arange(R) if node_ids is None else torch.tensor(node_ids)
    order = torch.sort(labels, stable=True).indices
    assert imp.rows.cpu().tolist() == ids[order].tolist()
    C = imp.mean.shape[-1]
    assert tuple(imp.mean.shape) == (3 if R >= 3 else R, F_RAW + 1, D, C) and imp.mean.device.type == torch.device(dev).type
    assert imp.hops.dtype == torch.float64 and imp.hops.cpu().tolist() == [float(d) for d in range(D - 1)] + [float("inf")]
    params = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    truth = attr_ref.explain_restatement(kind, x, nd, norm, params, bool(m.normalize_rho), D, node_ids)
    assert_fields(imp, moments_of(truth, labels), f"{name}/{which} against the restatement", 1e-5)
    ex = interpret.explain(m, data, node_ids=node_ids)
    assert_fields(imp, moments_of(ex.by_feature_distance, labels), f"{name}/{which} against explain", same_device_floor)
    # mean * count over (feature, distance) is the sum of the outputs of the group's rows
    total = (imp.mean * imp.count.view(-1, 1, 1, 1)).sum(dim=(1, 2)).cpu()
    out = ex.by_feature_distance.double().sum(dim=(1, 2)).cpu()      # explain's output, its float32 terms added in float64
    want = torch.stack([out[labels == lab].sum(0) for lab in imp.group_labels.cpu().tolist()])
    assert_rule(total, want, what=f"{name}/{which}: mean * count against explain's outputs", floor=same_device_floor)
    if not getattr(m, "is_graph_task", False):
        y = forward(m, data, node_ids).double().cpu()
        want = torch.stack([y[labels == lab].sum(0) for lab in imp.group_labels.cpu().tolist()])
        assert_rule(total, want, what=f"{name}/{which}: mean * count against forward", floor=TWO_FLOORS)
    # |sum_d a| <= sum_d |a| row by row, so for the means (the same float32 terms on both sides: float64 rounding only)
    upper = imp.mean_abs.sum(dim=2)
    assert bool((imp.feature_mean_abs <= upper * (1 + 1e-12) + 1e-300).all())
    # no groups: one group of all requested rows, in the order given
    whole = interpret.importance(m, data, node_ids=node_ids)
    assert whole.rows.cpu().tolist() == ids.tolist() and whole.group_labels.cpu().tolist() == [0] and whole.count.cpu().tolist() == [R]
    assert_fields(whole, moments_of(truth, torch.zeros(R)), f"{name}/{which} ungrouped", 1e-5)


def check_rows_subset(dev, floor):
    m = build("models_tensor_node", dev)
    data = inputs_on("csr", dev)
    rows = [190, 3, 3, 0, 77, 12, 3]
    labels = [2, 0, 2, 0, 2, 2, 9]
    imp = interpret.importance(m, data, rows=rows, groups=labels)
    assert imp.rows.cpu().tolist() == [3, 0, 190, 3, 77, 12, 3] and imp.group_labels.cpu().tolist() == [0, 2, 9]
    assert imp.count.cpu().tolist() == [2.0, 4.0, 1.0]
    ex = interpret.explain(m, data, rows=rows)
    assert_fields(imp, moments_of(ex.by_feature_distance, labels), "rows subset against explain", floor)
    same = interpret.importance(m, data, node_ids=torch.tensor(rows), groups=torch.tensor(labels))
    for name in FIELDS:
        assert torch.equal(getattr(same, name), getattr(imp, name)), name
    try:
        interpret.importance(m, data, rows=rows, groups=labels[:-1])
    except ValueError as e:
        assert "one label per requested row" in str(e)
    else:
        raise AssertionError("a label list shorter than the rows must be refused")


def check_nam(dev, floor):
    from gnan_amd import models
    x = graph_case("dense")[0]
    m = models.NAM(F_RAW + 1, 3, 3, hidden_channels=8)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for _, p in m.named_parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * 0.4)
    m = m.to(dev).eval()
    labels = torch.arange(x.shape[0]) % 2
    imp = interpret.importance(m, x.to(dev), groups=labels)
    ex = interpret.explain(m, x.to(dev))
    assert tuple(imp.mean.shape)[:3] == (2, F_RAW + 1, 1) and imp.hops.cpu().tolist() == [0.0]
    assert_fields(imp, moments_of(ex.by_feature_distance, labels), "NAM against explain", floor)
    assert torch.equal(imp.feature_mean_abs, imp.mean_abs[:, :, 0])


def check_refusals(dev):
    import pytest
    from gnan_amd import _lib, batched
    m = build("models_tensor_node", dev)
    data = inputs_on("dense", dev)
    with pytest.raises(_lib.GnanHipError, match="eval"):
        interpret.importance(m.train(), data)
    with pytest.raises(_lib.GnanHipError, match="batched.TensorGNAN"):
        interpret.importance(batched.TensorGNAN(F_RAW + 1, 2, 2, hidden_channels=4).eval(), data)
    other = "meta" if torch.device(dev).type == "cpu" else "cpu"
    with pytest.raises(_lib.GnanHipError, match="ONE device"):
        interpret.importance(m.eval(), inputs_on("dense", other) if other == "cpu" else
                             type(data)(x=torch.empty(30, F_RAW + 1, device="meta")))
