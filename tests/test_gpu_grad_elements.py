"""``gnan_fpwl_param_grads`` (csrc/fpwl_grad.hip: fpwl_grad2_kernel, fpwl_grad3_kernel<NG, CQ>, fpwl_grad3_sweep_kernel,
fpwl_grad4_kernel<2, CQ>) element by element against the exact reference of tests/grads_ref.py, on the case matrix of
tests/grads_cases.py: every element of all six gradient tensors inside ``u32 |t| + (1 + u32) gamma64_k Mag + 2^-149`` with the
kernel's own counted ``k``, exact zeros where the bound is zero, the same bits twice, and the integer families bit for bit.

Every case goes through ``functional._fpwl_param_grads_launch`` with the moments handed in (int64 with power-of-two scales, or
float32): no nodes, a launch of microseconds.  The tables record's ``max_pieces`` picks the kernel.  The random, range and thirds
families take their tables from the kernel builder (``gnan_pwl_build``); the two real-chain cases also take the raw moments of
``_fpwl_moments(raw=True)`` and feed those very integers to the reference."""
import numpy as np
import pytest
import torch

import grads_cases as GC
import grads_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
KERNEL_TABLES = ("L2-H5-C4", "L2-H33-C5", "L3-sweep-H5-C1", "L3-sweep-H33-C3", "L3-piece4-H5-C1", "L3-piece2-H8-C8",
                 "L4-H8-C8", "L4-H33-C4", "L3-range", "L3-range-piece", "L4-range", "L2-range", "L3-thirds", "L3-thirds-piece",
                 "L4-thirds")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


def _to(p, dev):
    return type(p)(*[None if q is None else q.to(dev) for q in p[:6]], *p[6:])


def _launch(case):
    from gnan_amd import functional, pwl
    p = _to(case.p, DEV)
    T = int(case.off[-1])
    t = pwl.PwlTables(torch.from_numpy(case.off).to(DEV), torch.from_numpy(np.concatenate(case.anchors)).to(DEV),
                      torch.zeros(T, p.C, device=DEV), torch.zeros(T, p.C, device=DEV), int(case.max_pieces), 1,
                      int(case.max_pieces))
    if case.exps is None:
        moments = torch.from_numpy(np.ascontiguousarray(case.M, dtype=np.float32)).to(DEV)
    else:
        scales = torch.tensor([2.0 ** case.exps[0], 2.0 ** case.exps[1]], dtype=torch.float64, device=DEV)
        moments = (torch.from_numpy(np.ascontiguousarray(case.M, dtype=np.int64)).to(DEV), scales)
    runs = []
    for _ in range(2):
        got = functional._fpwl_param_grads_launch(list(p[:6]), t, moments, p.L, p.H, p.C, p.F)
        torch.cuda.synchronize()
        runs.append([None if g is None else g.cpu() for g in got])
    return runs


def _hold(case):
    first, second = _launch(case)
    for a, b in zip(first, second):
        assert (a is None and b is None) or torch.equal(a, b), "the same bits twice"
    ref = G.reference(case)
    assert sum(ex.undecided for ex in ref) == 0
    got = G.split(case, first)
    ratio, where, zero_bounds = G.hold(case, got)
    print(f"GRAD-ELEMENTS {case.name} route={case.route[0]}/{case.route[1]} nl={[ex.nl for ex in ref]} ratio={ratio:.4f} "
          f"at={where} zero_bounds={zero_bounds}")
    assert ratio <= 1.0, (case.name, ratio, where)
    if case.exact:
        for g, ex in zip(got, ref):
            for nm, a in g.items():
                want = np.array([float(t) for t in ex.grads[nm].reshape(-1)], dtype=np.float64)
                assert np.array_equal(a.reshape(-1).astype(np.float64), want), (case.name, nm)
    return first


@pytest.mark.parametrize("name", GC.ALL)
def test_every_element_is_inside_its_bound(name):
    _hold(GC.case(name))


@pytest.mark.parametrize("name", KERNEL_TABLES)
def test_every_element_on_the_kernel_builders_tables(name):
    from gnan_amd import pwl

    def tables(p):
        pd = _to(p, DEV)
        assert pwl.hip_build_applies(pd)
        return pwl.build_tables(pd)
    case = GC.case(name, tables=tables)
    _hold(case._replace(name=name + "@gnan_pwl_build"))


@pytest.mark.parametrize("tag", ["L2", "sweep", "piece4", "piece2", "L4"])
def test_power_of_two_scales_move_the_exponent_only(tag):
    unit = _launch(GC.case(f"integer-{tag}-e0"))[0]
    for e in (100, -100):
        moved = _launch(GC.case(f"integer-{tag}-e{e}"))[0]
        for a, b in zip(unit, moved):
            if a is None:
                continue
            assert torch.equal(torch.ldexp(a, torch.tensor(-e)), b), (tag, e)
            nz = b[b != 0].abs()
            assert nz.numel() == 0 or float(nz.min()) >= 2.0 ** -126


@pytest.mark.parametrize("L,H,C,seed", [(3, 8, 1, 71), (4, 8, 2, 72)])
def test_real_chain_tables_and_raw_moments(L, H, C, seed):
    """Tables from ``gnan_pwl_build``, raw int64 moments from ``_fpwl_moments(raw=True)`` (n = 2000, F = 3): those very integers
    go to the kernel and to the reference."""
    import math
    import tables_ref as R
    from gnan_amd import functional, pwl
    F, n = 3, 2000
    p = R.random_state(F, L, H, C, True, seed)
    pd = _to(p, DEV)
    t = pwl.build_tables(pd)
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(n, F, generator=g) * 4 - 2).to(DEV)
    grad = torch.randn(n, F * C, generator=g).to(DEV)
    Mi, scales = functional._fpwl_moments(x, t, grad, False, raw=True)
    exps = tuple(int(round(math.log2(float(s)))) for s in scales.cpu())
    assert all(2.0 ** e == float(s) for e, s in zip(exps, scales.cpu())), "power-of-two scales"
    off = t.off.cpu().tolist()
    anchor = t.anchor.cpu().numpy()
    anchors = [anchor[off[k]:off[k + 1]].copy() for k in range(F)]
    case = G.Case(f"real-chain-L{L}", p, anchors, Mi.cpu().numpy()[:off[F]], exps, int(t.max_pieces), G.features_of(p, kinks=False))
    assert case.route[0] == ("sweep" if L == 3 else "grad4")
    _hold(case)
