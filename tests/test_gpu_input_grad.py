"""The two kernels of the table path's input gradient on the MI355X.

``gnan_fpwl_input_grad`` on hand-built tables (``moments_ref.hand_tables``) and hand-built derivative rows: EVERY element is held
to ``|gx - t| <= gamma_{C+1} sum_c |g_c| |d_c|`` with ``t`` the float64 sum of the kernel's own float32 inputs (a chain of C fused
multiply-adds from 0 commits at most C roundings; a zero bound demands an exact zero), integer-valued inputs are compared without
tolerance, the piece a node is put on is read back through a derivative table that holds every piece's own index, a NaN stays in
its element, two runs give the same bits and the launch's plan (``gnan_fpwl_input_grad_describe``) is asserted.

``gnan_pwl_piece_dfdx`` against its float64 restatement (``pwl.piece_derivatives_reference``) within one rounding,
``2^-24 |t| + 2^-149``, on tables of both builders; rows behind ``off[F]`` are zeros."""
import numpy as np
import pytest
import torch

import moments_ref as R
from gpu_util import DEV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")


def cyc(pattern, F):
    return [pattern[k % len(pattern)] for k in range(F)]


# name: (n, pieces per feature, C, features per group (None: the planner's), sum_features, x family, x view, grad view)
CASES = {
    "n1-F1-P1-C1": (1, [1], 1, None, False, "uniform", "plain", "plain"),
    "n255-F3-C2-sum": (255, [1, 2, 257], 2, None, True, "levels", "plain", "plain"),
    "n256-F16-C1-quads": (256, [256] * 14 + [1, 2], 1, 16, False, "onehot", "plain", "plain"),
    "n257-F16-C1-sum": (257, [256] * 14 + [1, 2], 1, 16, True, "cover", "plain", "plain"),
    "n1000-F20-C3": (1000, cyc([1, 2, 256, 257, 7], 20), 3, None, False, "rays", "plain", "plain"),
    "n1000-F33-C1-sum-ragged": (1000, cyc([5, 64, 2, 1, 130], 33), 1, 16, True, "uniform", "plain", "plain"),
    "n257-F33-C8-fg8": (257, cyc([5, 33, 2, 1, 17], 33), 8, 8, False, "levels", "plain", "plain"),
    "n255-F20-C9-fg4-sum": (255, cyc([9, 2, 65, 1], 20), 9, 4, True, "cover", "plain", "plain"),
    "n256-F3-C40-sum": (256, [257, 2, 130], 40, 1, True, "uniform", "plain", "plain"),
    "n1000-F16-C40": (1000, cyc([130, 64, 257], 16), 40, 1, False, "onehot", "plain", "plain"),
    "n257-F3-P1024-C1": (257, [1024, 2, 1], 1, None, False, "cover", "plain", "plain"),
    "n1000-F16-P1024-C1-fg4-sum": (1000, [1024] * 4 + [256] * 12, 1, 4, True, "uniform", "plain", "plain"),
    "n256-F20-C2-fg2": (256, cyc([257, 1, 2, 256], 20), 2, 2, False, "levels", "plain", "plain"),
    "n1000-F16-C1-offset-view": (1000, [130] * 16, 1, 16, False, "uniform", "offset1", "plain"),
    "n1000-F16-C1-aligned-view-sum": (1000, [130] * 16, 1, 16, True, "rays", "offset4", "plain"),
    "n257-F20-C3-strided-grad": (257, cyc([7, 256, 2], 20), 3, 4, False, "uniform", "plain", "strided"),
    "n255-F16-C8-strided-grad-sum": (255, cyc([40, 3], 16), 8, 8, True, "onehot", "offset1", "strided"),
}
_BUILT = {}


def build(name):
    """Inputs of a case, drawn once (numpy, float32) — every test of the case reads the same arrays."""
    if name not in _BUILT:
        n, counts, C, fg, sum_features, family, xview, gview = CASES[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        ht = R.hand_tables(counts, rng)
        F = ht.F
        x = R.draw_x(rng, family, ht, n)
        g = R.draw_g(rng, "unit", n, C if sum_features else F * C)
        dfdx = rng.standard_normal((int(ht.off[-1]), C)).astype(np.float32)
        _BUILT[name] = dict(ht=ht, x=x, g=g, dfdx=dfdx, rng=rng)
    return _BUILT[name]


def device_views(name, x, g):
    """x / grad on the device as the case views them: 'offset1' a column-offset view (rows not 16-byte aligned), 'offset4' one
    whose rows stay 16-byte aligned, 'strided' gradient rows with five floats of padding."""
    _, _, _, _, _, _, xview, gview = CASES[name]
    n, F = x.shape
    xt = torch.from_numpy(x)
    if xview == "plain":
        xd = xt.to(DEV)
    else:
        lead = 1 if xview == "offset1" else 4
        big = torch.full((n, F + lead + (3 if lead == 1 else 4)), float("nan"))
        big[:, lead:lead + F] = xt
        xd = big.to(DEV)[:, lead:lead + F]
    gt = torch.from_numpy(g)
    if gview == "plain":
        gd = gt.to(DEV)
    else:
        big = torch.full((n, g.shape[1] + 5), float("nan"))
        big[:, :g.shape[1]] = gt
        gd = big.to(DEV)[:, :g.shape[1]]
    return xd, gd


def tables_of(name, device=DEV):
    from gnan_amd import pwl
    _, _, C, fg, _, _, _, _ = CASES[name]
    b = build(name)
    t = R.as_pwl(b["ht"], C, np.random.default_rng(1), device, features_per_group=fg)
    assert not pwl.oversize(t), "the case must fit the thread-per-node look-up"
    return t


def truth_and_bound(x, g, dfdx, ht, C, sum_features):
    """float64 ``t[n, k] = sum_c g d`` and ``gamma_{C+1} sum_c |g| |d|`` from the float32 inputs; the owner by #{anchors[1:] <= x}."""
    own = R.owners(x, ht)
    n, F = x.shape
    t = np.empty((n, F))
    mag = np.empty((n, F))
    g64 = g.astype(np.float64)
    for k in range(F):
        d = dfdx[own[:, k]].astype(np.float64)                                  # [n, C]
        gk = g64 if sum_features else g64[:, k * C:(k + 1) * C]
        t[:, k] = (gk * d).sum(1)
        mag[:, k] = (np.abs(gk) * np.abs(d)).sum(1)
    return t, R.gamma(C + 1) * mag


def run(name, x, g, dfdx, describe=None):
    from gnan_amd import functional
    _, _, _, _, sum_features, _, _, _ = CASES[name]
    t = tables_of(name)
    xd, gd = device_views(name, x, g)
    gx = functional._fpwl_input_grad(xd, t, torch.from_numpy(dfdx).to(DEV), gd, sum_features, describe=describe)
    torch.cuda.synchronize()
    return gx.cpu().numpy()


def expected_plan(name, x_is_aligned):
    from gnan_amd import pwl
    n, counts, C, _, _, _, xview, _ = CASES[name]
    t = tables_of(name, "cpu")
    F, fg = len(counts), t.features_per_group
    npb = min(4096, max(256, (n // 1024 + 255) // 256 * 256))
    x_stride = F if xview == "plain" else F + (4 if xview == "offset1" else 8)
    vec = int(fg % 4 == 0 and F % 4 == 0 and x_stride % 4 == 0 and x_is_aligned)
    return dict(block_size=512 if fg >= 8 else 256, nodes_per_block=npb, features_per_group=fg,
                lds_bytes=t.max_group_pieces * (1 + pwl.table_stride(C)) * 4, vec=vec, n_groups=-(-F // fg), n_blocks=-(-n // npb))


@pytest.mark.parametrize("name", list(CASES))
def test_every_element_within_its_bound(name):
    n, counts, C, _, sum_features, _, xview, _ = CASES[name]
    b = build(name)
    d = []
    gx = run(name, b["x"], b["g"], b["dfdx"], describe=d)
    assert d[0] == expected_plan(name, xview != "offset1"), d[0]
    assert gx.shape == b["x"].shape and gx.dtype == np.float32
    t, bound = truth_and_bound(b["x"], b["g"], b["dfdx"], b["ht"], C, sum_features)
    err = np.abs(gx.astype(np.float64) - t)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    assert np.all(err <= bound), f"{name}: element {worst}: |err| {err[worst]:.3e} > bound {bound[worst]:.3e}"
    assert np.array_equal(run(name, b["x"], b["g"], b["dfdx"]).view(np.uint32), gx.view(np.uint32)), "two runs, two results"


@pytest.mark.parametrize("name", list(CASES))
def test_integer_inputs_are_exact_and_zero_rows_give_zeros(name):
    """Integer-valued gradient and derivative rows: every product and partial sum is an integer below 2^24 — no tolerance.
    Rows of the gradient that are zero give exact zeros (a zero bound)."""
    n, counts, C, _, sum_features, _, _, _ = CASES[name]
    b = build(name)
    rng = np.random.default_rng(7)
    g = R.draw_g(rng, "integers", n, b["g"].shape[1])
    g[::3] = 0.0
    dfdx = rng.integers(-4, 5, b["dfdx"].shape).astype(np.float32)
    gx = run(name, b["x"], g, dfdx)
    t, bound = truth_and_bound(b["x"], g, dfdx, b["ht"], C, sum_features)
    assert np.array_equal(gx.astype(np.float64), t)
    assert np.all(bound[::3] == 0) and np.all(gx[::3] == 0)


@pytest.mark.parametrize("name", list(CASES))
def test_piece_ownership_is_the_forwards(name):
    """A derivative table that holds every piece's own index in channel 0 (zeros elsewhere) and a unit gradient: ``gx`` IS the
    piece the kernel put the node on — compared with ``#{anchors[1:] <= x}`` (x on anchors: 'levels', 'onehot', 'cover')."""
    n, counts, C, _, sum_features, _, _, _ = CASES[name]
    b = build(name)
    ht = b["ht"]
    dfdx = np.zeros(b["dfdx"].shape, dtype=np.float32)
    for k in range(ht.F):
        dfdx[ht.off[k]:ht.off[k + 1], 0] = np.arange(ht.off[k + 1] - ht.off[k])
    g = np.ones(b["g"].shape, dtype=np.float32)
    gx = run(name, b["x"], g, dfdx)
    own = R.owners(b["x"], ht) - ht.off[:-1][None, :]
    assert np.array_equal(gx.astype(np.int64), own)


@pytest.mark.parametrize("name", ["n1000-F33-C1-sum-ragged", "n257-F33-C8-fg8", "n1000-F16-C1-aligned-view-sum", "n257-F20-C3-strided-grad",
                                  "n256-F16-C1-quads"])
def test_a_nan_stays_in_its_element(name):
    """gx[n, k] depends on x[n, k] and row n of grad alone.  A NaN x is owned by piece 0 (no anchor is <= NaN) and changes nothing
    else; a NaN gradient entry makes NaN what reads it — its feature's element in the per-feature layout, its row with sum_features."""
    n, counts, C, _, sum_features, _, _, _ = CASES[name]
    b = build(name)
    F = len(counts)
    clean = run(name, b["x"], b["g"], b["dfdx"])
    r0, k0 = n // 2, F - 1
    x = b["x"].copy()
    x[r0, k0] = np.nan
    got = run(name, x, b["g"], b["dfdx"])
    mask = np.ones(clean.shape, dtype=bool)
    mask[r0, k0] = False
    assert np.array_equal(got.view(np.uint32)[mask], clean.view(np.uint32)[mask])
    lo = x.copy()
    lo[r0, k0] = -1.0e30                               # piece 0 by the rule
    assert got.view(np.uint32)[r0, k0] == run(name, lo, b["g"], b["dfdx"]).view(np.uint32)[r0, k0]
    g = b["g"].copy()
    r1, k1 = n - 1, min(1, F - 1)
    col = 0 if sum_features else k1 * C + C - 1
    g[r1, col] = np.nan
    got = run(name, b["x"], g, b["dfdx"])
    hit = np.zeros(clean.shape, dtype=bool)
    if sum_features:
        hit[r1, :] = True
    else:
        hit[r1, k1] = True
    assert np.all(np.isnan(got[hit])) and np.array_equal(got.view(np.uint32)[~hit], clean.view(np.uint32)[~hit])


def test_oversize_tables_and_no_nodes():
    from gnan_amd import _lib, functional, pwl
    rng = np.random.default_rng(3)
    ht = R.hand_tables([1024, 5], rng)
    t = R.as_pwl(ht, 40, rng, DEV, features_per_group=1)
    assert pwl.oversize(t)
    x = torch.zeros(10, 2, device=DEV)
    with pytest.raises(_lib.GnanHipError, match="exceed"):
        functional._fpwl_input_grad(x, t, torch.zeros(1029, 40, device=DEV), torch.zeros(10, 40, device=DEV), True)
    small = R.as_pwl(R.hand_tables([3, 5], rng), 2, rng, DEV)
    d = []
    gx = functional._fpwl_input_grad(x[:0], small, torch.zeros(8, 2, device=DEV), torch.zeros(0, 2, device=DEV), True, describe=d)
    assert gx.shape == (0, 2) and all(v == 0 for v in d[0].values())
    torch.cuda.synchronize()


# ---- gnan_pwl_piece_dfdx --------------------------------------------------------------------------------------------------
# (F, L, H, C, biases: True / False / "zero" = bias tensors that are all zero, every kink at 0)
DFDX_CASES = [(3, 2, 8, 1, True), (2, 2, 128, 3, True), (4, 3, 16, 2, True), (3, 3, 64, 1, True), (3, 4, 16, 3, True),
              (2, 4, 64, 1, True), (3, 2, 8, 2, False), (3, 3, 16, 1, False), (2, 4, 64, 2, False), (3, 3, 64, 40, "zero"),
              (4, 2, 128, 1, "zero"), (3, 4, 16, 1, "zero"), (2, 3, 64, 130, True), (2, 2, 128, 70, True)]


def _dfdx_tables(case, backend):
    from gnan_amd import pwl
    from test_gpu_deep_tables import _mlp_state
    F, L, H, C, bias = case
    sd = _mlp_state(F, L, H, C, bool(bias), seed=F * 7 + H + L)
    if bias == "zero":
        for key in sd:
            if key.endswith(".bias") and not key.endswith(f".{3 * (L - 1)}.bias"):
                sd[key].zero_()
    from gnan_amd.functional import StackedMLP

    def cat(li, what):
        return torch.stack([sd[f"fs.{k}.{3 * li}.{what}"] for k in range(F)], 0).to(DEV)
    has = bool(bias)
    w_mid = torch.stack([cat(li, "weight") for li in range(1, L - 1)], 0) if L > 2 else None
    b_mid = torch.stack([cat(li, "bias") for li in range(1, L - 1)], 0) if (L > 2 and has) else None
    st = StackedMLP(cat(0, "weight")[..., 0], cat(0, "bias") if has else None, w_mid, b_mid, cat(L - 1, "weight"),
                    cat(L - 1, "bias") if has else None, L, H, C, F)
    saved = pwl.BUILD_BACKEND
    try:
        pwl.BUILD_BACKEND = backend
        assert pwl.hip_build_applies(st) == (backend == "auto")
        t = pwl.build_tables(st, use_graph=False)
    finally:
        pwl.BUILD_BACKEND = saved
    assert t is not None
    return st, t


@pytest.mark.parametrize("backend", ["auto", "torch"], ids=["hip-builder", "torch-builder"])
@pytest.mark.parametrize("case", DFDX_CASES, ids=lambda c: "-".join(map(str, c)))
def test_piece_derivatives_within_one_rounding(case, backend):
    from gnan_amd import _lib, functional, pwl
    F, L, H, C, bias = case
    st, t = _dfdx_tables(case, backend)
    got = functional._piece_dfdx_launch(list(st[:6]), t, L, H, C, F)
    again = functional._piece_dfdx_launch(list(st[:6]), t, L, H, C, F)
    want = pwl.piece_derivatives_reference(st, t)
    torch.cuda.synchronize()
    assert got.shape == want.shape == (t.anchor.numel(), C) and torch.equal(got, again)
    err = (got.double() - want).abs()
    bound = 2.0 ** -24 * want.abs() + 2.0 ** -149
    worst = int(torch.argmax(err - bound))
    assert bool((err <= bound).all()), f"row {worst // C} channel {worst % C}: |err| {float(err.view(-1)[worst]):.3e} > {float(bound.view(-1)[worst]):.3e}"
    if bias == "zero":
        up = torch.nextafter(t.anchor, torch.full_like(t.anchor, float("inf")))
        assert bool(((t.anchor[1:] > t.anchor[:-1]) & (t.anchor[1:] <= up[:-1])).any()), "no point piece in the tables"
    # capacity rows: a buffer with 37 rows behind off[F], prefilled with NaN — the pieces as before, zeros behind them
    T = t.anchor.numel()
    anchor = torch.cat([t.anchor, torch.full((37,), float("nan"), device=DEV)])
    out = torch.full((T + 37, C), float("nan"), device=DEV)
    keep = [None if q is None else q.detach().float().contiguous() for q in st[:6]]
    a = _lib.PwlDfdxArgs(off=_lib.ptr(t.off), anchor=_lib.ptr(anchor), T=T + 37, w_first=_lib.ptr(keep[0]), b_first=_lib.ptr(keep[1]),
                         w_mid=_lib.ptr(keep[2]), b_mid=_lib.ptr(keep[3]), w_last=_lib.ptr(keep[4]), F=F, L=L, H=H, C=C,
                         dfdx=_lib.ptr(out))
    _lib.check(_lib.lib().gnan_pwl_piece_dfdx(a, _lib.stream_of(out)), "gnan_pwl_piece_dfdx")
    torch.cuda.synchronize()
    assert torch.equal(out[:T], got) and bool((out[T:] == 0).all())
