"""The narrow aggregation's restatements of tests/rowwise.py pinned without a GPU.

``emulate_pb`` restates the propagation-blocked forward (csrc/spmm_pb.hip) in the kernel's OWN arithmetic on the plan's arrays:
``to_fixed`` on every expanded entry, wrapping int64 sums per accumulator slot, the float32 epilogue of ``fwd_rows`` with fmaf as the
exact product plus one rounding.  It must sit inside ``rowwise.pb_reference``'s bound on every operand family, its shell sums must
equal ``rowwise.pb_shell_exact`` bit for bit, and each planted mutant must fail at least one of the two.  The truths of the forward
and backward references are held to the oracle's float64 ``spmm_csr`` and its autograd."""
import numpy as np
import pytest
import torch

import rowwise
from oracle import gnan_oracle as O

MUTANTS = ("coarse", "absmax_listed", "next_weight", "self_w0", "drop_slot", "nearest")


def _fma32(a, b, c):
    """fmaf on float32 arrays, correctly rounded: the product of two float32 is exact in float64; the float64 sum is rounded to odd
    (TwoSum gives its error), after which the rounding to float32 is the single rounding of the exact value."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _to_fixed(v, shift, nearest=False):
    """The emulation's own ``v * 2^shift`` as int64, not ``rowwise.to_fixed``: the value is split by ``frexp`` (exact for subnormals
    too), its 24-bit mantissa scaled as a Python integer and cut toward zero.  ``nearest``: the mutant that rounds to nearest."""
    v = np.asarray(v, dtype=np.float32)
    frac, ex = np.frexp(v.astype(np.float64))                           # v = frac * 2^ex, |frac| in [0.5, 1): frac * 2^24 is an integer
    mant = np.abs(frac * 2.0 ** 24).astype(np.int64)
    sh = ex.astype(np.int64) - 24 + int(shift)
    out = np.empty(v.shape, dtype=np.int64)
    for i, (m, s, neg) in enumerate(zip(mant.ravel().tolist(), sh.ravel().tolist(), (v.ravel() < 0).tolist())):
        x = m << s if s >= 0 else ((m + ((1 << (-s - 1)) if nearest else 0)) >> -s if -s < 80 else 0)
        out.ravel()[i] = -x if neg else x
    return out


def _plan(monkeypatch, rowptr, col, code, n_cols, D, W, cnt=None, lds=None):
    from gnan_amd import HopGraph, graph as G
    monkeypatch.setattr(G, "PB_LDS_BYTES", 1024 * W if lds is None else lds)
    monkeypatch.setattr(G, "PB_SLOT_PAIRS", 8)
    g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=n_cols, n_codes=D,
                          cnt=None if cnt is None else torch.from_numpy(cnt))
    plan = g.pb_plan(W)
    assert plan is not None
    return g, plan


def emulate_pb(plan, g, S, lut, use_cnt, s_total, mutant=None):
    """``(Y float32 [n, W], the rows' scaled shell sums float32 [n, n_acc, W])`` of pb_expand_kernel + pb_reduce_kernel."""
    from gnan_amd import graph as G
    S = np.ascontiguousarray(S, dtype=np.float32)
    n, W, D, n_acc, R = g.n_rows, S.shape[1], g.n_codes, plan.n_acc, plan.acc_per_bin
    src, dst = plan.src.numpy().astype(np.int64), plan.dst.numpy().astype(np.int64)
    # phase 1: every entry expanded by exactly one column block
    E = np.zeros((plan.n_entries, W), dtype=np.float32)
    written = np.zeros(plan.n_entries, dtype=np.int64)
    chunk_q, cptr = plan.chunk_q.numpy().astype(np.int64), plan.cb_chunk_ptr.numpy()
    for cb in range(plan.n_cblocks):
        q = (chunk_q[cptr[cb]:cptr[cb + 1], None] + np.arange(G.PB_CHUNK)[None, :]).ravel()
        assert np.all(src[q] < plan.cb_width)
        E[q] = S[np.minimum(cb * plan.cb_width + src[q], g.n_cols - 1)]
        written[q] += 1
    assert np.all(written == 1)
    # phase 2: the entries of a bin are one contiguous range; slot -> row through slot_ptr
    eptr, rptr, slot_ptr = plan.bin_entry_ptr.numpy().astype(np.int64), plan.bin_row_ptr.numpy().astype(np.int64), plan.slot_ptr.numpy().astype(np.int64)
    assert eptr[-1] == plan.n_entries and rptr[-1] == n and sorted(plan.bin_order.tolist()) == list(range(plan.n_bins))
    real = np.nonzero(dst != R - 1)[0]
    assert len(real) == plan.n_pairs
    b = np.searchsorted(eptr, real, side="right") - 1
    gslot = slot_ptr[rptr[b]] + dst[real] // n_acc
    a = dst[real] % n_acc
    row = np.searchsorted(slot_ptr, gslot, side="right") - 1
    assert np.all((row >= rptr[b]) & (row < rptr[b + 1])), "an entry adds to a row of another bin"
    mx = np.abs(E[real]).max() if mutant == "absmax_listed" else np.abs(S).max()
    e = int(np.frexp(np.float32(mx))[1]) if mx > 0 else 0
    shift = 62 - plan.headroom_bits - e - (8 if mutant == "coarse" else 0)
    fixed = _to_fixed(E[real], shift, nearest=mutant == "nearest")
    if mutant == "drop_slot":
        last = (gslot == slot_ptr[row + 1] - 1) & (slot_ptr[row + 1] - slot_ptr[row] > 1)
        assert last.any()
        row, a, fixed = row[~last], a[~last], fixed[~last]
    T = np.zeros((n, n_acc, W), dtype=np.int64)
    np.add.at(T, (row, a), fixed)                                       # (int64 wraps, as the LDS atomics do)
    tf = (T.astype(np.float64) * np.ldexp(1.0, -shift)).astype(np.float32)
    # the epilogue, float32 throughout
    l = lut.reshape(-1).astype(np.float32)
    wt = np.broadcast_to(l[None, :], (n, D)).copy()
    if use_cnt:
        wt = (wt / np.maximum(g.cnt.numpy(), 1).astype(np.float32)).astype(np.float32)
    w_rest = wt[:, D - 1].copy() if s_total is not None else np.zeros(n, dtype=np.float32)
    out = np.zeros((n, W), dtype=np.float32)
    if plan.self_col is not None:
        sc = plan.self_col.numpy().astype(np.int64)
        have = sc >= 0
        w_self = wt[:, 0] if mutant == "self_w0" else (wt[:, 0] - w_rest).astype(np.float32)
        out[have] = _fma32(w_self[have, None], S[sc[have]], out[have])
    for k in range(n_acc):
        d = plan.code_base + k + (1 if (mutant == "next_weight" and D == 4) else 0)
        out = _fma32((wt[:, d] - w_rest).astype(np.float32)[:, None], tf[:, k], out)
    if s_total is not None:
        out = _fma32(w_rest[:, None], np.asarray(s_total, dtype=np.float32)[None, :], out)
    return out, tf


def _case(monkeypatch, D, W, layout, top, shape, seed):
    rng = np.random.default_rng(seed)
    rowptr, col, code = rowwise.narrow_csr(rng, shape[0], shape[1], D, layout, top)
    g, plan = _plan(monkeypatch, rowptr, col, code, shape[1], D, W)
    assert plan.n_bins > 3 and plan.n_cblocks > 3
    longest = top + int(plan.code_base == 0 and D > 2 and layout != "none")          # (a bucketed code 0: the self pair is accumulated too)
    assert plan.headroom_bits == (longest - 1).bit_length() and (plan.code_base == 0 or plan.headroom_bits == {64: 6, 65: 7, 128: 7, 129: 8, 150: 8}[top])
    assert int((plan.slot_ptr[1:] - plan.slot_ptr[:-1]).max()) == -(-longest // 8)
    assert not bool((col == shape[1] - 1).any())
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    return rng, rowptr, col, code, g, plan, lut


def _judge(rowptr, col, code, g, plan, S, lut, use_cnt, with_rest, mutant=None):
    """``(worst |err| / bound, shell sums equal pb_shell_exact)`` of the emulation on one operand."""
    s_total = S.astype(np.float64).sum(0).astype(np.float32) if with_rest else None
    y, tf = emulate_pb(plan, g, S, lut, use_cnt, s_total, mutant)
    truth, bound = rowwise.pb_reference(rowptr, col, code, S, lut, g.cnt.numpy() if use_cnt else None, s_total,
                                        plan.headroom_bits, plan.code_base)
    ratio = rowwise.worst_ratio(y, truth, bound)
    same = True
    if plan.n_acc == 1:
        want = rowwise.pb_shell_exact(rowptr, col, code, S, plan.headroom_bits, plan.code_base).reshape(g.n_rows, -1)
        same = bool(np.array_equal(tf[:, 0, :].view(np.uint32), want.view(np.uint32)))
    return ratio, same


@pytest.mark.parametrize("D,W,layout,use_cnt,with_rest,top,shape", rowwise.NARROW_CASES)
def test_emulation_sits_inside_the_bound_and_its_shell_sums_are_exact(D, W, layout, use_cnt, with_rest, top, shape, monkeypatch):
    rng, rowptr, col, code, g, plan, lut = _case(monkeypatch, D, W, layout, top, shape, D * 100 + W * 10 + top)
    if layout in ("self",) and D > 2:
        assert plan.code_base == 1 and plan.self_is_row == (shape[0] <= shape[1])
    if layout == "double" or D == 2:
        assert plan.code_base == 0 and plan.self_col is None
    if layout == "none" and D > 2:
        assert plan.code_base == 1 and int(plan.self_col.max()) == -1
    worst = {}
    for fam in rowwise.NARROW_FAMILIES:
        S = rowwise.narrow_operand(rng, fam, shape[1], W)
        worst[fam], same = _judge(rowptr, col, code, g, plan, S, lut, use_cnt, with_rest)
        assert same, f"{fam}: the emulation's shell sums differ from pb_shell_exact"
    assert all(r < 1.0 for r in worst.values()), f"worst |err| / bound per family: {worst}"
    print("NARROW-EMU", (D, W, layout, top), {k: round(v, 3) for k, v in worst.items()})


def test_every_emulation_mutant_fails_a_case(monkeypatch):
    """Each planted error leaves the bound, or the exact shell sums, on at least one case — and the cases it must fail on are named."""
    failed = {m: [] for m in MUTANTS}
    for D, W, layout, use_cnt, with_rest, top, shape in [c for c in rowwise.NARROW_CASES if c[1] == 1 or c[0] == 4][:9]:
        rng, rowptr, col, code, g, plan, lut = _case(monkeypatch, D, W, layout, top, shape, D * 100 + W * 10 + top)
        for fam in rowwise.NARROW_FAMILIES:
            S = rowwise.narrow_operand(rng, fam, shape[1], W)
            for m in MUTANTS:
                if m == "next_weight" and D != 4:
                    continue
                if m == "self_w0" and (plan.self_col is None or not with_rest):
                    continue
                ratio, same = _judge(rowptr, col, code, g, plan, S, lut, use_cnt, with_rest, m)
                if not (ratio < 1.0):
                    failed[m].append((D, W, layout, fam, "bound"))
                elif not same:
                    failed[m].append((D, W, layout, fam, "shell"))
    for m in MUTANTS:
        assert failed[m], f"mutant {m} passes every case"
    assert any(f[3] == "range" and f[4] == "bound" for f in failed["coarse"])          # an operand of many magnitudes sees 2^8
    assert any(f[3] == "outlier" for f in failed["absmax_listed"])                     # only an unlisted row pins absmax
    assert all(f[4] == "shell" for f in failed["nearest"])                             # half a quantum: the exact check alone
    print("NARROW-MUTANTS", {m: len(v) for m, v in failed.items()})


@pytest.mark.parametrize("D,W,layout,with_rest,top", [(3, 1, "self", True, 150), (4, 2, "none", True, 129), (2, 4, "self", False, 65),
                                                      (4, 1, "double", True, 128), (3, 4, "moved", True, 64)])
@pytest.mark.parametrize("weights", ["quarters", "sixteenths"])
def test_integer_cases_are_exact(D, W, layout, with_rest, top, weights, monkeypatch):
    """Integer operand, weights in quarters — and in sixteenths through counts of 1, 2 and 4: every product and partial sum is exact in
    float32, the fixed point holds integers exactly, so the emulation equals the int64 sum with no tolerance."""
    rng = np.random.default_rng(D + W + top)
    n_rows, n_cols = 700, 900
    rowptr, col, code = rowwise.narrow_csr(rng, n_rows, n_cols, D, layout, top)
    cnt = (2 ** rng.integers(0, 3, (n_rows, D))).astype(np.int32) if weights == "sixteenths" else None
    g, plan = _plan(monkeypatch, rowptr, col, code, n_cols, D, W, cnt=cnt)
    S = rowwise.narrow_operand(rng, "integers", n_cols, W)
    lut = (rng.integers(-8, 9, (D, 1)) / 4.0).astype(np.float32)
    s_total = S.sum(0) if with_rest else None
    scale = 4 if cnt is None else 16
    t, a = rowwise.exact_scaled(rowptr, col, code, S, lut, s_total, 0, cnt, scale)
    assert int(a.max()) < 2 ** 24
    y, _ = emulate_pb(plan, g, S, lut, cnt is not None, s_total)
    assert np.array_equal(y.astype(np.float64) * scale, t.numpy().astype(np.float64))


@pytest.mark.parametrize("D,W,layout,use_cnt,with_rest", [(3, 1, "self", True, True), (4, 2, "moved", True, False), (2, 1, "self", False, True),
                                                          (4, 4, "none", True, True)])
def test_reference_truths_equal_the_oracle(D, W, layout, use_cnt, with_rest):
    """pb_reference's and narrow_bwd_reference's truths == the oracle's float64 spmm_csr and its autograd, to 1e-12."""
    from gnan_amd import HopGraph, graph as G
    assert rowwise.LONG_ROW_THRESHOLD_NARROW == G.LONG_ROW_THRESHOLD_NARROW
    rng = np.random.default_rng(D + 10 * W)
    n = 500
    rowptr, col, code = rowwise.narrow_csr(rng, n, n, D, layout, 65, hubs=((5, 64), (101, 65)))
    g = HopGraph.from_csr(torch.from_numpy(rowptr), torch.from_numpy(col), torch.from_numpy(code), n_cols=n, n_codes=D)
    S = rowwise.narrow_operand(rng, "unit", n, W)
    lut = rng.standard_normal((D, 1)).astype(np.float32)
    dY = rng.standard_normal((n, W)).astype(np.float32)
    S64, lut64 = torch.from_numpy(S).double().requires_grad_(True), torch.from_numpy(lut).double().requires_grad_(True)
    wt = lut64.unsqueeze(0).expand(n, -1, -1)
    if use_cnt:
        wt = wt / g.cnt.clamp_min(1).double().unsqueeze(-1)
    want = O.spmm_csr(rowptr, col, code, S64, wt, with_rest=with_rest)
    tot = S64.detach().sum(0) if with_rest else None
    cnt = g.cnt.numpy() if use_cnt else None
    truth, bound = rowwise.pb_reference(rowptr, col, code, S, lut, cnt, tot, 7, 1)
    assert np.abs(truth - want.detach().numpy()).max() <= 1e-12 * max(1.0, float(want.detach().abs().max()))
    assert np.all(bound >= 0)
    gS, gl = torch.autograd.grad(want, [S64, lut64], torch.from_numpy(dY).double())
    for route in ("rows", "pb1", "pb2"):
        dS, dSb, dl, dlb = rowwise.narrow_bwd_reference(rowptr, col, code, S, lut, cnt, dY, tot, route, 7, 1, 7)
        assert np.abs(dS - gS.numpy()).max() <= 1e-12 * max(1.0, float(gS.abs().max())), route
        assert np.abs(dl - gl.numpy().reshape(-1)).max() <= 1e-12 * max(1.0, float(gl.abs().max())), route
        assert np.all(dSb >= 0) and np.all(dlb >= 0) and dSb.shape == dS.shape and dlb.shape == dl.shape
