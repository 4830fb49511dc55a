"""The exact reference of the table path's parameter gradients (tests/grads_ref.py) checked against itself, the numpy emulations
of the kernels' two algorithms and the torch route held to it on every case of tests/grads_cases.py, and planted errors that
each fail a named case.  No GPU.  The kernels themselves: tests/test_gpu_grad_elements.py."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import grads_cases as GC
import grads_ref as G


def _old_rule(case, per_feature, tol=1e-5):
    """The older tests' rule: every element within ``tol`` of the largest gradient entry over all parameters of all features."""
    ref = G.reference(case)
    scale = max(abs(float(t)) for ex in ref for a in ex.grads.values() for t in a.reshape(-1))
    worst = 0.0
    for got, ex in zip(per_feature, ref):
        for name, g in got.items():
            T = np.array([float(t) for t in ex.grads[name].reshape(-1)])
            worst = max(worst, float(np.abs(np.asarray(g, np.float64).reshape(-1) - T).max(initial=0.0)))
    return worst <= tol * scale


# ---- every case: decided masks, the emulation of its kernel under the bound ----------------------------------------------------------
@pytest.mark.parametrize("name", GC.ALL)
def test_case_is_decided_and_its_emulation_is_inside_the_bound(name):
    case = GC.case(name)
    ref = G.reference(case)
    assert sum(ex.undecided for ex in ref) == 0, "a committed case has no undecided mask"
    got = G.emulate(case)
    ratio, where, _ = G.hold(case, got, k_scale=2)
    assert ratio <= 1.0, (name, ratio, where)
    if name.startswith("point-"):
        assert sum(ex.point_zeros for ex in ref) > 0, "the case is about exact zeros of a hidden unit on an anchor"
    if case.exact:
        for g, ex in zip(got, ref):
            for nm, a in g.items():
                T = ex.grads[nm].reshape(-1)
                for gv, t in zip(a.reshape(-1), T):
                    assert Fraction(float(gv)) == t, (name, nm, float(gv), float(t))
                    assert t == 0 or 2.0 ** -126 <= abs(float(t)) < 2.0 ** 127


@pytest.mark.parametrize("name", [n for n in GC.ALL if "sweep" in n or n in ("L3-range", "L3-dead", "L3-thirds", "L3-no-bias")])
def test_sweep_cases_on_the_per_piece_emulation_as_well(name):
    """What the sweep is given, the four-group per-piece algorithm computes too (``max_pieces = 1025`` routes it there)."""
    case = GC.case(name)
    assert case.route[0] == "sweep"
    other = case._replace(name=name + "/max_pieces=1025", max_pieces=1025)
    assert other.route == ("grad3", 4)
    ratio, where, _ = G.hold(other, G.emulate(other), k_scale=2)
    assert ratio <= 1.0, (name, ratio, where)


@pytest.mark.parametrize("tag", ["L2", "sweep", "piece4", "piece2", "L4"])
def test_power_of_two_scales_move_the_exponent_only(tag):
    """Scales of 2^(+-100) give the unit result times 2^(-+100), bit for bit, inside the float32 normal range."""
    unit = G.emulate(GC.case(f"integer-{tag}-e0"))
    for e in (100, -100):
        moved = G.emulate(GC.case(f"integer-{tag}-e{e}"))
        for a, b in zip(unit, moved):
            for nm in a:
                want = np.ldexp(a[nm].astype(np.float64), -e).astype(np.float32)
                assert np.array_equal(want, b[nm]), (tag, e, nm)
                nz = np.abs(b[nm][b[nm] != 0])
                assert nz.size == 0 or (nz.min() >= 2.0 ** -126 and np.isfinite(nz).all())


# ---- the reference against two independent restatements ----------------------------------------------------------------------------------
def _brute_force(ex, A, M, exps):
    """Fractions all the way, masks from ``preacts_direct`` at ``xi``; loops, no shared code with :func:`grads_ref._pass`."""
    H, C, L, S = ex.H, ex.C, ex.L, ex.S
    sc = Fraction(1, 1 << S)
    w1, b1 = [int(v) * sc for v in ex.w1], [int(v) * sc for v in ex.b1]
    mids = [([[int(v) * sc for v in row] for row in W], [int(v) * sc for v in b]) for W, b in ex.mids]
    wl = [[int(v) * sc for v in row] for row in ex.wl]
    m0, m1, E = G.moments_as_integers(M, exps)
    out = dict(w_first=[Fraction(0)] * H, b_first=[Fraction(0)] * H, w_last=[[Fraction(0)] * H for _ in range(C)],
               b_last=[Fraction(0)] * C, w_mid=[[[Fraction(0)] * H for _ in range(H)] for _ in range(L - 2)],
               b_mid=[[Fraction(0)] * H for _ in range(L - 2)])
    for t in range(len(A)):
        M0, M1 = [Fraction(int(v), 1 << E) for v in m0[t]], [Fraction(int(v), 1 << E) for v in m1[t]]
        if not any(M0) and not any(M1):
            continue
        a, xi = G.piece_points(A, t)
        D = [[bool(v > 0) for v in z] for z in ex.preacts_direct(xi)[:-1]]
        a = Fraction(a)
        ha = [[(w1[i] * a + b1[i]) if D[0][i] else Fraction(0) for i in range(H)]]
        hp = [[w1[i] if D[0][i] else Fraction(0) for i in range(H)]]
        for l, (W, b) in enumerate(mids, start=1):
            ha.append([(sum(W[j][i] * ha[-1][i] for i in range(H)) + b[j]) if D[l][j] else Fraction(0) for j in range(H)])
            hp.append([sum(W[j][i] * hp[-1][i] for i in range(H)) if D[l][j] else Fraction(0) for j in range(H)])
        top_a, top_p = ha[-1], hp[-1]
        for c in range(C):
            out["b_last"][c] += M0[c]
            for j in range(H):
                out["w_last"][c][j] += M0[c] * top_a[j] + M1[c] * top_p[j]
        e0 = [sum(wl[c][j] * M0[c] for c in range(C)) if D[-1][j] else Fraction(0) for j in range(H)]
        e1 = [sum(wl[c][j] * M1[c] for c in range(C)) if D[-1][j] else Fraction(0) for j in range(H)]
        for l in range(L - 3, -1, -1):
            W = mids[l][0]
            for j in range(H):
                out["b_mid"][l][j] += e0[j]
                for i in range(H):
                    out["w_mid"][l][j][i] += e0[j] * ha[l][i] + e1[j] * hp[l][i]
            e0 = [sum(W[j][i] * e0[j] for j in range(H)) if D[l][i] else Fraction(0) for i in range(H)]
            e1 = [sum(W[j][i] * e1[j] for j in range(H)) if D[l][i] else Fraction(0) for i in range(H)]
        for i in range(H):
            out["w_first"][i] += e0[i] * a + e1[i]
            out["b_first"][i] += e0[i]
    return out


@pytest.mark.parametrize("name", ["L2-H5-C4", "L3-sweep-H3-C4", "L3-sweep-H5-C1", "L4-H3-C1", "point-sweep", "point-L4",
                                  "m0-zero-sweep", "L3-dead", "L3-sweep-float-moments", "integer-L4-e0", "L3-no-bias"])
def test_reference_equals_a_brute_force_pass(name):
    case = GC.case(name)
    for k, (ex, A, ref) in enumerate(zip(case.exs, case.anchors, G.reference(case))):
        want = _brute_force(ex, A, case.feature_moments(k), case.exps)
        for nm in G.NAMES:
            got = ref.grads[nm]
            flat = np.array(want[nm], dtype=object).reshape(-1) if len(want[nm]) else np.zeros(0, object)
            assert got.size == flat.size, (nm, got.shape)
            assert all(x == y for x, y in zip(got.reshape(-1), flat)), (name, k, nm)


def _autograd(case, k):
    """``G`` written out in torch float64 (masks at ``xi`` frozen, value and slope at the anchor) and differentiated."""
    w1, b1, mids, wl = [q if isinstance(q, list) else torch.tensor(q, dtype=torch.float64) for q in G.weights_f64(case.p, k)]
    mids = [(torch.tensor(W, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)) for W, b in mids]
    bl = torch.zeros(case.p.C, dtype=torch.float64)
    leaves = [w1, b1] + [q for Wb in mids for q in Wb] + [wl, bl]
    for q in leaves:
        q.requires_grad_(True)
    A = case.anchors[k]
    M = torch.tensor(G.moments_f64(case.feature_moments(k), case.exps))
    obj = torch.zeros((), dtype=torch.float64)
    for t in range(len(A)):
        if not bool((M[t] != 0).any()):
            continue
        a, xi = G.piece_points(A, t)
        with torch.no_grad():
            z = w1 * xi + b1
            D = [z > 0]
            for W, b in mids:
                z = W @ torch.relu(z) + b
                D.append(z > 0)
        ha, hp = D[0] * (w1 * a + b1), D[0] * w1
        for l, (W, b) in enumerate(mids, start=1):
            ha, hp = D[l] * (W @ ha + b), D[l] * (W @ hp)
        obj = obj + M[t, 0] @ (wl @ ha + bl) + M[t, 1] @ (wl @ hp)
    if not obj.requires_grad:
        return None
    g = torch.autograd.grad(obj, leaves, allow_unused=True)
    g = [torch.zeros_like(q) if x is None else x for x, q in zip(g, leaves)]
    n = len(mids)
    return dict(w_first=g[0].numpy(), b_first=g[1].numpy(), w_mid=np.stack([g[2 + 2 * l].numpy() for l in range(n)]) if n else None,
                b_mid=np.stack([g[3 + 2 * l].numpy() for l in range(n)]) if n else None, w_last=g[-2].numpy(), b_last=g[-1].numpy())


@pytest.mark.parametrize("name", ["L2-H5-C4", "L3-sweep-H5-C1", "L3-piece2-H8-C8", "L4-H8-C8", "L4-H3-C1", "L3-range", "point-L4"])
def test_reference_equals_float64_autograd_of_the_objective(name):
    """At float64 accuracy: ``gamma64_k Mag`` with the per-piece count of one group, doubled (no fma), plus ``H`` for the matmuls'
    own order — no float32 term."""
    case = GC.case(name)
    p = case.p
    for k, ref in enumerate(G.reference(case)):
        got = _autograd(case, k)
        if got is None:
            continue
        kk = 2 * G.k_piece(p.L, p.H, p.C, ref.nl, 1) + 2 * p.H + p.C
        g64 = G.gamma(kk, G.U64)
        for nm, a in got.items():
            if a is None:
                continue
            for gv, t, m in zip(a.reshape(-1), ref.grads[nm].reshape(-1), ref.mag[nm].reshape(-1)):
                assert abs(Fraction(float(gv)) - t) <= g64 * m, (name, k, nm, float(gv), float(t))


# ---- the torch route (two probe points per piece) held to the same truth ---------------------------------------------------------------
def _torch_route(case):
    from gnan_amd import pwl
    from gnan_amd.functional import StackedMLP, _fmlp_eager
    p = case.p
    T = int(case.off[-1])
    t = pwl.PwlTables(torch.from_numpy(case.off), torch.from_numpy(np.concatenate(case.anchors)), torch.zeros(T, p.C),
                      torch.zeros(T, p.C), case.max_pieces, 1, case.max_pieces)
    M = torch.from_numpy(np.concatenate([G.moments_f64(case.feature_moments(k), case.exps) for k in range(p.F)]))
    present = [q is not None for q in p[:6]]
    leaves = [q.clone().requires_grad_(True) for q in p[:6] if q is not None]
    it = iter(leaves)
    st = StackedMLP(*[next(it) if pr else None for pr in present], *p[6:])
    got = pwl.parameter_grads_from_moments(
        st, t, M, lambda U, q: _fmlp_eager(U, StackedMLP(*[None if a is None else a.double() for a in q[:6]], *q[6:]), False))
    it = iter(got)
    return [next(it) if pr else None for pr in present]


def _probe_magnitudes(case, k):
    """``Mag`` of the two-probe form: the pass of magnitudes over the ``2 nl`` probe points ``u1 = a + h``, ``u2 = a + 2 h`` with the
    weights ``|c1| <= 2 |M0| + |M1| / |h|``, ``|c2| <= |M0| + |M1| / |h|`` as value moments (float64, rounded up by 2^-40) — the
    division by a third of the piece width is where this route is amplified against the kernels'."""
    from gnan_amd import pwl
    A = case.anchors[k]
    t = pwl.PwlTables(torch.tensor([0, len(A)], dtype=torch.int32), torch.from_numpy(A), None, None, len(A), 1, len(A))
    u1, u2, h = [q.numpy() for q in pwl.piece_probe_points(t)]
    M = np.abs(G.moments_f64(case.feature_moments(k), case.exps))
    live = [t_ for t_ in range(len(A)) if M[t_].any()]
    rows, pts = [], []
    for t_ in live:
        c2 = (M[t_, 0] + M[t_, 1] / abs(h[t_])) * (1 + 2.0 ** -40)
        rows += [np.stack([c2 + M[t_, 0], 0 * c2]), np.stack([c2, 0 * c2])]
        pts += [(float(u1[t_]), 0.0), (float(u2[t_]), 0.0)]
    if not rows:
        return None
    m0, m1, E = G.moments_as_integers(np.stack(rows), None)
    return G._pass(case.exs[k], A, m0, m1, E, True, points=pts)[0]


@pytest.mark.parametrize("name", [n for n in GC.ALL if "wrapper" not in n and "H127" not in n and "H128" not in n])
def test_torch_route_is_inside_its_own_bound(name):
    """``pwl.parameter_grads_from_moments`` on the CPU (float64 inside, the gradients returned in the leaves' float32): the bound of
    :func:`grads_ref.check` with ``MagProbe`` in place of ``Mag`` and
    ``k = 8 + 2 (L - 1) (H + 2) + C + 4 max_pieces``: the weights ``c`` (a division, two subtractions), the probe points (an
    addition each; their rounding moves ``f`` by at most ``2^-53`` of its magnitude), ``H + 2`` per layer forward and backward in
    whatever order the matmuls take, ``C`` for the objective and ``2 max_pieces`` rows summed twice."""
    case = GC.case(name)
    p = case.p
    got = G.split(case, _torch_route(case))
    kk = 8 + 2 * (p.L - 1) * (p.H + 2) + p.C + 4 * case.max_pieces
    for k, ref in enumerate(G.reference(case)):
        mag = _probe_magnitudes(case, k)
        if mag is None:
            mag = {nm: np.vectorize(lambda t: Fraction(0), otypes=[object])(a) if a.size else a for nm, a in ref.grads.items()}
        ratio, where, _ = G.check(got[k], ref._replace(mag=mag), kk)
        assert ratio <= 1.0, (name, k, where, ratio)


# ---- planted errors, each failing a named case ---------------------------------------------------------------------------------------------
PLANTS = [
    ("live_m0", "m0-zero-sweep"), ("live_m0", "m0-zero-piece4"), ("live_m0", "m0-zero-L2"), ("live_m0", "m0-zero-L4"),
    ("ge2", "point-sweep"), ("ge2", "point-piece4"), ("ge3", "point-L4"),
    ("prefix_after", "switches-sweep"), ("order_desc", "switches-sweep"), ("starts_on_diff", "switches-sweep"),
    ("moment_f32", "integer-sweep-e0"), ("moment_f32", "integer-piece2-e0"), ("moment_f32", "integer-L2-e0"),
    ("moment_f32", "integer-L4-e0"), ("skip_last_group", "L3-piece4-tails"), ("skip_last_group", "L3-piece2-H8-C8"),
    ("skip_last_group", "L4-tails"),
]


@pytest.mark.parametrize("plant,name", PLANTS)
def test_planted_error_fails_its_case(plant, name):
    case = GC.case(name)
    assert G.hold(case, G.emulate(case), k_scale=2)[0] <= 1.0
    ratio, where, _ = G.hold(case, G.emulate(case, plant=plant), k_scale=2)
    assert ratio > 1.0, (plant, name, ratio)


def test_old_rule_passes_what_the_bounds_refuse():
    """The older tests' rule (1e-5 of the largest entry over all features) is blind to (a) the live list built from M0 alone on
    a table where one live piece has M0 = 0 and a small M1, (b) a wrong gradient confined to a feature whose last layer is 2^-40
    of the others (here: its hidden layers' gradients off by a thousandth); the per-element bound refuses both."""
    # (a) M1 of the M0 = 0 piece is small beside the other pieces' moments: below 1e-5 of the largest entry, far above the bound
    case = GC.case("m0-zero-sweep")
    M = case.M.copy()
    t = [i for i in range(len(M)) if not M[i, 0].any() and M[i, 1].any()][0]
    M[t, 1] = np.sign(M[t, 1]) * (1 << 26) + 1
    small = case._replace(name="m0-zero-sweep-small-m1", M=M)
    assert G.hold(small, G.emulate(small), k_scale=2)[0] <= 1.0
    bad = G.emulate(small, plant="live_m0")
    assert _old_rule(small, bad)
    assert G.hold(small, bad, k_scale=2)[0] > 1.0
    # (b)
    for name in ("small-feature-sweep", "small-feature-L4"):
        case = GC.case(name)
        good = G.emulate(case)
        bad = [dict(g) for g in good]
        bad[1] = {nm: (v * np.float32(1.001)).astype(np.float32) for nm, v in good[1].items() if nm in ("w_first", "b_first", "w_mid", "b_mid")}
        bad[1].update({nm: v for nm, v in good[1].items() if nm not in bad[1]})
        assert _old_rule(case, bad)
        assert G.hold(case, good, k_scale=2)[0] <= 1.0 < G.hold(case, bad, k_scale=2)[0]
