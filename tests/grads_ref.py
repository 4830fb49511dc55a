"""Exact reference of the table path's parameter gradients (``gnan_fpwl_param_grads``, csrc/fpwl_grad.hip) and the bound every
element of the kernels' result is held to — TEST INFRASTRUCTURE ONLY (numpy and Python integers; no GPU, no product code).

**Contract.**  For feature ``k`` and every piece ``t`` with a non-zero moment (any of its ``2 C``): anchor ``a_t``, point ``xi_t`` as
csrc/piece_points.hpp takes it (``a - 1`` on the first piece, ``a + 1`` on the last, ``a`` on a piece at most one float32 step
wide, else the float64 midpoint), masks ``D_l = [z_l(xi_t) > 0]`` (strict), and

    G = sum_t <M0_t, f_D(a_t)> + <M1_t, s_D>

with ``f_D`` / ``s_D`` value and slope of the network frozen at the masks.  The truth is ``dG / d theta`` for the six stacked
parameter tensors by the reverse passes written at the head of fpwl_grad.hip, L = 2, 3, 4.

**Exactness.**  Weights and anchors are float32, ``xi`` a float64, the moments integers times a power of two (or float32): all
dyadic rationals.  :func:`exact_grads` runs the whole pass in Python integers (:class:`tables_ref.ExactFeature` holds the
weights as integers times ``2^S``) and returns ``fractions.Fraction``.  There is no float64 truth.

**Bound** per element (:func:`check`)::

    |got - t| <= u32 |t| + (1 + u32) gamma64_k Mag + 2^-149             u32 = 2^-24: the one rounding at the store

``Mag`` is the same reverse pass with every weight, bias, anchor and moment replaced by its magnitude and every mask set to 1,
summed over the live pieces (unmasked: the sweep keeps layer 2's form by adding and subtracting unit contributions and forms
``total - prefix``, so its error scales with all units and all pieces).  ``k`` counts the float64 roundings on the longest path of
one term, from the code (``q = ceil(H / 4)``, ``cq = ceil(C / 4)``, ``nl`` live pieces of the feature):

    per-piece kernels (fpwl_grad2_kernel: NG = 1; fpwl_grad3_kernel<NG, .>; fpwl_grad4_kernel<2, .>)           :func:`k_piece`
        1                         the moment's conversion (an int64 above 2^53; the power-of-two scale is exact)
      + 1 + (L - 2) (q + 3)       forward: the first layer's fma; per further layer q fmas, two butterfly adds, the bias
      + cq + 2 + (L - 2) (q + 2)  backward: the last layer's chain and butterfly; per further layer q fmas and the butterfly
      + 2 ceil(nl / NG) + NG      two fmas per live piece of a group, the NG - 1 group adds, fma(q0, a, q1)
    sweep (fpwl_grad3_sweep_kernel)                                                                            :func:`k_sweep`
        1                         conversion
      + q + 3 + H + 1             the form left of all switches (q fmas, butterfly, bias), one add per switch, fma(Aj, a, Bj)
      + 4                         the four-channel chain of e0 / e1
      + 2 nl                      RG += fma(e0, a, e1) / dW3's two fmas, per live piece
      + 1 + 1                     total - prefix; b * se
      + max(2, q + 2)             fma(w, sg, .)  /  the chain and butterfly of dw1, db1

Through the Python wrapper (C > 64: chunks of 64 channels, the hidden layers' gradients added in float32) the hidden layers get
``gamma32_(chunks - 1) Mag`` on top: each chunk's store is at most ``u32`` of its own magnitude, every intermediate add at most
``u32`` of the magnitudes so far, and the last add is the ``u32 |t|`` already counted; ``k`` is then the largest count of the
chunks' kernels (a last chunk of at most four channels at L = 3 goes to the sweep).  A zero bound demands an exact zero.

**Decided masks** (a condition on the CASE, not a tolerance): :func:`exact_grads` counts as *undecided* every hidden unit of
layer >= 2 on a live piece whose exact ``|z_l(xi)|`` is non-zero but not above ``gamma64_kz mag(z_l)`` (``mag``: all units on,
magnitudes; ``kz`` the forward count of the route, the sweep's included), and every exact zero whose float64 evaluation is not
provably exact in any order (all terms — of every unit, on or off — integer multiples of one quantum with a sum of magnitudes
below ``2^53`` quanta, and the layer below likewise).  The first layer is one fma: its sign is always the exact one.  The
committed cases have none.

**Kink-free pieces.**  The hidden activation patterns at ``xi`` and at the first and last float32 value of a live piece are
asserted equal (plain integer dot products): the kernels (masks at ``xi``), the torch route (probes at thirds) and this
reference then share one contract.

**Emulations** in numpy float64 of the two algorithms in the kernels' own order — :func:`emulate_piece` (groups of NG, in-order
group add) and :func:`emulate_sweep` (switch positions, order by (bnd, index), running (Aj, Bj), prefixes, total - prefix) —
with ``plant=`` for deliberate errors.  numpy has no fma: a multiply-add rounds twice, so they are held to ``2 k``.
"""
from fractions import Fraction
from typing import NamedTuple, Optional

import numpy as np

import tables_ref as R

U32 = Fraction(1, 2 ** 24)
U64 = Fraction(1, 2 ** 53)
TINY = Fraction(1, 2 ** 149)
NAMES = ("w_first", "b_first", "w_mid", "b_mid", "w_last", "b_last")
SWEEP_PIECES = 1024


def gamma(k, u):
    return Fraction(k) * u / (1 - k * u)


def k_piece(L, H, C, nl, NG):
    q, cq = -(-H // 4), -(-C // 4)
    return 1 + (1 + (L - 2) * (q + 3)) + (cq + 2 + (L - 2) * (q + 2)) + (2 * -(-nl // NG) + NG)


def k_sweep(H, C, nl):
    q = -(-H // 4)
    return 1 + (q + 3 + H + 1) + 4 + 2 * nl + 2 + max(2, q + 2)


def kz_of(route, L, H):
    q = -(-H // 4)
    return max(1 + (L - 2) * (q + 3), (q + 3 + H + 1) if route == "sweep" else 0)


def route_of(L, C, max_pieces):
    """``(name, NG)`` of the kernel ``gnan_fpwl_param_grads`` launches."""
    if L == 2:
        return "grad2", 1
    if L == 4:
        return "grad4", 2
    if C <= 4 and max_pieces <= SWEEP_PIECES:
        return "sweep", 1
    return "grad3", 4 if C <= 4 else 2


class Weights(R.ExactFeature):
    """The integer weights only (no kink search): for tables that come from a builder."""

    def _find_kinks(self):
        self.kinks = None


def features_of(p, kinks=True):
    if kinks:
        return R.features_of(p)
    out = []
    for k in range(p.F):
        mids = [(p.w_mid[l][k].numpy(), None if p.b_mid is None else p.b_mid[l][k].numpy()) for l in range(p.L - 2)]
        out.append(Weights(p.w_first[k].numpy(), None if p.b_first is None else p.b_first[k].numpy(), mids,
                           p.w_last[k].numpy(), None if p.b_last is None else p.b_last[k].numpy()))
    return out


def table_anchors(ex, extra=()):
    """Anchor array ``[P]`` of a table that refines the exact partition: every kink rounded up, the point pieces, and the
    superfluous anchors ``extra``; piece 0 is anchored at the first breakpoint.  No breakpoint: one piece anchored at 0."""
    bps, _ = ex.expected_anchors()
    every = sorted(set(bps.tolist()) | {float(np.float32(v)) for v in extra})
    if not every:
        return np.zeros(1, np.float32)
    return np.array([every[0]] + every, dtype=np.float32)


def piece_points(A, li):
    """csrc/piece_points.hpp in numpy: ``(a, xi)`` as Python floats (float64)."""
    P, a = len(A), float(A[li])
    if li == 0:
        return a, a - 1.0
    if li == P - 1:
        return a, a + 1.0
    if A[li + 1] <= np.nextafter(A[li], np.float32(np.inf)):
        return a, a
    return a, 0.5 * (a + float(A[li + 1]))


def piece_ends(A, li):
    """First and last float32 value of piece ``li`` (a ray: the end and a point one beyond the kernel's)."""
    P = len(A)
    if P == 1:
        return [float(A[0]) - 2.0, float(A[0]) + 2.0]
    if li == 0:
        return [float(A[0]) - 2.0, float(R.down(A[1]))]
    if li == P - 1:
        return [float(A[li]), float(A[li]) + 2.0]
    return [float(A[li]), float(max(R.down(A[li + 1]), A[li]))]


def _ints(a):
    out = np.empty(np.shape(a), dtype=object)
    flat = out.reshape(-1)
    for i, v in enumerate(np.asarray(a).reshape(-1)):
        flat[i] = int(v)
    return out


def moments_as_integers(M, exps):
    """``(m0 [P, C], m1 [P, C], E)`` with ``M0 = m0 / 2^E``, ``M1 = m1 / 2^E``, Python integers.  ``M [P, 2, C]`` is int64 with
    ``exps = (e0, e1)`` (the scales are ``2^e0``, ``2^e1``) or float32 with ``exps = None``."""
    if exps is None:
        flat = [R._as_ratio(v) for v in np.asarray(M, np.float64).reshape(-1)]
        E = max([e for _, e in flat] + [0])
        m = np.empty(len(flat), dtype=object)
        m[:] = [n << (E - e) for n, e in flat]
        m = m.reshape(M.shape)
        return m[:, 0], m[:, 1], E
    e0, e1 = exps
    E = max(e0, e1, 0)
    m = _ints(M)
    return m[:, 0] * (1 << (E - e0)), m[:, 1] * (1 << (E - e1)), E


def _span_ok(terms):
    nz = [abs(int(t)) for t in terms if t != 0]
    if not nz:
        return True
    g = min((t & -t).bit_length() - 1 for t in nz)
    return (sum(nz) >> g) < 2 ** 53


def _zero(shape):
    out = np.empty(shape, dtype=object)
    out.reshape(-1)[:] = 0
    return out


class Exact(NamedTuple):
    grads: dict            # name -> object array of Fraction (w_mid [L - 2, H, H], b_mid [L - 2, H])
    mag: dict              # the same pass of magnitudes, all masks on
    nl: int
    undecided: int
    point_zeros: int       # exact zeros of a hidden unit of layer >= 2 on a live piece (all provably exact, or counted above)


def _pass(ex, A, m0, m1, E, magnitudes, kz=0, route="grad3", points=None):
    """The reverse pass of one feature over its live pieces in integers -> (dict of Fraction arrays, nl, undecided, zeros).
    ``points = [(a, xi)]``: row ``t`` of the moments belongs to that anchor and point instead of piece ``t`` of ``A`` (magnitudes
    of the two-probe form)."""
    H, C, L, S = ex.H, ex.C, ex.L, ex.S
    fix = (lambda v: abs(v)) if magnitudes else (lambda v: v)
    w1, b1, wl = fix(ex.w1), fix(ex.b1), fix(ex.wl)
    mids = [(fix(W), fix(b)) for W, b in ex.mids]
    live = [t for t in range(len(m0)) if any(v != 0 for v in m0[t]) or any(v != 0 for v in m1[t])]
    pts = [piece_points(A, t) if points is None else points[t] for t in live]
    q = max([R._as_ratio(v)[1] for pt in pts for v in pt] + [0])
    Q = 1 << q

    def scaled(v):
        n, e = R._as_ratio(v)
        return n << (q - e)

    g = dict(w_first=_zero(H), b_first=_zero(H), w_mid=_zero((L - 2, H, H)), b_mid=_zero((L - 2, H)), w_last=_zero((C, H)),
             b_last=_zero(C))
    undecided = zeros = 0
    gz = gamma(kz, U64) if kz else None
    for t, (a, xi) in zip(live, pts):
        An, Xn = scaled(a), scaled(xi)
        M0, M1 = fix(m0[t]), fix(m1[t])
        if magnitudes:
            An, Xn = abs(An), abs(Xn)
        # forward at xi: the masks
        z = w1 * Xn + b1 * Q
        D = [np.ones(H, bool) if magnitudes else (z > 0)]
        zs = [z]
        h = np.where(D[0], z, 0)
        for l, (W, b) in enumerate(mids, start=1):
            z = W.dot(h) + b * (Q << (S * l))
            D.append(np.ones(H, bool) if magnitudes else (z > 0))
            zs.append(z)
            h = np.where(D[l], z, 0)
        if not magnitudes:
            # kink-free: the same patterns at both float32 ends of the piece
            for x in piece_ends(A, t):
                for l, zz in enumerate(ex.preacts_direct(x)[:-1]):
                    assert bool(((zz > 0) == D[l]).all()), f"piece {t}: a unit of hidden layer {l + 1} switches inside"
            if gz is not None and L > 2:
                # decided masks of the layers >= 2
                aw1, ab1, aX = abs(ex.w1), abs(ex.b1), abs(Xn)
                mz = aw1 * aX + ab1 * Q
                exact_below = all(_span_ok([int(v)]) for v in zs[0])
                for l, (W, b) in enumerate(ex.mids, start=1):
                    mz = abs(W).dot(mz) + abs(b) * (Q << (S * l))
                    hprev = np.where(D[l - 1], zs[l - 1], 0)
                    ok = exact_below
                    for j in range(H):
                        terms = list(W[j] * hprev) + [b[j] * (Q << (S * l))]
                        if l == 1 and route == "sweep":
                            # the sweep adds and removes every unit: the form's coefficients on their own, all units (at
                            # xi = 0 the slope coefficient does not enter: fma(Aj, 0, Bj) = Bj)
                            ok_j = (Xn == 0 or _span_ok(list(W[j] * ex.w1))) and _span_ok(list(W[j] * ex.b1) + [b[j] << S]) \
                                and _span_ok(terms + list(W[j] * zs[0]))
                        else:
                            ok_j = _span_ok(terms)
                        ok = ok and ok_j
                        if zs[l][j] == 0:
                            zeros += 1
                            if not (exact_below and ok_j):
                                undecided += 1
                        elif Fraction(abs(int(zs[l][j]))) <= gz * int(mz[j]):
                            undecided += 1
                    exact_below = ok
        # value and (Q times the) slope of the hidden layers at the anchor
        ha, hp = np.where(D[0], w1 * An + b1 * Q, 0), np.where(D[0], w1 * Q, 0)
        HA, HP = [ha], [hp]
        for l, (W, b) in enumerate(mids, start=1):
            ha, hp = np.where(D[l], W.dot(ha) + b * (Q << (S * l)), 0), np.where(D[l], W.dot(hp), 0)
            HA.append(ha)
            HP.append(hp)
        # backward
        g["w_last"] += np.multiply.outer(M0, HA[-1]) + np.multiply.outer(M1, HP[-1])
        g["b_last"] += M0
        e0, e1 = np.where(D[-1], wl.T.dot(M0), 0), np.where(D[-1], wl.T.dot(M1), 0)
        for l in range(L - 3, -1, -1):
            W = mids[l][0]
            g["w_mid"][l] += np.multiply.outer(e0, HA[l]) + np.multiply.outer(e1, HP[l])
            g["b_mid"][l] += e0
            e0, e1 = np.where(D[l], W.T.dot(e0), 0), np.where(D[l], W.T.dot(e1), 0)
        g["w_first"] += e0 * An + e1 * Q
        g["b_first"] += e0
    top = E + (L - 1) * S
    den = dict(w_first=top + q, b_first=top, w_last=top + q, b_last=E)
    out = {}
    for name in ("w_first", "b_first", "w_last", "b_last"):
        out[name] = _fractions(g[name], den[name])
    out["w_mid"] = _fractions(g["w_mid"], top + q)
    out["b_mid"] = np.stack([_fractions(g["b_mid"][l], E + (L - 2 - l) * S) for l in range(L - 2)]) if L > 2 else _zero((0, H))
    return out, len(live), undecided, zeros


def _fractions(a, e):
    out = np.empty(a.shape, dtype=object)
    d = 1 << e
    flat = out.reshape(-1)
    for i, v in enumerate(a.reshape(-1)):
        flat[i] = Fraction(int(v), d)
    return out


def exact_grads(ex, A, M, exps, route="grad3") -> Exact:
    """Truth and magnitudes of one feature: ``A [P]`` float32 anchors, ``M [P, 2, C]`` its moments (see
    :func:`moments_as_integers`)."""
    m0, m1, E = moments_as_integers(M, exps)
    grads, nl, und, zeros = _pass(ex, A, m0, m1, E, False, kz_of(route, ex.L, ex.H), route)
    mag = _pass(ex, A, m0, m1, E, True)[0]
    return Exact(grads, mag, nl, und, zeros)


def k_of(route, NG, L, H, C, nl):
    return k_sweep(H, C, nl) if route == "sweep" else k_piece(L, H, C, nl, NG)


def check(got, exact: Exact, k, chunks=1, present=None):
    """Hold one feature's result ``got`` (name -> float array, shaped as ``exact.grads``) to the bound.  Returns ``(worst ratio,
    name of its tensor, number of zero-bound elements)``; a zero bound demands an exact zero (ratio inf otherwise)."""
    g64 = gamma(k, U64)
    worst, where, zero_bounds = 0.0, None, 0
    for name in NAMES:
        if name not in got or got[name] is None:
            continue
        extra = gamma(chunks - 1, U32) if (chunks > 1 and name not in ("w_last", "b_last")) else 0
        G = np.asarray(got[name], dtype=np.float64).reshape(-1)
        T, Mg = exact.grads[name].reshape(-1), exact.mag[name].reshape(-1)
        assert len(G) == len(T), (name, len(G), len(T))
        for gv, t, m in zip(G, T, Mg):
            if not np.isfinite(gv):
                return float("inf"), name, zero_bounds
            err = abs(Fraction(float(gv)) - t)
            if m == 0:
                zero_bounds += 1
                r = 0.0 if err == 0 else float("inf")
            else:
                bound = U32 * abs(t) + (1 + U32) * g64 * m + extra * m + TINY
                r = float(err / bound)
            if r > worst:
                worst, where = r, name
    return worst, where, zero_bounds


# =============================================================================
# emulations in the kernels' own order (numpy float64, no fma)
# =============================================================================
def _f64(ex_arrays):
    return [None if a is None else np.asarray(a, np.float64) for a in ex_arrays]


def moments_f64(M, exps, plant=None):
    """``piece_moment``: the int64 converted to float64 (round to nearest) times the exact power of two; float32 widened."""
    if exps is None:
        out = np.asarray(M, np.float32).astype(np.float64)
    else:
        v = np.asarray(M, np.int64).astype(np.float64)
        if plant == "moment_f32":
            v = np.asarray(M, np.int64).astype(np.float32).astype(np.float64)
        out = np.stack([np.ldexp(v[:, 0], -exps[0]), np.ldexp(v[:, 1], -exps[1])], 1)
    return out


def _live(M, plant):
    raw = np.asarray(M)
    nz = (raw[:, 0] != 0).any(1) if plant == "live_m0" else (raw != 0).any((1, 2))
    return [int(t) for t in np.nonzero(nz)[0]]


def _chain_blocks(W, v):
    """``out[j] = sum_i W[j, i] v[i]``: four lanes take consecutive blocks of ``ceil(n / 4)`` in order, then the butterfly."""
    n = W.shape[1]
    BI = -(-n // 4)
    s = np.zeros((4, W.shape[0]))
    for ib in range(4):
        for r in range(BI):
            i = ib * BI + r
            if i < n:
                s[ib] = W[:, i] * v[i] + s[ib]
    return (s[0] + s[1]) + (s[2] + s[3])


def _chain_strided(W, v):
    """``out[j] = sum_c W[j, c] v[c]`` with lane ``ib`` taking ``c = ib, ib + 4, ...``."""
    n = W.shape[1]
    s = np.zeros((4, W.shape[0]))
    for ib in range(4):
        for c in range(ib, n, 4):
            s[ib] = W[:, c] * v[c] + s[ib]
    return (s[0] + s[1]) + (s[2] + s[3])


def emulate_piece(w, A, M, exps, NG, plant=None):
    """``fpwl_grad2_kernel`` (NG = 1), ``fpwl_grad3_kernel<NG>``, ``fpwl_grad4_kernel<NG>`` on one feature.  ``w = (w1 [H], b1, mids
    [(W, b)], wl [C, H])`` float arrays.  Plants: ``live_m0``, ``ge2``, ``ge3``, ``moment_f32``, ``skip_last_group``."""
    w1, b1, mids, wl = w
    H, C, n_mid = len(w1), len(wl), len(mids)
    Mv = moments_f64(M, exps, plant)
    live = _live(M, plant)

    def fresh():
        return dict(w_first=np.zeros(H), b_first=np.zeros(H), w_mid=np.zeros((n_mid, H, H)), b_mid=np.zeros((n_mid, H)),
                    w_last=np.zeros((C, H)), b_last=np.zeros(C))
    groups = [fresh() for _ in range(NG)]
    for at, t in enumerate(live):
        acc = groups[at % NG]
        a, xi = piece_points(A, t)
        M0, M1 = Mv[t, 0], Mv[t, 1]
        z = w1 * xi + b1
        on = [z > 0]
        hi, ha, hp = np.where(on[0], z, 0.0), np.where(on[0], w1 * a + b1, 0.0), np.where(on[0], w1, 0.0)
        HA, HP = [ha], [hp]
        for l, (W, b) in enumerate(mids):
            si, sa, sp = _chain_blocks(W, hi), _chain_blocks(W, ha), _chain_blocks(W, hp)
            o = (si + b >= 0) if plant == ("ge2", "ge3")[l] else (si + b > 0)
            on.append(o)
            hi, ha, hp = np.where(o, si + b, 0.0), np.where(o, sa + b, 0.0), np.where(o, sp, 0.0)
            HA.append(ha)
            HP.append(hp)
        acc["w_last"] = np.outer(M0, HA[-1]) + (np.outer(M1, HP[-1]) + acc["w_last"])
        acc["b_last"] = acc["b_last"] + M0
        e0, e1 = np.where(on[-1], _chain_strided(wl.T, M0), 0.0), np.where(on[-1], _chain_strided(wl.T, M1), 0.0)
        for l in range(n_mid - 1, -1, -1):
            W = mids[l][0]
            acc["w_mid"][l] = np.outer(e0, HA[l]) + (np.outer(e1, HP[l]) + acc["w_mid"][l])
            acc["b_mid"][l] = acc["b_mid"][l] + e0
            e0, e1 = np.where(on[l], _chain_blocks(W.T, e0), 0.0), np.where(on[l], _chain_blocks(W.T, e1), 0.0)
        acc["w_first"] = acc["w_first"] + (e0 * a + e1)
        acc["b_first"] = acc["b_first"] + e0
    out = groups[0]
    for gi in range(1, NG - 1 if (plant == "skip_last_group" and NG > 1) else NG):
        for name in out:
            out[name] = out[name] + groups[gi][name]
    return out


def emulate_sweep(w, A, M, exps, plant=None):
    """``fpwl_grad3_sweep_kernel`` on one feature (L = 3, C <= 4).  Plants: ``live_m0``, ``ge2``, ``moment_f32``,
    ``prefix_after`` (the switches of a piece handled behind its accumulation), ``order_desc`` (units of equal ``bnd`` ordered
    by index descending where the prefixes are stored and the factors read, while the form's W2 entry is still read in the old
    order), ``starts_on_diff`` (``total - prefix`` for a unit that starts on as well)."""
    w1, b1, mids, wl = w
    (W2, b2), = mids
    H, C = len(w1), len(wl)
    Mv = moments_f64(M, exps, plant)
    live = _live(M, plant)
    nl = len(live)
    pts = [piece_points(A, t) for t in live]
    an, xs = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    starts_on = (w1 < 0) | ((w1 == 0) & (b1 > 0))
    on = np.array([int(((w1[i] * xs + b1[i]) > 0).sum()) for i in range(H)], dtype=int) if nl else np.zeros(H, int)
    bnd = np.where(starts_on, on, nl - on)
    order = sorted(range(H), key=lambda i: (bnd[i], i))
    store = sorted(range(H), key=lambda i: (bnd[i], -i)) if plant == "order_desc" else order
    Aj = _chain_blocks(W2 * starts_on[None, :], w1)
    Bj = _chain_blocks(W2 * starts_on[None, :], b1) + b2
    sw_w = np.where(w1 > 0, w1, -w1)
    sw_b = np.where(w1 > 0, b1, -b1)
    PG, PE = np.zeros((H, H)), np.zeros((H, H))
    RG, RE, db2 = np.zeros(H), np.zeros(H), np.zeros(H)
    dW3, db3 = np.zeros((C, H)), np.zeros(C)
    cursor = 0

    def switches(g):
        nonlocal cursor, Aj, Bj
        while cursor < H and bnd[order[cursor]] == g:
            i, s = order[cursor], store[cursor]
            PG[:, s], PE[:, s] = RG, RE
            Aj = Aj + W2[:, i] * sw_w[s]
            Bj = Bj + W2[:, i] * sw_b[s]
            cursor += 1
    for g in range(nl):
        if plant != "prefix_after":
            switches(g)
        x, a = xs[g], an[g]
        M0, M1 = Mv[live[g], 0], Mv[live[g], 1]
        z = Aj * x + Bj
        on2 = (z >= 0) if plant == "ge2" else (z > 0)
        h2a, h2p = np.where(on2, Aj * a + Bj, 0.0), np.where(on2, Aj, 0.0)
        p0, p1 = np.zeros(H), np.zeros(H)
        for c in range(C):
            p0 = wl[c] * M0[c] + p0
            p1 = wl[c] * M1[c] + p1
            dW3[c] = M0[c] * h2a + (M1[c] * h2p + dW3[c])
        db3 = db3 + M0
        e0, e1 = np.where(on2, p0, 0.0), np.where(on2, p1, 0.0)
        db2 = db2 + e0
        RG = RG + (e0 * a + e1)
        RE = RE + e0
        if plant == "prefix_after":
            switches(g)
    for c in range(cursor, H):
        PG[:, store[c]], PE[:, store[c]] = RG, RE
    TG, TE = RG, RE
    so = np.zeros(H, bool) if plant == "starts_on_diff" else starts_on
    SG = np.where(so[None, :], PG, TG[:, None] - PG)
    SE = np.where(so[None, :], PE, TE[:, None] - PE)
    dW2 = w1[None, :] * SG + b1[None, :] * SE
    dw1 = np.array([_chain_blocks(W2[:, u][None, :], SG[:, u])[0] for u in range(H)])
    db1 = np.array([_chain_blocks(W2[:, u][None, :], SE[:, u])[0] for u in range(H)])
    return dict(w_first=dw1, b_first=db1, w_mid=dW2[None], b_mid=db2[None], w_last=dW3, b_last=db3)


# =============================================================================
# cases
# =============================================================================
class Case(NamedTuple):
    name: str
    p: object                  # StackedMLP of CPU float32 tensors
    anchors: list              # per feature: float32 [P_k]
    M: np.ndarray              # [T, 2, C] int64 (with exps) or float32 (exps None)
    exps: Optional[tuple]
    max_pieces: int
    exs: list                  # ExactFeature per feature
    exact: bool = False        # every route must return the truth's own bits

    @property
    def off(self):
        return np.concatenate([[0], np.cumsum([len(a) for a in self.anchors])]).astype(np.int32)

    @property
    def route(self):
        return route_of(self.p.L, min(self.p.C, 64), self.max_pieces)

    def feature_moments(self, k):
        o = self.off
        return self.M[o[k]:o[k + 1]]


def weights_f64(p, k):
    H = p.H
    z = np.zeros(H)
    b1 = z if p.b_first is None else p.b_first[k].double().numpy()
    mids = [(p.w_mid[l][k].double().numpy(), z if p.b_mid is None else p.b_mid[l][k].double().numpy()) for l in range(p.L - 2)]
    return p.w_first[k].double().numpy(), b1, mids, p.w_last[k].double().numpy()


def split(case, got):
    """The six tensors of a whole-stack result (None where a bias is absent; torch or numpy) -> per feature dicts shaped as
    :class:`Exact` (an absent bias's gradient is not compared)."""
    arr = [None if g is None else (g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)) for g in got]
    out = []
    for k in range(case.p.F):
        d = {}
        for name, a in zip(NAMES, arr):
            if a is None:
                continue
            d[name] = a[:, k] if name in ("w_mid", "b_mid") else a[k]
        out.append(d)
    return out


def reference(case):
    """Exact truth of every feature, cached on the case name."""
    if case.name not in _REF:
        C = case.p.C
        routes = {route_of(case.p.L, min(64, C - c0), case.max_pieces)[0] for c0 in range(0, C, 64)}
        route = "sweep" if "sweep" in routes else case.route[0]         # (the decided-mask condition of every chunk's kernel)
        _REF[case.name] = [exact_grads(ex, A, case.feature_moments(k), case.exps, route)
                           for k, (ex, A) in enumerate(zip(case.exs, case.anchors))]
    return _REF[case.name]


_REF = {}


def hold(case, per_feature, k_scale=1, chunks=None):
    """Worst ratio of a whole result (list of per-feature dicts) against the truth; asserts nothing.  ``k_scale = 2``: the numpy
    emulations (no fma)."""
    route, NG = case.route
    C = case.p.C
    chunks = (-(-C // 64)) if chunks is None else chunks
    worst, where, zb = 0.0, None, 0
    for k, (got, ex) in enumerate(zip(per_feature, reference(case))):
        # (through the wrapper every chunk of channels is a launch of its own, a last chunk of at most four channels at L = 3
        # goes to the sweep: the largest count of the chunks' kernels)
        widths = {min(64, C - c0) for c0 in range(0, C, 64)}
        kk = k_scale * max(k_of(*route_of(case.p.L, w, case.max_pieces), case.p.L, case.p.H, w, ex.nl) for w in widths)
        r, name, z = check(got, ex, kk, chunks)
        zb += z
        if r > worst:
            worst, where = r, (k, name)
    return worst, where, zb


def emulate(case, plant=None, which=None):
    """The emulation of the kernel the case is routed to (``which``: "sweep" / "piece" to force one), per feature."""
    route, NG = case.route
    out = []
    for k in range(case.p.F):
        w, A, M = weights_f64(case.p, k), case.anchors[k], case.feature_moments(k)
        if (which or route) == "sweep":
            g = emulate_sweep(w, A, M, case.exps, plant)
        else:
            g = emulate_piece(w, A, M, case.exps, NG if which is None else 4, plant)
        with np.errstate(over="ignore"):
            out.append({name: v.astype(np.float32) for name, v in g.items()})        # the one rounding at the store
    return out


def _dy(rng, shape, den=8, lim=8):
    """Small dyadics: integers in [-lim, lim] over ``den``."""
    return rng.integers(-lim, lim + 1, size=shape).astype(np.float64) / den


def switch_net(H, C, kinks, rng, dominant=None, const_on=(), const_off=()):
    """L = 3 feature whose first-layer unit ``i`` is ``relu(s_i (x - kinks[i]))`` with ``s_i = +-1`` from the sign given in
    ``kinks = [(sign, position)]``; units in ``const_on`` / ``const_off`` have ``w1 = 0`` and ``b1 = 1/2`` / ``b1 = 0 or -1/2``; small
    dyadic W2, b2, last layer.  ``dominant = i``: ``W2[:, i]`` times 2^20."""
    w1, b1 = np.zeros(H), np.zeros(H)
    for i, (s, pos) in enumerate(kinks):
        w1[i], b1[i] = s, -s * pos
    for n, i in enumerate(const_on):
        w1[i], b1[i] = 0.0, 0.5
    for n, i in enumerate(const_off):
        w1[i], b1[i] = 0.0, (0.0 if n % 2 == 0 else -0.5)
    W2, b2 = _dy(rng, (H, H)), _dy(rng, H, 16)
    W2[W2 == 0] = 0.125
    if dominant is not None:
        W2[:, dominant] *= 2.0 ** 20
    wl, bl = _dy(rng, (C, H)), _dy(rng, C)
    return dict(w1=w1, b1=b1, mids=[(W2, b2)], wl=wl, bl=bl)


def int_moments(rng, P, C, live, bits=40, both=True):
    M = np.zeros((P, 2, C), dtype=np.int64)
    for t in live:
        M[t] = rng.integers(-(1 << bits), 1 << bits, size=(2, C))
        M[t, 0, 0] |= 1
        if not both:
            M[t, 1] = 0
    return M


def point_pieces(A):
    """Inner pieces at most one float32 step wide: they hold the nodes with ``x == a`` only, so their slope moment is zero."""
    return [t for t in range(1, len(A) - 1) if A[t + 1] <= np.nextafter(A[t], np.float32(np.inf))]


def _assemble(name, p, exs, anchors, Ms, exps, max_pieces=None, exact=False):
    for A, M_ in zip(anchors, Ms):
        M_[point_pieces(A), 1] = 0
    M = np.concatenate(Ms, 0)
    mp = max(len(a) for a in anchors) if max_pieces is None else max_pieces
    assert mp >= max(len(a) for a in anchors)
    return Case(name, p, anchors, M, exps, mp, exs, exact)


def live_spread(P, n):
    """``n`` piece indices spread over ``[0, P)``, both rays among them from two on."""
    if n <= 0:
        return []
    if n == 1:
        return [P // 2]
    return sorted({int(round(i * (P - 1) / (n - 1))) for i in range(n)})


def random_case(name, F, L, H, C, seed, n_live, bias=True, fixed=True, max_pieces=None, family="random", tables=None,
                live=None, tweak=None):
    """Random / range / dead networks with the tables of a builder (``tables(p) -> PwlTables``; default: the torch builder on the
    CPU) — every live piece is then checked kink-free by the reference itself."""
    import torch
    from gnan_amd import pwl
    if family == "range":
        p = R.range_family(F, L, H, C, seed)[0]
    elif family == "thirds":
        # kinks at m + 1/3, roots at odd twelfths: no float32 holds any of them (tests/test_tables_bound.py:_thirds)
        r = [(1, 0.25), (2, 0.75), ("neg", 0.25), (4, 1.75), (0, 7.75)]
        r3 = [(3, 0.25), (4, 0.75), ("neg", 0.25), (4, 1.75), (0, 7.75)]
        feats = [R.ladder(3, H, C, 6, r, w=3.0, step=3.0, offset=1.0) if L == 3 else
                 R.ladder(4, H, C, 6, r[:2], r3, w=3.0, step=3.0, offset=1.0)]
        p = R.stack_of(feats, L, H, C)
    elif family == "dead":
        p = R.dead_family(L, H, C, seed)
        F = 3
    else:
        p = R.random_state(F, L, H, C, bias, seed)
    if tweak is not None:
        p = tweak(p)
    t = (tables or pwl.build_tables)(p)
    off = t.off.cpu().tolist()
    anchor = t.anchor.cpu().numpy()
    anchors = [anchor[off[k]:off[k + 1]].copy() for k in range(F)]
    rng = np.random.default_rng(seed)
    Ms = []
    for k, A in enumerate(anchors):
        # live pieces of positive width only (a zero-width piece holds no node)
        ok = [t_ for t_ in range(len(A)) if t_ == 0 or t_ == len(A) - 1 or A[t_ + 1] > A[t_]]
        want = live[k] if live is not None else n_live
        pick = [ok[i] for i in live_spread(len(ok), want)] if isinstance(want, int) else want
        if fixed:
            Ms.append(int_moments(rng, len(A), C, pick))
        else:
            m = np.zeros((len(A), 2, C), np.float32)
            for t_ in pick:
                m[t_] = rng.standard_normal((2, C)).astype(np.float32)
            Ms.append(m)
    exs = features_of(p, kinks=False)
    return _assemble(name, p, exs, anchors, Ms, (30, 36) if fixed else None, max_pieces)


def hand_case(name, feats, L, H, C, extra, live, rng, bias=True, exps=(30, 36), max_pieces=None, moments=None, exact=False,
              bits=40):
    """Features given as arrays (ladders, switch nets) with tables that refine the exact partition: ``extra[k]`` superfluous
    anchors, ``live[k]`` the live piece indices (or a callable of the anchors), ``moments(k, A, M)`` edits the integers."""
    p = R.stack_of(feats, L, H, C, bias=bias)
    exs = R.features_of(p)
    anchors, Ms = [], []
    for k, ex in enumerate(exs):
        A = table_anchors(ex, extra[k] if extra else ())
        lv = live[k](A) if callable(live[k]) else live[k]
        M = int_moments(rng, len(A), C, lv, bits=bits)
        if moments is not None:
            M = moments(k, A, M)
        anchors.append(A)
        Ms.append(M)
    return _assemble(name, p, exs, anchors, Ms, exps, max_pieces, exact)
