"""The table path's per-piece moments restated on the CPU, with a DERIVED bound per element — TEST INFRASTRUCTURE ONLY (numpy; no GPU).

The kernels (csrc/fpwl_moments.hip, csrc/fpwl_moments_c1_body.hpp, csrc/fpwl_rows.hip) bin, per piece t of a feature and per channel c,

    M0[t, c] = sum g            M1[t, c] = sum g (x - anchor[t])          over the nodes whose x falls into the piece,

in 64-bit fixed point with two GLOBAL scales 2^e0, 2^e1 (``gnan_fpwl_moment_scales``): the error of a term is absolute.

Scales       bits = min(50, 61 - max(1, bit_length(max(n, 2) - 1))),   e0 = floor(bits - log2 max|g|),
             e1 = floor(bits - log2(max|g| (max|x| + max|anchor|))), clamped to +-1000; the maxima over the gradient AS PASSED.
Ownership    piece of x in feature k = #{ j >= 1 : anchor_k[j] <= x }  (an x ON an anchor belongs to the piece that anchor opens).
Restatement  M0 = sum rint(float64(g) 2^e0)   (half to even: what ``fixed_bits`` does below 2^51), exact in int64;
             M1 = sum rint(float64(float32(g * float32(x - a))) 2^e1)  on every route but the kept one: a float32 subtraction,
             then a float32 product, no fma between them (numpy float32 arithmetic is IEEE, one rounding per operation).
             Compared with the kernels' raw bins bit for bit.
Kept route   (``fpwl_moments_c1_kernel`` over the forward's pieces)  M1x = sum rint(g x 2^e1): the float64 product of two float32
             values is exact and the fma onto 1.5 * 2^52 rounds once.  A workgroup w then adds
                 m1_w = m1x_w - rn(fl64(a * fl64(m0_w)) * 2^(e1 - e0))
             so the kernel's M1 differs from R = M1x - a M0 2^(e1 - e0) (a rational number, formed exactly here) by at most
                 K_t = W_t / 2  +  |a| 2^(e1 - e0) A0_t 2^-52 (1 + 2^-50)                                    [quanta of 2^-e1]
             W_t: workgroups that hold a node of the piece (node blocks of ``nodes_per_block`` nodes from the route query; at
                  most one per node of the piece, at most the blocks of the launch) — one ``__double2ll_rn`` each: 1/2;
             A0_t = sum |rint(g 2^e0)| >= sum_w |m0_w|; the 2^-52: two float64 roundings of relative 2^-53 per workgroup, the
                  product a * m0 and the conversion of an m0 above 2^53 (counted whether or not m0 is that large); the
                  multiplication by the power of two 2^(e1 - e0) is exact.
Truth        T0 = sum g, T1 = sum g x - a sum g with ``math.fsum`` over products that are exact in float64: correctly rounded.
Bound        |M0 2^-e0 - T0| <= n_t 2^-e0 / 2
             |M1 2^-e1 - T1| <= n_t 2^-e1 / 2 + gamma_2 A1 + n_t 2^-149      float32-product routes, A1 = sum |g| |x - a|,
                                gamma_k = k u / (1 - k u), u = 2^-24; the last term: a product that underflows;
             |M1 2^-e1 - T1| <= (n_t / 2 + |a| 2^(e1 - e0) n_t / 2 + K_t) 2^-e1     kept route (no float32 term: the quantisation
                                of the g x terms, of M0 carried through a M0, and the flush);
             float bins (``fpwl_moments_kernel<.., false>``): the LDS chain over the piece's m_w nodes in a block and one global add
             per block put a term through at most (m_w - 1) + (W_t - 1) <= n_t - 1 additions (the bins start at zero: the first add
             is exact), the M1 term through two more roundings:  gamma_(n_t - 1) A0  and  gamma_(n_t + 1) A1 + n_t 2^-149.
             Each plus 2^-52 |T| for the truth's own rounding.  n_t = 0 demands an exact zero; no element is left out.
"""
import math
from fractions import Fraction
from typing import NamedTuple

import numpy as np

U = 2.0 ** -24
MAGIC = 6755399441055744.0            # 1.5 * 2^52 (csrc/fpwl_common.hpp fixed_bits)
MAGIC_BITS = 0x4338000000000000


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


class HandTables(NamedTuple):
    off: np.ndarray      # int32 [F + 1]
    anchor: np.ndarray   # float32 [T], strictly increasing inside a feature
    step: float          # every anchor is an integer multiple of it

    @property
    def F(self):
        return len(self.off) - 1

    def of(self, k):
        return self.anchor[self.off[k]:self.off[k + 1]]


def hand_tables(counts, rng, step=2.0 ** -10, offset=()):
    """Tables with ``counts[k]`` pieces in feature k.  Anchors: distinct multiples of ``step`` — within about +-2 for
    step = 2^-10 (0 and 1 among them from three pieces on: one-hot inputs sit ON anchors), integers for step = 1 —; features
    listed in ``offset`` have theirs in [1000, 1001] (step = 1: from 1000 up) — the kept route's cancellation."""
    off = np.zeros(len(counts) + 1, dtype=np.int32)
    off[1:] = np.cumsum(counts)
    anchor = np.empty(off[-1], dtype=np.float32)
    for k, P in enumerate(counts):
        if step == 1.0:
            lo, hi = (1000, 1000 + 2 * P + 8) if k in offset else (-P - 4, P + 4)
        else:
            lo, hi = (1000 * 1024, 1001 * 1024) if k in offset else (-2048, 2048)
        must = [0, int(round(1 / step))] if (P >= 3 and k not in offset and lo <= 0 and hi >= 1 / step) else []
        pool = np.setdiff1d(np.arange(lo, hi + 1), must)
        pick = np.sort(np.concatenate([rng.choice(pool, P - len(must), replace=False), must]).astype(np.int64))
        anchor[off[k]:off[k + 1]] = (pick.astype(np.float64) * step).astype(np.float32)
        assert np.all(np.diff(anchor[off[k]:off[k + 1]]) > 0)
    return HandTables(off, anchor, step)


def as_pwl(ht, C, rng, device="cpu", features_per_group=None):
    """``pwl.PwlTables`` of hand-built anchors: ``val`` / ``slope`` arbitrary (the moments do not read them), the grouping from
    ``pwl._plan_groups`` (or a stated group width: the C ABI takes 1, 2, 4, 8, 16)."""
    import torch
    from gnan_amd import pwl
    off = [int(v) for v in ht.off]
    F, T = ht.F, off[-1]
    if features_per_group is None:
        fg, mg = pwl._plan_groups(off, C)
    else:
        fg = features_per_group
        mg = max(off[min(F, k + fg)] - off[k] for k in range(0, F, fg))
    val = torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32))
    slope = torch.from_numpy(rng.standard_normal((T, C)).astype(np.float32))
    return pwl.PwlTables(torch.from_numpy(ht.off.copy()).to(device), torch.from_numpy(ht.anchor.copy()).to(device), val.to(device),
                         slope.to(device), int(np.diff(ht.off).max()), fg, mg)


X_FAMILIES = ("uniform", "levels", "onehot", "rays", "cover", "onepiece", "grid")


def draw_x(rng, family, ht, n):
    """float32 ``[n, F]``.  'uniform' over the anchors' range and one unit beyond (tables with an offset feature: the offset
    family); 'levels' every x exactly ON an anchor of its feature (d = 0, ownership by <=); 'onehot' 0 or 1 (on anchors where
    the feature has them); 'rays' up to 10^4 beyond the outer anchors, the extreme attained; 'cover' row by row through every
    piece's midpoint, every anchor and both rays — except, from four pieces on, piece 2 (left EMPTY) and piece 3 (ONE node: row 0,
    on its anchor); 'onepiece' all nodes strictly inside one piece per feature — with the same-sign gradient the largest sum
    the headroom must hold (it cannot see a headroom one bit short: n terms below 2^bits stay below 2^62 and an int64 has one
    more bit); 'grid' uniform on multiples of the tables' step (every x - a is such a multiple)."""
    F = ht.F
    x = np.empty((n, F), dtype=np.float32)
    for k in range(F):
        a = ht.of(k).astype(np.float64)
        P = len(a)
        if family == "uniform":
            col = rng.uniform(a[0] - 1.0, a[-1] + 1.0, n)
        elif family == "grid":
            col = rng.integers(int(a[0] / ht.step) - 64, int(a[-1] / ht.step) + 65, n) * ht.step
        elif family == "levels":
            col = a[rng.integers(0, P, n)]
        elif family == "onehot":
            col = rng.integers(0, 2, n).astype(np.float64)
        elif family == "rays":
            r = rng.uniform(0.0, 1.0e4, n)
            r[0] = r[n // 2] = 1.0e4
            col = np.where(rng.integers(0, 2, n) == 1, a[-1] + r, a[0] - r)
            col[0], col[n // 2] = a[-1] + 1.0e4, a[0] - 1.0e4
        elif family == "cover":
            mids = [a[0] - 0.5 * max(ht.step, 1e-3)] + [0.5 * (a[i] + a[i + 1]) for i in range(1, P - 1)] + ([a[-1] + 0.25] if P > 1 else [])
            own = list(range(P))            # mids[i] lies in piece i (piece 0: left of a[1], here left of a[0] as well)
            cands = [(i, mids[i]) for i in own] + [(i, a[i]) for i in range(P)] + [(0, a[0] - 77.0), (P - 1, a[-1] + 77.0)]
            if P >= 4:
                cands = [c for c in cands if c[0] not in (2, 3)]
            vals = np.array([c[1] for c in cands])
            col = vals[np.arange(n) % len(vals)]
            if P >= 4:
                col[0] = a[3]
        elif family == "onepiece":
            i = int(rng.integers(0, P))
            lo = a[i] if i > 0 else a[0] - 1.0
            hi = a[i + 1] if i + 1 < P else a[-1] + 1.0
            col = rng.uniform(lo + 0.25 * (hi - lo), lo + 0.75 * (hi - lo), n)
        else:
            raise ValueError(family)
        x[:, k] = col.astype(np.float32)
    return x


G_FAMILIES = ("unit", "range", "outlier", "same-sign", "same-sign-neg", "zeros", "integers", "unit-up", "unit-down")


def draw_g(rng, family, n, width):
    """float32 ``[n, width]``, after ``rowwise.narrow_operand``: 'unit' N(0, 1) (|g| >= 2^-12: see 'unit-up'); 'range' every row
    times 2^k, k uniform in [-40, 10] — the M0 quantisation is attained (for 'unit' g 2^e0 is an integer: M0 is exact); 'outlier'
    one 2^60 entry: the pieces of small gradients lose everything, which is the contract, and the bound says so; 'same-sign'
    every entry the float below 2, and its negation; 'zeros'; 'integers' in [-4, 4]; 'unit-up' / 'unit-down' the unit gradient
    times 2^+-100: the same bins bit for bit with the scales shifted by 100, as long as no float32 product underflows."""
    g = rng.standard_normal((n, width)).astype(np.float32)
    g = np.where(np.abs(g) < 2.0 ** -12, np.float32(2.0 ** -12), g).astype(np.float32)
    if family == "range":
        g = (g * np.exp2(rng.integers(-40, 11, (n, 1)).astype(np.float64))).astype(np.float32)
    elif family == "outlier":
        g[n - 1, width - 1] = np.float32(2.0 ** 60)
    elif family in ("same-sign", "same-sign-neg"):
        g[:] = np.nextafter(np.float32(2.0), np.float32(0.0))
        g = -g if family.endswith("neg") else g
    elif family == "zeros":
        g[:] = 0.0
    elif family == "integers":
        g = rng.integers(-4, 5, (n, width)).astype(np.float32)
    elif family == "unit-up":
        g = (g.astype(np.float64) * 2.0 ** 100).astype(np.float32)
    elif family == "unit-down":
        g = (g.astype(np.float64) * 2.0 ** -100).astype(np.float32)
    elif family != "unit":
        raise ValueError(family)
    return g


def restate_bits(n):
    return min(50, 61 - max(1, (max(n, 2) - 1).bit_length()))


def restate_scales(n, g, x, anchor):
    """(e0, e1) as ``gnan_fpwl_moment_scales`` forms them, from the arrays as passed.  (``floor(bits - log2 v)`` in float64, as the
    kernel writes it; a zero maximum is taken as DBL_MIN.)"""
    bits = restate_bits(n)
    gm = max(float(np.max(np.abs(g))) if g.size else 0.0, 2.2250738585072014e-308)
    dm = max(float(np.max(np.abs(x.astype(np.float64)))) + float(np.max(np.abs(anchor.astype(np.float64)))), 2.2250738585072014e-308)
    e0 = min(max(math.floor(bits - math.log2(gm)), -1000), 1000)
    e1 = min(max(math.floor(bits - math.log2(gm * dm)), -1000), 1000)
    return int(e0), int(e1)


def owners(x, ht, strict=False):
    """Global piece index ``[n, F]``: off[k] + #{ j >= 1 : anchor_k[j] <= x }.  (``strict``: the planted ``<``.)"""
    t = np.empty(x.shape, dtype=np.int64)
    for k in range(ht.F):
        a = ht.of(k)
        t[:, k] = ht.off[k] + np.searchsorted(a[1:], x[:, k], side="left" if strict else "right")
    return t


def _g_of(g, k, C, sum_features):
    return g if sum_features else g[:, k * C:(k + 1) * C]


def _rint_scaled(v64, e):
    """rint(v * 2^e) as int64 (|v 2^e| < 2^51: exact in float64; numpy's rint rounds half to even)."""
    return np.rint(np.ldexp(v64, e)).astype(np.int64)


def restate(x, g, ht, C, sum_features, e0, e1):
    """The exact integer restatement: dict of int64 ``[T, C]`` arrays  M0, M1 (float32-product routes), M1x (kept route: sum
    rint(g x 2^e1)), A0 = sum |rint(g 2^e0)|, and ``shifts`` = whether every nonzero float32 product is a normal number."""
    T = int(ht.off[-1])
    out = {k: np.zeros((T, C), dtype=np.int64) for k in ("M0", "M1", "M1x", "A0")}
    t = owners(x, ht)
    normal = True
    for k in range(ht.F):
        gk = np.ascontiguousarray(_g_of(g, k, C, sum_features))
        tk = t[:, k]
        d = (x[:, k] - ht.anchor[tk]).astype(np.float32)                  # float32 subtraction
        prod = (gk * d[:, None]).astype(np.float32)                         # float32 product, rounded once
        normal = normal and bool(np.all((prod == 0) | (np.abs(prod) >= np.float32(2.0 ** -126))))
        q0 = _rint_scaled(gk.astype(np.float64), e0)
        q1 = _rint_scaled(prod.astype(np.float64), e1)
        q1x = _rint_scaled(gk.astype(np.float64) * x[:, k].astype(np.float64)[:, None], e1)   # exact product of two float32
        order = np.argsort(tk, kind="stable")                               # (int64 sums per piece: sort, then reduceat)
        ts = tk[order]
        starts = np.flatnonzero(np.concatenate([[True], np.diff(ts) != 0]))
        for name, q in (("M0", q0), ("M1", q1), ("M1x", q1x), ("A0", np.abs(q0))):
            out[name][ts[starts]] += np.add.reduceat(q[order], starts, axis=0)
    out["normal"] = normal
    return out


def truth(x, g, ht, C, sum_features):
    """float64 ``[T, C]``: T0, T1 (correctly rounded: fsum over exact products), A0 = sum |g|, A1 = sum |g| |x - a|; cnt ``[T]``."""
    T = int(ht.off[-1])
    T0, T1 = np.zeros((T, C)), np.zeros((T, C))
    A0, A1 = np.zeros((T, C)), np.zeros((T, C))
    cnt = np.zeros(T, dtype=np.int64)
    t = owners(x, ht)
    for k in range(ht.F):
        gk = _g_of(g, k, C, sum_features).astype(np.float64)
        tk = t[:, k]
        xk = x[:, k].astype(np.float64)
        ak = ht.anchor[tk].astype(np.float64)
        cnt += np.bincount(tk, minlength=T)
        np.add.at(A0, tk, np.abs(gk))
        np.add.at(A1, tk, np.abs(gk) * np.abs(xk - ak)[:, None])
        order = np.argsort(tk, kind="stable")
        ts = tk[order]
        cuts = np.flatnonzero(np.diff(ts)) + 1
        starts = np.concatenate([[0], cuts])
        ends = np.concatenate([cuts, [len(ts)]])
        gx = gk * xk[:, None]                                              # exact: two float32 values
        ga = gk * ak[:, None]
        for s, e in zip(starts, ends):
            rows = order[s:e]
            piece = int(ts[s])
            for c in range(C):
                T0[piece, c] = math.fsum(gk[rows, c].tolist())
                T1[piece, c] = math.fsum(gx[rows, c].tolist() + (-ga[rows, c]).tolist())
    return {"T0": T0, "T1": T1, "A0": A0, "A1": A1, "cnt": cnt}


def blocks_per_piece(x, ht, nodes_per_block):
    """W_t ``[T]``: node blocks [b npb, (b + 1) npb) that hold a node of piece t."""
    T = int(ht.off[-1])
    t = owners(x, ht)
    nb = (x.shape[0] + nodes_per_block - 1) // nodes_per_block
    blk = (np.arange(x.shape[0]) // nodes_per_block)[:, None]
    seen = np.unique((t * nb + blk).ravel())
    return np.bincount(seen // nb, minlength=T).astype(np.int64)


def kept_slack(ht, ref, e0, e1, W):
    """K_t ``[T, C]`` in quanta of 2^-e1 (file header)."""
    a = np.abs(ht.anchor.astype(np.float64))[:, None]
    return W[:, None] / 2.0 + a * 2.0 ** (e1 - e0) * ref["A0"].astype(np.float64) * 2.0 ** -52 * (1.0 + 2.0 ** -50)


def kept_residual(M1, ht, ref, e0, e1):
    """|M1 - (M1x - a M0 2^(e1 - e0))| ``[T, C]`` in quanta, the rational number formed exactly."""
    T, C = ref["M0"].shape
    out = np.zeros((T, C))
    ratio = Fraction(2) ** (e1 - e0)
    for t in range(T):
        a = Fraction(float(ht.anchor[t]))
        for c in range(C):
            r = Fraction(int(ref["M1x"][t, c])) - a * int(ref["M0"][t, c]) * ratio
            out[t, c] = float(abs(Fraction(int(M1[t, c])) - r))
    return out


def fixed_bounds(tr, e0, e1, ht=None, kept_K=None):
    """(b0, b1) ``[T, C]`` of the fixed-point routes (header); with ``kept_K`` the kept route's."""
    n_t = tr["cnt"].astype(np.float64)[:, None]
    b0 = n_t * 2.0 ** -e0 / 2.0 + 2.0 ** -52 * np.abs(tr["T0"])
    if kept_K is None:
        b1 = n_t * 2.0 ** -e1 / 2.0 + gamma(2) * tr["A1"] + n_t * 2.0 ** -149
    else:
        a = np.abs(ht.anchor.astype(np.float64))[:, None]
        b1 = (n_t / 2.0 + a * 2.0 ** (e1 - e0) * n_t / 2.0 + kept_K) * 2.0 ** -e1
    return b0, b1 + 2.0 ** -52 * np.abs(tr["T1"])


def float_bounds(tr):
    n_t = tr["cnt"].astype(np.float64)[:, None]
    b0 = gamma(np.maximum(n_t - 1, 0)) * tr["A0"] + 2.0 ** -52 * np.abs(tr["T0"])
    b1 = gamma(n_t + 1) * tr["A1"] + n_t * 2.0 ** -149 + 2.0 ** -52 * np.abs(tr["T1"])
    return b0 * (tr["cnt"] > 0)[:, None], b1 * (tr["cnt"] > 0)[:, None]


def worst_ratio(got, want, bound):
    """max |got - want| / bound over the elements with a bound; where the bound is 0 the value must be EXACTLY the truth."""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    zero = bound == 0
    if np.any(err[zero] != 0):
        return float("inf")
    if np.all(zero):
        return 0.0
    return float(np.max(err[~zero] / bound[~zero]))


def assert_within(got, want, bound, what=""):
    r = worst_ratio(got, want, bound)
    assert r <= 1.0, f"{what}: |err| / bound = {r:.3g}"
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# The kernels' own arithmetic, in numpy: the search route and the kept route over an explicit node-block partition.  Each
# ``plant`` is one of the planted errors of tests/test_moments_bound.py.
# ---------------------------------------------------------------------------------------------------------------------------
def _fixed_bits(v64, s, trunc=False):
    """``fixed_bits``: fma(v, s, 1.5 * 2^52) — v s is exact (s a power of two), so the fma is ONE float64 addition — and the
    integer read out of the low mantissa bits."""
    p = v64 * s
    if trunc:
        return np.trunc(p).astype(np.int64)
    return (p + MAGIC).view(np.int64) - np.int64(MAGIC_BITS)


def _search(a, xs, step0, strict=False):
    """``search<>`` of csrc/fpwl_common.hpp: idx = #{ j in 1..pn : a[j] <= x } by descending powers of two."""
    pn = len(a) - 1
    idx = np.zeros(len(xs), dtype=np.int64)
    step = step0
    while step > 0:
        j = idx + step
        ok = j <= pn
        aj = a[np.where(ok, j, 0)]
        idx = np.where(ok & ((aj < xs) if strict else (aj <= xs)), j, idx)
        step >>= 1
    return idx


def emulate(x, g, ht, C, sum_features, route="search", nodes_per_block=256, plant=None):
    """int64 ``[T, 2, C]`` and (e0, e1).  ``route``: 'search' (float32 product) or 'kept' (C = 1: sum g x, anchor at the flush of
    every node block).  ``plant``: None | 'coarse' | 'trunc' | 'half-max' | 'strict' | 'neighbour' | 'tail' | 'ratio'."""
    n, F = x.shape
    T = int(ht.off[-1])
    gs = g[:n // 2] if plant == "half-max" else g
    e0, e1 = restate_scales(n, gs, x, ht.anchor)
    if plant == "coarse":
        e0, e1 = e0 - 8, e1 - 8
    s0, s1 = 2.0 ** e0, 2.0 ** e1
    trunc = plant == "trunc"
    maxp = int(np.diff(ht.off).max())
    step0 = 0
    while (step0 * 2 if step0 else 1) <= maxp - 1:
        step0 = step0 * 2 if step0 else 1
    M = np.zeros((T, 2, C), dtype=np.int64)
    cols = np.arange(C)[None, :]
    keep = np.ones(n, dtype=bool)
    if plant == "tail":
        keep[n - 1] = False                      # the last node of the last block's tail
    for k in range(F):
        a = ht.of(k)
        loc = _search(a, x[:, k], step0, strict=plant == "strict")
        tk = ht.off[k] + loc
        gk = np.ascontiguousarray(_g_of(g, k, C, sum_features))
        if route == "search":
            ta = ht.off[k] + np.minimum(loc + 1, len(a) - 1) if plant == "neighbour" else tk
            d = (x[:, k] - ht.anchor[ta]).astype(np.float32)
            prod = (gk * d[:, None]).astype(np.float32)
            idx = (np.broadcast_to(tk[:, None], gk.shape)[keep], np.broadcast_to(cols, gk.shape)[keep])
            np.add.at(M[:, 0, :], idx, _fixed_bits(gk.astype(np.float64), s0, trunc)[keep])
            np.add.at(M[:, 1, :], idx, _fixed_bits(prod.astype(np.float64), s1, trunc)[keep])
        else:
            assert C == 1
            ratio = s0 / s1 if plant == "ratio" else s1 / s0
            for lo in range(0, n, nodes_per_block):
                sl = slice(lo, min(lo + nodes_per_block, n))
                kp = keep[sl]
                m0 = np.zeros(T, dtype=np.int64)
                m1x = np.zeros(T, dtype=np.int64)
                g64 = gk[sl, 0].astype(np.float64)
                np.add.at(m0, tk[sl][kp], _fixed_bits(g64, s0, trunc)[kp])
                v = (g64 * s1) * x[sl, k].astype(np.float64)                 # g 2^e1 exact, the product exact in the fma
                np.add.at(m1x, tk[sl][kp], (np.trunc(v) if trunc else np.rint(v)).astype(np.int64)[kp])
                ta = np.arange(T)
                if plant == "neighbour":
                    ta = np.minimum(ta + 1, ht.off[k + 1] - 1)
                with np.errstate(invalid="ignore", over="ignore"):      # (a planted ratio may leave the int64 range)
                    sub = np.rint(ht.anchor[ta].astype(np.float64) * m0.astype(np.float64) * ratio).astype(np.int64)
                own = (np.arange(T) >= ht.off[k]) & (np.arange(T) < ht.off[k + 1])
                M[own, 0, 0] += m0[own]
                M[own, 1, 0] += (m1x - sub)[own]
    return M, (e0, e1)


# ---------------------------------------------------------------------------------------------------------------------------
# The cases of tests/test_gpu_moment_pieces.py.  tests/test_moments_bound.py runs the reference alone over every one of them
# (and asks the library's host-only route query about each) before a GPU is involved.
# ---------------------------------------------------------------------------------------------------------------------------
MIX16 = (1, 2, 3, 64, 65, 128, 129, 256, 5, 17, 1, 2, 33, 7, 100, 12)
MIX32 = MIX16 + (256, 255, 4, 9, 1, 3, 2, 31, 32, 63, 66, 127, 130, 20, 6, 8)
NODES_C1 = 128                 # nodes per round of the c1 kernels with 16-feature groups (512 threads, a feature quad each)
BLOCK_SMALL = 256              # tuned_moment_block below 16 384 nodes


class Case(NamedTuple):
    name: str
    counts: tuple
    n: int
    route: str                     # the kernel the query must report (GNAN_FPWL_MOMENTS_* without the prefix, lower case)
    C: int = 1
    sum_features: bool = True
    gfam: str = "unit"
    xfam: str = "cover"
    step: float = 2.0 ** -10
    offset: tuple = ()
    kept: bool = False             # the pieces of a real forward are handed to the moments
    gshift: bool = False           # the gradient is a column-offset view of a wider buffer
    xshift: bool = False           # ... and so is x
    general: bool = False          # functional.MOMENTS_GENERAL
    fixed: bool = True             # functional.MOMENTS_FIXED_POINT
    fpg: int = 0                   # a stated features_per_group instead of pwl._plan_groups'
    stale_pieces: bool = False     # a piece buffer is attached although the tables exceed the byte: it must be ignored
    rows_min: int = 0              # functional.FPWL_ROWS_MIN_NODES for the case (rows kernels)
    nstep: int = -1                # the tree depth the query must report (-1: not asserted)
    block: int = 0                 # nodes_per_block the query must report (0: not asserted)


def _family_cases():
    out = []
    for route, kept in (("c1_search", False), ("c1_kept", True)):
        for gfam in G_FAMILIES:
            for xname in ("uniform", "levels", "offset"):
                ints = gfam == "integers"
                xfam = {"uniform": "grid" if ints else "uniform", "levels": "levels", "offset": "grid" if ints else "uniform"}[xname]
                out.append(Case(f"fam-{route}-{gfam}-{xname}", MIX16, 2 * BLOCK_SMALL + NODES_C1 + 1, route, gfam=gfam, xfam=xfam,
                                step=1.0 if ints else 2.0 ** -10, offset=(1, 7) if xname == "offset" else (), kept=kept, nstep=8,
                                block=BLOCK_SMALL))
    return out


def _tail_cases():
    out = []
    for route, kept in (("c1_search", False), ("c1_kept", True)):
        for tail in (1, NODES_C1 - 1, NODES_C1, NODES_C1 + 1, 2 * NODES_C1):
            out.append(Case(f"tail-{route}-{tail}", MIX32, BLOCK_SMALL + tail, route, gfam="range", kept=kept, nstep=8, block=BLOCK_SMALL))
        out.append(Case(f"tail-{route}-one-node", MIX32, 1, route, gfam="range", kept=kept, block=BLOCK_SMALL))
        out.append(Case(f"tail-{route}-rays", MIX16, BLOCK_SMALL + 3, route, gfam="unit", xfam="rays", kept=kept))
        for n in (4096, 4097):
            for gfam in ("same-sign", "same-sign-neg"):
                out.append(Case(f"headroom-{route}-{n}-{gfam}", (5, 64, 256, 2) + (3,) * 12, n, route, gfam=gfam, xfam="onepiece", kept=kept))
    # blocks of three rounds (tuned_moment_block's branch from 16 384 nodes; 4 groups x 87 blocks of 384 nodes fill the chip's
    # 512 resident workgroups once): the kept loop's third round, and last blocks of 2 NODES + 1 and 3 NODES - 1 nodes
    for tail in (2 * NODES_C1 + 1, 3 * NODES_C1 - 1):
        out.append(Case(f"tail-c1_kept-three-rounds-{tail}", MIX16 * 4, 86 * 3 * NODES_C1 + tail, "c1_kept", gfam="range", xfam="uniform",
                        kept=True, block=3 * NODES_C1))
    out.append(Case("tail-c1_search-16385", MIX16, 16385, "c1_search", gfam="range", xfam="uniform", block=BLOCK_SMALL))
    # the search route in blocks of three rounds: trees of depth 10 leave one workgroup per compute unit, and 5 groups x 51 blocks
    # of 384 nodes fill 256 units once (77 blocks of 256 nodes would take two rounds)
    deep80 = (1024, 3, 5, 2) + (4,) * 12 + MIX16 * 4
    for tail in (2 * NODES_C1 + 1, 3 * NODES_C1 - 1):
        out.append(Case(f"tail-c1_search-three-rounds-{tail}", deep80, 50 * 3 * NODES_C1 + tail, "c1_search", gfam="range",
                        xfam="uniform", nstep=10, block=3 * NODES_C1))
    return out


def _edge_cases():
    out = []
    for top, nstep in ((64, 6), (65, 7), (128, 7), (129, 8), (256, 8)):
        counts = (top, 1, 2, 3) + (4,) * 12
        for route, kept in (("c1_search", False), ("c1_kept", True)):
            out.append(Case(f"edge-{route}-{top}", counts, BLOCK_SMALL + NODES_C1 + 1, route, kept=kept, nstep=nstep))
    out.append(Case("edge-257-byte-abandoned", (257, 3, 5, 2) + (4,) * 12, 600, "c1_search", stale_pieces=True, nstep=9))
    out.append(Case("edge-1023", (1023, 3, 5, 2) + (4,) * 12, 2100, "c1_search", nstep=10))
    out.append(Case("edge-1024", (1024, 3, 5, 2) + (4,) * 12, 2100, "c1_search", nstep=10))
    out.append(Case("edge-1025-general", (1025, 3, 5, 2) + (4,) * 12, 2100, "general_fixed", nstep=0))
    return out


def _other_routes():
    out = []
    # unit, range and integer gradients; x through every piece and anchor (cover), 0 | 1 (one-hot), ON anchors only (levels), integers
    mixes = (("unit", "cover", 2.0 ** -10), ("range", "onehot", 2.0 ** -10), ("integers", "grid", 1.0), ("unit", "onehot", 2.0 ** -10),
             ("range", "levels", 2.0 ** -10))
    n = BLOCK_SMALL + NODES_C1 + 1
    for gfam, xfam, step in mixes:
        fam = dict(gfam=gfam, xfam=xfam, step=step)
        gfam = f"{gfam}-{xfam}"
        out += [
            Case(f"perfeature-kept-{gfam}", MIX32, n, "c1_kept", sum_features=False, kept=True, **fam),
            Case(f"perfeature-saved-{gfam}", MIX32, n, "c1_saved", sum_features=False, kept=True, gshift=True, **fam),
            Case(f"perfeature-search-{gfam}", MIX32, n, "c1_search", sum_features=False, **fam),
            Case(f"ragged-20-{gfam}", MIX16 + (3, 9, 2, 40), n, "c1_ragged", xshift=True, **fam),
            Case(f"ragged-33-{gfam}", MIX32 + (11,), n, "c1_ragged", sum_features=False, xshift=True, gshift=True, **fam),
            Case(f"ragged-3-{gfam}", (9, 1, 130), n, "c1_ragged", **fam),
            Case(f"narrow-groups-3-{gfam}", (9, 1, 130), n, "general_fixed", fpg=2, **fam),
            Case(f"general-flag-{gfam}", MIX16, n, "fast", general=True, **fam),
            Case(f"general-flag-ragged-{gfam}", MIX16 + (3, 9, 2, 40), n, "general_fixed", general=True, **fam),
        ]
        for C in (2, 3, 8, 9):
            out.append(Case(f"fast-C{C}-{gfam}", (5, 2, 33, 1, 17, 3, 64, 4) * 2, 300, "fast", C=C, sum_features=C % 2 == 0, **fam))
        for C, kind in ((12, "rows"), (40, "rows_pairs"), (64, "rows"), (65, "rows_pairs"), (130, "rows")):
            for sf in (True, False):
                # (piece, dx) kept by the forward or located again: both with every C at one setting of the feature sum, and for
                # 40 and 64 channels (8-byte pair loads; one node per step) at the other as well
                for kept in ((sf, not sf) if C in (40, 64) else (sf,)):
                    out.append(Case(f"rows-C{C}-{'sum' if sf else 'per'}-{'kept' if kept else 'located'}-{gfam}", (5, 9, 2), 1024 + 65,
                                    kind, C=C, sum_features=sf, kept=kept, rows_min=1024, block=1024, **fam))
    out += [
        Case("float-c1-unit", MIX16, n, "general_float", fixed=False),
        Case("float-C3-range", (5, 2, 33, 1, 17, 3, 64, 4) * 2, 300, "general_float", C=3, sum_features=False, gfam="range", fixed=False),
        Case("float-narrow-integers", (9, 1, 130), n, "general_float", fpg=2, gfam="integers", xfam="grid", step=1.0, fixed=False),
    ]
    return out


CASES = _family_cases() + _tail_cases() + _edge_cases() + _other_routes()
KERNELS = ("none", "c1_search", "c1_kept", "c1_saved", "c1_ragged", "fast", "general_fixed", "general_float", "rows", "rows_pairs")
_BUILT = {}


def build_case(case):
    """Tables, inputs, scales, restatement and truth of a case — computed once, shared by every test that needs them, never
    written to."""
    import zlib
    if case.name not in _BUILT:
        # (the scaled families share their draws with the unit case of the same name: the bins are compared bit for bit)
        rng = np.random.default_rng(zlib.crc32(case.name.replace("unit-up", "unit").replace("unit-down", "unit").encode()))
        ht = hand_tables(case.counts, rng, case.step, case.offset)
        x = draw_x(rng, case.xfam, ht, case.n)
        g = draw_g(rng, case.gfam, case.n, case.C if case.sum_features else ht.F * case.C)
        e0, e1 = restate_scales(case.n, g, x, ht.anchor)
        built = dict(ht=ht, x=x, g=g, e0=e0, e1=e1, ref=restate(x, g, ht, case.C, case.sum_features, e0, e1),
                     truth=truth(x, g, ht, case.C, case.sum_features))
        for v in (ht.off, ht.anchor, x, g):
            v.setflags(write=False)
        _BUILT[case.name] = built
    return _BUILT[case.name]


def check_fixed(case, M, scales, nodes_per_block, what=""):
    """Everything a fixed-point result owes its case: the scales, the exact restatement (kept route: M0 exact, M1 inside its
    counted bound around the rational R), the truth bound on EVERY element.  Returns the worst |err| / bound of (M0, M1, and
    on the kept route the flush against K_t)."""
    b = build_case(case)
    ht, ref, tr, e0, e1 = b["ht"], b["ref"], b["truth"], b["e0"], b["e1"]
    assert (float(scales[0]), float(scales[1])) == (2.0 ** e0, 2.0 ** e1), f"{what}: scales {scales} != 2^{e0}, 2^{e1}"
    M = np.asarray(M, dtype=np.int64)
    assert np.array_equal(M[:, 0, :], ref["M0"]), f"{what}: M0 differs from the restatement in {int((M[:, 0, :] != ref['M0']).sum())} bins"
    flush = 0.0
    if case.route == "c1_kept":
        K = kept_slack(ht, ref, e0, e1, blocks_per_piece(b["x"], ht, nodes_per_block))
        flush = assert_within(kept_residual(M[:, 1, :], ht, ref, e0, e1), 0.0, K, what + " kept flush")
        b0, b1 = fixed_bounds(tr, e0, e1, ht, K)
    else:
        assert np.array_equal(M[:, 1, :], ref["M1"]), f"{what}: M1 differs from the restatement in {int((M[:, 1, :] != ref['M1']).sum())} bins"
        b0, b1 = fixed_bounds(tr, e0, e1)
    r0 = assert_within(np.ldexp(M[:, 0, :].astype(np.float64), -e0), tr["T0"], b0, what + " M0")
    r1 = assert_within(np.ldexp(M[:, 1, :].astype(np.float64), -e1), tr["T1"], b1, what + " M1")
    if case.gfam == "integers":              # small integers times integer-valued x - a: exact through every route
        assert np.array_equal(np.ldexp(M[:, 0, :].astype(np.float64), -e0), tr["T0"]), what
        assert np.array_equal(np.ldexp(M[:, 1, :].astype(np.float64), -e1), tr["T1"]), what
    if case.gfam == "zeros":
        assert not M.any(), what
    return r0, r1, flush


def assert_route(case, info):
    assert KERNELS[info["kernel"]] == case.route, (case.name, KERNELS[info["kernel"]])
    assert case.nstep < 0 or info["nstep"] == case.nstep, (case.name, info)
    assert case.block == 0 or info["nodes_per_block"] == case.block, (case.name, info)
    assert info["pieces_kept"] == int(case.kept and case.route.startswith("c1")), (case.name, info)
    assert info["n_blocks"] == -(-case.n // info["nodes_per_block"])
    if case.route.startswith("c1") or case.route == "fast":
        assert (info["nodes_per_round"], info["block_size"]) == (NODES_C1, 512), (case.name, info)     # 16-feature groups


def sibling(case):
    """The unit case a 'unit-up' / 'unit-down' case shares its draws with, and the shift of its scales' exponents."""
    for fam, shift in (("unit-up", -100), ("unit-down", 100)):
        if case.gfam == fam:
            name = case.name.replace(fam, "unit")
            return next(c for c in CASES if c.name == name), shift
    return None, 0


def launch_inputs(case, device):
    """(tables, x, gradient) as torch tensors on ``device``, the column-offset views included (``wide[:, 1:w + 1]`` of a buffer three
    columns wider: rows that are neither 16-byte aligned nor a multiple of four floats apart)."""
    import torch
    b = build_case(case)
    t = as_pwl(b["ht"], case.C, np.random.default_rng(1), device, case.fpg or None)

    def put(a, shift):
        v = torch.from_numpy(a.copy()).to(device)
        if not shift:
            return v
        wide = torch.zeros((a.shape[0], a.shape[1] + 3), dtype=v.dtype, device=device)
        wide[:, 1:a.shape[1] + 1] = v
        return wide[:, 1:a.shape[1] + 1]
    return t, put(b["x"], case.xshift), put(b["g"], case.gshift)
