"""Attributions reduced over groups of rows (``gnan_attr_reduce``) restated in float64 with a DERIVED bound per element — TEST
INFRASTRUCTURE ONLY, built on ``tests/attr_ref.reference`` (the per-row truth ``t`` and bound ``b`` of every term).

Truth        M[g, 0, d, w] = sum_q t          M[g, 1, d, w] = sum_q |t|          M[g, 2, d, w] = sum_q t^2            d < D
             M[g, j, D, w] = the same moments of T[q, w] = sum_{d < D} t[q, d, w]
             over the requested rows q = group_ptr[g] .. group_ptr[g + 1] - 1 (``None``: one group of all of them)

Bound, with n the rows of the group and gamma64(n) = n 2^-53 / (1 - n 2^-53):
  all-distances slot, per row   B = sum_d b[d] + gamma64(D) sum_d (|t[d]| + b[d])      D float64 additions in shell order of terms that
                                                                                       are each within b of their truth
  sum and abs-sum               sum_q b + gamma64(n) sum_q (|t| + b)                   ||x| - |y|| <= |x - y|: the magnitude never widens
                                                                                       the gap between a computed term and its truth
  square sum                    sum_q s + gamma64(n) sum_q (t^2 + s),  s = b (2 |t| + b)

The per-term bound b = gamma_k M of attr_ref holds for csrc/attr_reduce.hip with the same count k = m + 1 (m' + 2 for a rest shell
formed from s_total), from the kernel's own roundings: the m pairs of a shell are added by the lanes of ONE wave — every pair slot keeps a
running sum that starts at +0 (0 + x is exact, as is x + 0 for a slot without a pair of the shell), the slots are added in slot order,
a long row's chunks in chunk order — so every float32 addition on a term's way to the root merges two disjoint groups that each hold
at least one pair, and a term passes at most m - 1 rounded additions whatever the tree; the weight adds one division and one product.
The rest shell from s_total: the listed sum over the m' pairs below D - 1 is the shells' sums in shell order (the same argument),
then the subtraction, the division and the product.

The float64 part: a term's double is exact, so is its magnitude, and so is its square (24-bit significand); the square of a row's
total is one rounded product.  A group's n values are added by a fixed tree (the rows of a wave in row order, the four waves of a
block, the blocks of a run, sixteen runs) whose empty branches add exact zeros: at most n - 1 rounded additions on a value's way, n
with the product — gamma64(n) on the magnitudes actually added, which lie within b (s) of |t| (t^2).

No element is left out of the comparison; where the bound is 0 the output must be exactly the truth (an empty group: exact zeros).
"""
import numpy as np
import torch

import attr_ref

U64 = 2.0 ** -53


def gamma64(n):
    n = np.asarray(n, dtype=np.float64)
    return n * U64 / (1.0 - n * U64)


def row_terms(code, S, lut, rowptr=None, col=None, cnt=None, s_total=None, rows=None):
    """``(T, B)`` float64 ``[R, D + 1, W]``: attr_ref's truth and bound per term, extended by the all-distances slot."""
    t, b, _ = attr_ref.reference(code, S, lut, rowptr, col, cnt, s_total, rows)
    D = t.shape[1]
    tot = np.zeros_like(t[:, 0])
    for d in range(D):                                                # shell order (the truth does not depend on it)
        tot = tot + t[:, d]
    btot = b.sum(1) + gamma64(D) * (np.abs(t) + b).sum(1)
    return np.concatenate([t, tot[:, None]], 1), np.concatenate([b, btot[:, None]], 1)


def moments(T, B, group_ptr=None):
    """``(truth, bound)`` float64 ``[G, 3, D + 1, W]`` of the row terms ``T`` with per-term bounds ``B``."""
    R = T.shape[0]
    gp = np.array([0, R]) if group_ptr is None else np.asarray(group_ptr, dtype=np.int64).reshape(-1)
    assert gp[0] == 0 and gp[-1] == R and (np.diff(gp) >= 0).all()
    G = len(gp) - 1
    truth = np.zeros((G, 3) + T.shape[1:])
    bound = np.zeros_like(truth)
    for g in range(G):
        t, b = T[gp[g]:gp[g + 1]], B[gp[g]:gp[g + 1]]
        n = t.shape[0]
        if n == 0:
            continue
        s = b * (2.0 * np.abs(t) + b)
        acc = gamma64(n)
        truth[g, 0], truth[g, 1], truth[g, 2] = t.sum(0), np.abs(t).sum(0), (t * t).sum(0)
        bound[g, 0] = bound[g, 1] = b.sum(0) + acc * (np.abs(t) + b).sum(0)
        bound[g, 2] = s.sum(0) + acc * (t * t + s).sum(0)
    return truth, bound


def reference(code, S, lut, rowptr=None, col=None, cnt=None, s_total=None, rows=None, group_ptr=None):
    T, B = row_terms(code, S, lut, rowptr, col, cnt, s_total, rows)
    return moments(T, B, group_ptr)


def _np(got):
    return got.detach().cpu().double().numpy() if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)


def violations(got, truth, bound):
    """Indices of the elements of ``got`` outside the bound (every element is judged; a non-finite value is a violation)."""
    g = _np(got).reshape(truth.shape)
    return np.argwhere(~np.isfinite(g) | ~(np.abs(g - truth) <= bound))


def check(got, truth, bound, what=""):
    bad = violations(got, truth, bound)
    if len(bad):
        i = tuple(bad[0])
        g = _np(got).reshape(truth.shape)
        raise AssertionError(f"{what}: {len(bad)} of {truth.size} elements outside their bound; first {list(i)}: got {g[i]!r}, truth "
                             f"{truth[i]!r}, |diff| {abs(g[i] - truth[i]):.3e} > bound {bound[i]:.3e}")
