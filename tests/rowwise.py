"""The aggregation restated in float64 with a DERIVED bound per output element — TEST INFRASTRUCTURE ONLY.  First the wide kernel
(this header), then the narrow routes further down: the propagation-blocked forward, its exact shell sums, the narrow backward.

``helpers.rule`` compares against the largest entry of the whole result, so an error confined to one short row hides under the
hub rows.  Here every element is judged against its own row's magnitude.  The inputs are the kernel's: CSR, codes, ``S``,
the weight table (shared ``[D, Cw]`` or per-row ``[n, D, Cw]``), the counts or none, and the float32 ``s_total`` actually
handed to the launch (so the column-sum kernel's own error is an input, not part of what is judged).

Truth        t[i, c] = sum_l w(i, d_l) S[j_l, c] + w(i, rest) (tot[c] - sum_l S[j_l, c]),      w = lut / max(cnt, 1)
             (listed codes >= D - 1 are clipped to the rest code, as the kernel does; without ``s_total``: the first sum alone)
Magnitude    A[i, c] = sum_l |w(i, d_l)| |S[j_l, c]| + |w(i, rest)| (sum_l |S[j_l, c]| + |tot[c]|)
Bound        |y - t| <= gamma_k A,   gamma_k = k u / (1 - k u),   u = 2^-24,   k = L_i + 5
             the 5: one division, the fold w_d - w_rest (inherits two roundings, adds one), the final fmaf; the L: the fmaf
             chain over the row's pairs.  Rows above the hub threshold: k = 2 L_i (slice partials and the fix-up add at most
             one rounding per slice, and a row has no more slices than pairs).
Fused read-out   channel c' collects the columns c = c' (mod cr):  gamma_{k + 10} sum_c A[i, c]  (at most 4 adds within a
             lane, 6 butterfly steps).
Where the bound is 0 the output must be exactly 0; no element is left out of the comparison.
"""
import numpy as np
import torch

U = 2.0 ** -24
HUB_THRESHOLD = 512          # graph.LONG_ROW_THRESHOLD (tests/test_rowwise_bound.py holds the two equal): rows with more pairs are cut into slices


def _t64(v):
    if torch.is_tensor(v):
        return v.detach().cpu().double()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(v, dtype=np.float64)))


def _idx(v):
    if torch.is_tensor(v):
        return v.detach().cpu().long()
    return torch.from_numpy(np.asarray(v).astype(np.int64))


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U / (1.0 - k * U)


def _truth_mag(rowptr, col, code, S, lut, cnt=None, s_total=None, rows=None):
    """Truth ``t`` and magnitude ``A`` of the header, float64 numpy ``[n, W]``, and the rows' pair counts ``[n]``."""
    rowptr, col, code = _idx(rowptr), _idx(col), _idx(code)
    S, lut = _t64(S), _t64(lut)
    n_all = rowptr.numel() - 1
    rows = torch.arange(n_all) if rows is None else _idx(rows)
    n, W = rows.numel(), S.shape[1]
    D, Cw = lut.shape[-2], lut.shape[-1]
    rest = D - 1
    wt = lut[rows] if lut.dim() == 3 else lut.unsqueeze(0).expand(n, D, Cw)
    if cnt is not None:
        wt = wt / _idx(cnt)[rows].clamp_min(1).double().unsqueeze(-1)
    lo, deg = rowptr[rows], rowptr[rows + 1] - rowptr[rows]
    out_of_pair = torch.repeat_interleave(torch.arange(n), deg)
    pair = torch.repeat_interleave(lo - (torch.cumsum(deg, 0) - deg), deg) + torch.arange(int(deg.sum()))
    pc, pd = col[pair], code[pair].clamp_max(rest)
    tot = None if s_total is None else _t64(s_total).reshape(-1)
    truth = torch.empty((n, W), dtype=torch.float64)
    mag = torch.empty((n, W), dtype=torch.float64)
    step = max(1, min(W, (1 << 22) // max(1, pair.numel())))          # columns per pass: bounds the [pairs, columns] temporaries
    for c0 in range(0, W, step):
        cs = torch.arange(c0, min(W, c0 + step))
        ch = cs % Cw
        w = wt[out_of_pair, pd][:, ch]                               # [pairs, columns]
        s = S[pc][:, cs]
        zero = torch.zeros((n, cs.numel()), dtype=torch.float64)
        t = zero.clone().index_add_(0, out_of_pair, w * s)
        a = zero.clone().index_add_(0, out_of_pair, w.abs() * s.abs())
        if tot is not None:
            wr = wt[:, rest][:, ch]
            t = t + wr * (tot[cs].unsqueeze(0) - zero.clone().index_add_(0, out_of_pair, s))
            a = a + wr.abs() * (zero.clone().index_add_(0, out_of_pair, s.abs()) + tot[cs].abs().unsqueeze(0))
        truth[:, c0:c0 + cs.numel()], mag[:, c0:c0 + cs.numel()] = t, a
    return truth.numpy(), mag.numpy(), deg.numpy()


def reference(rowptr, col, code, S, lut, cnt=None, s_total=None, reduce_cr=0, hub_threshold=HUB_THRESHOLD, rows=None):
    """``(truth, bound)``, float64 numpy ``[n, W]`` (``[n, reduce_cr]`` with the fused read-out).  ``S`` as the kernel reads it
    (a bf16 operand: its values widened); ``cnt`` None: no shell normalisation; ``s_total`` None: no rest term.
    ``rows``: evaluate these rows only (row ``q`` of the result is row ``rows[q]`` of the graph)."""
    truth, mag, deg = _truth_mag(rowptr, col, code, S, lut, cnt, s_total, rows)
    n, W = truth.shape
    k = np.where(deg > hub_threshold, 2 * deg, deg + 5).astype(np.float64)
    if reduce_cr:
        truth = truth.reshape(n, W // reduce_cr, reduce_cr).sum(1)
        mag = mag.reshape(n, W // reduce_cr, reduce_cr).sum(1)
        k = k + 10
    return truth, gamma(k)[:, None] * mag


def worst_ratio(y, truth, bound):
    """Largest ``|y - t| / bound`` over the elements with a positive bound (inf when any element — one with a zero bound, which must
    be exactly zero, included — fails or is not finite)."""
    y = _t64(y).numpy().reshape(truth.shape)
    err = np.abs(y - truth)
    if not bool(np.all(err <= bound)):              # (a NaN compares false)
        return float("inf")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def assert_within(y, truth, bound, what=""):
    """Every element within its bound; returns the worst ratio."""
    yv = _t64(y).numpy().reshape(truth.shape)
    err = np.abs(yv - truth)
    bad = ~(err <= bound)
    if bad.any():
        i, c = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements outside the per-row bound; first at row {i}, column {c}: "
                             f"got {yv[i, c]!r}, truth {truth[i, c]!r}, |err| {err[i, c]:.3e} > bound {bound[i, c]:.3e}")
    return worst_ratio(y, truth, bound)


def exact_scaled(rowptr, col, code, S, lut, s_total=None, reduce_cr=0, cnt=None, scale=4):
    """The same sum for integer ``S`` and weights ``lut / max(cnt, 1)`` that are multiples of ``1 / scale`` (a power of two), in int64:
    ``(scale t, scale A)`` with ``A`` the magnitude above.  While ``scale A < 2^24`` every product and every partial sum of the float32
    evaluation is a multiple of ``1 / scale`` below ``2^24 / scale``, hence exact in any order: the output must equal ``t``."""
    rowptr, col, code = _idx(rowptr), _idx(col), _idx(code)
    S = _t64(S)
    n, W = rowptr.numel() - 1, S.shape[1]
    lut = _t64(lut).reshape(1, -1)
    rest = lut.shape[1] - 1
    w = lut.expand(n, rest + 1) * scale
    if cnt is not None:
        w = w / _idx(cnt).clamp_min(1).double()
    assert bool((S == S.round()).all()) and bool((w == w.round()).all())
    S, w = S.long(), w.long()
    deg = rowptr[1:] - rowptr[:-1]
    row_of_pair = torch.repeat_interleave(torch.arange(n), deg)
    wp, s = w[row_of_pair, code.clamp_max(rest)].unsqueeze(1), S[col]
    zero = torch.zeros((n, W), dtype=torch.int64)
    t = zero.clone().index_add_(0, row_of_pair, wp * s)
    a = zero.clone().index_add_(0, row_of_pair, wp.abs() * s.abs())
    if s_total is not None:
        tot = _t64(s_total).reshape(-1)
        assert bool((tot == tot.round()).all())
        tot, wr = tot.long(), w[:, rest:rest + 1]
        t = t + wr * (tot.unsqueeze(0) - zero.clone().index_add_(0, row_of_pair, s))
        a = a + wr.abs() * (zero.clone().index_add_(0, row_of_pair, s.abs()) + tot.abs().unsqueeze(0))
    if reduce_cr:
        t, a = t.view(n, W // reduce_cr, reduce_cr).sum(1), a.view(n, W // reduce_cr, reduce_cr).sum(1)
    return t, a


def exact_quarters(rowptr, col, code, S, lut, s_total=None, reduce_cr=0):
    """:func:`exact_scaled` for weights that are multiples of 1/4 and no counts: ``(4 t, 4 A)``."""
    return exact_scaled(rowptr, col, code, S, lut, s_total, reduce_cr, None, 4)


def short_csr(n, rng, D=4, hubs=((7, 600), (1234, 2000), (-1, 513)), self_share=0.8):
    """The degree mix of tests/test_gpu_short_tiles.py for any code count: rows of 0 .. 9 pairs and a few of 30, ``hubs`` =
    (row, pairs); most rows of 1 .. 4 pairs list themselves first (code 0), some do not; the other codes are 1 .. D - 2
    (D = 2: code 0 throughout)."""
    deg = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 30], size=n, p=[.05, .35, .12, .1, .08, .06, .05, .05, .05, .05, .04])
    for r, d in hubs:
        deg[r] = d
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    col = rng.integers(0, n, nnz).astype(np.int32)
    code = (rng.integers(1, D - 1, nnz) if D > 2 else np.zeros(nnz)).astype(np.uint8)
    for i in np.nonzero((deg > 0) & (deg <= 4) & (rng.random(n) < self_share))[0]:
        col[rowptr[i]], code[rowptr[i]] = i, 0
    return rowptr, col, code


def csr_of_degrees(deg, n_cols, rng, D=4):
    """A CSR with exactly these row lengths, random neighbours and codes 0 .. D - 2."""
    deg = np.asarray(deg, dtype=np.int64)
    rowptr = np.zeros(len(deg) + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    nnz = int(rowptr[-1])
    return rowptr, rng.integers(0, n_cols, nnz).astype(np.int32), rng.integers(0, max(D - 1, 1), nnz).astype(np.uint8)


def lanes_per_row(W, vec=4):
    """The lane group of a row of W floats read ``vec`` at a time: the smallest power of two covering it, at most a wavefront."""
    lpr = 1
    while lpr * vec < W and lpr < 64:
        lpr *= 2
    return lpr


def tile_partition(deg, lpr, lmax):
    """The short-row tiles of a degree-sorted copy with these row lengths, restated: run L = the rows of exactly L pairs, a lane
    group takes R_L rows of it (R_0 = 8, R_L = max(1, 8 // L)), a wave 64 / lpr groups, one tile per wave.
    ``(n_tiles, row_q0, first tile of every run)``."""
    deg = np.asarray(deg)
    first, t = [], 0
    for L in range(lmax + 1):
        first.append(t)
        per = (64 // lpr) * (8 if L == 0 else max(1, 8 // L))
        t += -(-int((deg == L).sum()) // per)
    return t, int((deg <= lmax).sum()), first


# =====================================================================================================================================
# The narrow aggregation (W in {1, 2, 4}): csrc/spmm_pb.hip and the narrow row walks of csrc/spmm.hip (spmm_hot_kernel) and csrc/spmm_fwd_body.hpp
# =====================================================================================================================================
# Propagation-blocked forward (pb_expand_kernel + pb_reduce_kernel).  Every operand entry is truncated toward zero to a multiple of
#     q = 2^(e + h - 62),    e = the frexp exponent of the float32 max |S| over ALL rows of S,    h = plan.headroom_bits,
# the integer sums are exact (no term depends on the row length), and fwd_rows evaluates in float32
#     y = fma(w_0 - w_r, S_self, 0) -> fma(w_d - w_r, T_d, .) per accumulated code -> fma(w_r, tot, .) -> + add
# Roundings a term can meet, counted from fwd_rows — K_PB = 10:
#     1  the division l_d / cnt(i, d)                 1  the division l_rest / cnt(i, rest)           1  the fold w_d - w_r
#     2  int64 -> double -> float of the scaled sum   5  the longest chain of fmaf / adds behind a term: self, at most 3 codes less the
#                                                        self code's (D <= 4: self + 2, or 3 without a self pair), rest, the final add
# Bound        |y - t| <= gamma_K A + (1 + gamma_K) sum_{d accumulated} |w(i, d) - w_rest(i)| L_{i,d} q
#              A as in the header (it bounds the folded form sum_d |w_d - w_r| |T_d| + |w_r| |tot| too); L_{i,d} = the pairs of row i
#              with code d that go through the accumulators (the self pair of code 0 does not when code_base == 1).  The fold's own
#              rounding times the quantisation term is of second order (<= 3 u (|w_d| + |w_r|) L q) and is left out.
#              An all-zero operand has no quantisation term (to_fixed(0) = 0).
K_PB = 10
K_BWD = 10                         # the narrow backward's constant: see narrow_bwd_reference
K_DLUT = 6
LONG_ROW_THRESHOLD_NARROW = 64     # graph.LONG_ROW_THRESHOLD_NARROW (tests/test_narrow_bound.py holds the two equal)


def pb_shift(S, headroom_bits):
    """``(shift, q)`` of pb_reduce_kernel for the operand ``S``: ``shift = 62 - h - e``, ``q = 2^-shift`` (0 for an all-zero operand)."""
    s32 = np.asarray(_t64(S).numpy(), dtype=np.float32)
    mx = float(np.abs(s32).max()) if s32.size else 0.0
    assert np.isfinite(mx)
    e = int(np.frexp(np.float32(mx))[1]) if mx > 0.0 else 0
    shift = 62 - int(headroom_bits) - e
    return shift, (2.0 ** -shift if mx > 0.0 else 0.0)


def to_fixed(v, shift):
    """``to_fixed`` of csrc/spmm_pb.hip in integer arithmetic on a float32 array: mantissa and exponent, truncation toward zero, a zero
    exponent field read as exponent 1 without the implicit bit."""
    b = np.ascontiguousarray(np.asarray(v, dtype=np.float32)).view(np.uint32).astype(np.int64)
    ex = (b >> 23) & 0xff
    m = (b & 0x7fffff) | np.where(ex != 0, 0x800000, 0)
    sh = np.where(ex != 0, ex, 1) - 150 + int(shift)
    up, down = np.clip(sh, 0, 62), np.clip(-sh, 0, 63)
    x = np.right_shift(np.left_shift(m, up), down)
    return np.where((b >> 31) != 0, -x, x)


def _pairs(rowptr, col, code):
    rowptr, col, code = (np.asarray(_idx(v).numpy()) for v in (rowptr, col, code))
    return rowptr, col, code, np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))


def _weights(lut, cnt, n):
    lut = _t64(lut).numpy().reshape(1, -1)
    w = np.broadcast_to(lut, (n, lut.shape[1])).copy()
    if cnt is not None:
        w = w / np.maximum(np.asarray(_idx(cnt).numpy()), 1).astype(np.float64)
    return w


def pb_reference(rowptr, col, code, S, lut, cnt, s_total, headroom_bits, code_base):
    """``(truth, bound)`` float64 ``[n, W]`` of ``gnan_spmm_pb_fwd``: see the comment above (K = 10, counted from fwd_rows)."""
    truth, mag, _ = _truth_mag(rowptr, col, code, S, lut, cnt, s_total)
    rowptr, col, code, row = _pairs(rowptr, col, code)
    n = len(rowptr) - 1
    w = _weights(lut, cnt, n)
    D = w.shape[1]
    wr = w[:, D - 1] if s_total is not None else np.zeros(n)
    _, q = pb_shift(S, headroom_bits)
    acc = code >= code_base
    L = np.zeros((n, D))
    np.add.at(L, (row[acc], np.minimum(code[acc], D - 1)), 1.0)
    quant = (np.abs(w - wr[:, None])[:, :D - 1] * L[:, :D - 1]).sum(1) * q
    g = float(gamma(K_PB))
    return truth, g * mag + (1.0 + g) * quant[:, None]


def pb_shell_exact(rowptr, col, code, S, headroom_bits, code_base):
    """The float32 ``[n]`` that ``shell_out`` must hold BIT FOR BIT (W == 1, one accumulated code):
    ``float32(float64(sum_l to_fixed(S[col_l], shift)) * 2^-shift)`` over the pairs that go through the accumulators.
    (An operand of W > 1 columns: ``[n, W]``, every column with the whole operand's shift, as the kernel's accumulators hold them.)"""
    rowptr, col, code, row = _pairs(rowptr, col, code)
    s = np.asarray(_t64(S).numpy(), dtype=np.float32)
    s = s.reshape(-1, 1) if s.ndim == 1 else s
    shift, _ = pb_shift(s, headroom_bits)
    acc = code >= code_base
    t = np.zeros((len(rowptr) - 1, s.shape[1]), dtype=np.int64)
    np.add.at(t, row[acc], to_fixed(s[col[acc]], shift))
    out = (t.astype(np.float64) * np.ldexp(1.0, -shift)).astype(np.float32)
    return out[:, 0] if s.shape[1] == 1 else out


def narrow_bwd_reference(rowptr, col, code, S, lut, cnt, dY, s_total, route, headroom_t=0, code_base=0, headroom_f=0, magnitudes=None):
    """``(dS_truth, dS_bound, dlut_truth, dlut_bound)`` (float64: ``[n_cols, W]`` twice, ``[D]`` twice) of the narrow aggregation's
    backward, ``s_total`` (the float32 total the forward was handed; None: no rest bucket) taken as the column sums of ``S``.

        dS[j]   = sum_{i lists j with code d} (w(i,d) - w_r(i)) dY_i  +  sum_i w_r(i) dY_i            (the last sum: rest bucket only)
        M[j]    = sum_{i lists j} (|w(i,d)| + |w_r(i)|) |dY_i|  +  |lut_r| sum_i |dY_i| / cnt(i, rest)
        dlut[d] = sum_i a_{i,d} T[i,d],   a_{i,d} = dY_i / max(cnt(i,d), 1);      dlut[rest] = sum_i a_{i,rest} (tot - sum_d T[i,d])

    ``magnitudes``: a list that receives ``M [n_cols, W]`` and the table gradient's sums of |terms| ``[D]``.
    ``route`` names the kernels that ran; every constant is counted from them:

    'rows'  gnan_spmm_bwd_narrow (spmm_lut_grad_kernel<BWD> / spmm_bwd_hot_kernel, bwd_finish) over the transposed graph: a float chain
            over the L_j pairs that list j.  A term meets 1 division (pack_bwd_rows), <= L_j chain adds, 3 adds over the codes (the rest
            half), <= 4 fmaf with the table, 1 add of the rest vector, whose own value is a float64 sum cast (1) times lut_r (1):
            k_j = L_j + 10; rows of more than 64 pairs (LONG_ROW_THRESHOLD_NARROW) are cut into slices: k_j = 2 L_j, as ``reference``.
            dS bound  gamma_{k_j} M[j].   dlut: the chain runs over the TRANSPOSED row, so the pair (i, j) carries k_j, not k_i:
            sum_{pairs of code d} gamma_{k_j} |a_{i,d}| |S_j|  (+ gamma_6 |tot| sum_i |a_{i,rest}| for the rest code; the fmaf with
            S_j, the lane and float64 block sums and the final cast are inside the 10).
    'pb1'   gnan_spmm_pb_pack1 + the two PB phases over the transposed graph with the operand c_i = l_1 a_{i,1} - l_r a_{i,r}
            (W = 1, a table of ones, e for the self pairs, q l_r added).  Per term: 2 divisions, the product l_r a_r, the fmaf that
            forms c (4), int64 -> double -> float (2), two fmaf and the final add (3): K = 10 >= 9.  The operand in the buckets is c:
            dS bound  gamma_10 M[j] + (1 + gamma_10) L_j 2 q_c,  L_j = the accumulated pairs listing j, q_c = 2^(e_c + h_t - 62) —
            TWICE q_c because e_c is restated from the float64 c, which can sit on the other side of a power of two from the kernel's
            float32 one.   dlut: the terms are the forward's kept shell sums times a_{i,d} in float64 (1 division, 2 for the kept
            float32 sum, the final cast; K_DLUT = 6), and the kept sums carry the FORWARD's truncation:
            gamma_6 sum_i |a_{i,d}| sum_l |S_l|  +  sum_i |a_{i,d}| L_{i,d} q_S   (q_S from S and the forward plan's headroom h_f).
    'pb2'   gnan_spmm_pb_bwd: the packed rows V[code_base] = [a_{i,d1} | a_{i,r}] (W = 2) through the buckets, a table of ones; bwd_rows:
            1 division, 2 conversion, the add of the self pair's rest half, l_0 a_0, two fmaf, the final add (<= 8 <= K = 10).
            dS bound  gamma_10 M[j] + (1 + gamma_10) (|l_d1| + |l_r|) L_j 2 q_V   (2 q_V as above: V is a float32 quotient).
            dlut: float64 sums of S_j times the scaled integer sums: gamma_6 sum_pairs |a_{i,d}| |S_j| + sum_j |S_j| L_j 2 q_V.
    """
    rowptr, col, code, row = _pairs(rowptr, col, code)
    n = len(rowptr) - 1
    S, dY = _t64(S).numpy(), _t64(dY).numpy()
    n_cols, W = S.shape
    w = _weights(lut, cnt, n)
    lutv = _t64(lut).numpy().reshape(-1)
    D, rest = w.shape[1], w.shape[1] - 1
    with_rest = s_total is not None
    wr = w[:, rest] if with_rest else np.zeros(n)
    inv = 1.0 / np.maximum(np.asarray(_idx(cnt).numpy()), 1) if cnt is not None else np.ones((n, D))
    cd = np.minimum(code, rest)
    # ---- operand gradient
    dS = np.zeros((n_cols, W))
    np.add.at(dS, col, (w[row, cd] - wr[row])[:, None] * dY[row])
    M = np.zeros((n_cols, W))
    np.add.at(M, col, (np.abs(w[row, cd]) + np.abs(wr[row]))[:, None] * np.abs(dY[row]))
    if with_rest:
        dS += (wr[:, None] * dY).sum(0)[None, :]
        M += abs(lutv[rest]) * (inv[:, rest:rest + 1] * np.abs(dY)).sum(0)[None, :]
    # ---- table gradient, pair by pair
    a = inv[:, :, None] * dY[:, None, :]                                  # [n, D, W]
    pair_t = a[row, cd] * S[col]                                          # [pairs, W]: a_{i,d} S_j
    pair_m = np.abs(a[row, cd]) * np.abs(S[col])
    dlut = np.zeros(D)
    np.add.at(dlut, cd, pair_t.sum(1))
    tot = _t64(s_total).numpy().reshape(-1) if with_rest else np.zeros(W)
    rest_m = np.abs(a[row, rest]) * np.abs(S[col])                        # the rest code sees every listed pair
    if with_rest:
        dlut[rest] = float((a[:, rest] * tot[None, :]).sum() - (a[row, rest] * S[col]).sum())
    tot_m = float((np.abs(a[:, rest]) * np.abs(tot)[None, :]).sum()) if with_rest else 0.0
    if magnitudes is not None:
        dl_mag = np.zeros(D)
        np.add.at(dl_mag, cd, pair_m.sum(1))
        if with_rest:
            dl_mag[rest] = float(rest_m.sum()) + tot_m
        magnitudes += [M, dl_mag]
    Lt = np.bincount(col, minlength=n_cols).astype(np.float64)            # pairs listing j
    acc = code >= code_base
    Lt_acc = np.bincount(col[acc], minlength=n_cols).astype(np.float64)
    dl_bound = np.zeros(D)
    if route == "rows":
        kj = np.where(Lt > LONG_ROW_THRESHOLD_NARROW, 2 * Lt, Lt + K_BWD)
        dS_bound = gamma(kj)[:, None] * M
        np.add.at(dl_bound, cd, (gamma(kj)[col][:, None] * pair_m).sum(1))
        if with_rest:
            dl_bound[rest] = float((gamma(kj)[col][:, None] * rest_m).sum()) + float(gamma(K_DLUT)) * tot_m
    elif route in ("pb1", "pb2"):
        g, gd = float(gamma(K_BWD)), float(gamma(K_DLUT))
        d1 = code_base
        if route == "pb1":
            c = lutv[d1] * a[:, d1] - (lutv[rest] * a[:, rest] if with_rest else 0.0)
            _, qc = pb_shift(c.astype(np.float32), headroom_t)
            quant = Lt_acc * 2.0 * qc
        else:
            V = np.concatenate([a[:, d1], a[:, rest] if with_rest else np.zeros((n, W))], axis=1)
            _, qv = pb_shift(V.astype(np.float32), headroom_t)
            quant = (abs(lutv[d1]) + (abs(lutv[rest]) if with_rest else 0.0)) * Lt_acc * 2.0 * qv
        dS_bound = g * M + (1.0 + g) * quant[:, None]
        np.add.at(dl_bound, cd, gd * pair_m.sum(1))
        if with_rest:
            dl_bound[rest] = gd * (float(rest_m.sum()) + tot_m)
        if route == "pb1":
            _, qs = pb_shift(S, headroom_f)
            qa = np.zeros(D)
            np.add.at(qa, cd[acc], np.abs(a[row[acc], cd[acc]]).sum(1) * qs)
            dl_bound += qa
            if with_rest:
                dl_bound[rest] += float(np.abs(a[row[acc], rest]).sum()) * qs
        else:
            sq = float((np.abs(S).sum(1) * Lt_acc).sum()) * 2.0 * qv
            dl_bound[d1] += sq
            if with_rest:
                dl_bound[rest] += sq
    else:
        raise ValueError(route)
    return dS, dS_bound, dlut, dl_bound


# ---- the graphs and operands of the narrow cases (tests/test_narrow_bound.py on the CPU, tests/test_gpu_narrow_rows.py on the GPU) ----
NARROW_HUBS = ((5, 64), (101, 65), (333, 128), (402, 129), (650, 150))     # (row, accumulated pairs): slot (8 per slot) and headroom edges
NARROW_LAYOUTS = ("self", "some", "moved", "none", "double")
NARROW_FAMILIES = ("unit", "range", "outlier", "same-sign", "same-sign-neg")
# (D, W, self-pair layout, use_cnt, with_rest, longest hub, (n_rows, n_cols)): every D x W, every layout, counts and rest on and off,
# every hub length as the graph's longest (headroom_bits 6, 7, 7, 8, 8), both shapes
NARROW_CASES = [
    (3, 1, "self", True, True, 150, (700, 900)), (3, 1, "self", False, False, 64, (700, 900)), (3, 1, "moved", True, True, 65, (900, 800)),
    (3, 1, "some", True, False, 128, (700, 900)), (3, 1, "none", True, True, 129, (700, 900)), (2, 1, "self", True, True, 150, (700, 900)),
    (2, 1, "self", False, True, 65, (900, 800)), (3, 2, "self", False, True, 150, (700, 900)), (3, 2, "some", True, True, 129, (900, 800)),
    (3, 4, "moved", True, False, 128, (700, 900)), (4, 1, "self", True, False, 150, (700, 900)), (4, 1, "double", True, True, 64, (700, 900)),
    (4, 2, "none", True, True, 65, (900, 800)), (4, 4, "self", True, True, 150, (700, 900)), (4, 4, "none", False, True, 129, (700, 900)),
    (2, 2, "self", True, False, 128, (700, 900)), (2, 4, "self", True, True, 64, (900, 800)), (3, 4, "self", True, True, 150, (900, 800)),
]


def narrow_csr(rng, n_rows, n_cols, D, layout="self", top_hub=150, hub_share=0.35, hubs=None, reserve=True):
    """``test_pb_plan.random_graph`` with hub rows of exactly 64 .. ``top_hub`` accumulated pairs, empty rows, ``hub_share`` of the
    pairs behind code 0 on six columns (hub rows of the transposed graph; the hot rows of the row walks) and one of the self-pair
    layouts: 'self' every row lists itself with code 0; 'some' a fifth of the rows has no code-0 pair; 'moved' a tenth of the code-0
    pairs points at another column; 'none' no code-0 pair at all; 'double' one row has two (code 0 is bucketed like any other).
    ``reserve``: column ``n_cols - 1`` is listed by no pair (the 'outlier' operand family puts its large row there)."""
    from test_pb_plan import random_graph
    hubs = [(r, d) for r, d in (NARROW_HUBS if hubs is None else hubs) if d <= top_hub]
    _, rowptr, col, code = random_graph(rng, n_rows, n_cols, D, hubs=hubs, self_pairs=layout != "none")
    col, code = col.copy(), code.copy()
    row = np.repeat(np.arange(n_rows), np.diff(rowptr))
    keep = np.ones(len(col), dtype=bool)
    is0 = (code == 0) & (D > 2)
    other = np.nonzero(~is0 & (rng.random(len(col)) < hub_share))[0]
    col[other] = rng.integers(0, 6, len(other)) * ((n_cols - 1) // 6)
    if layout == "some":
        keep &= ~(is0 & (rng.random(n_rows) < 0.2)[row])
    elif layout == "moved":
        moved = np.nonzero(is0 & (rng.random(len(col)) < 0.1))[0]
        col[moved] = rng.integers(0, n_cols, len(moved))
    elif layout == "double" and D > 2:
        e = int(np.nonzero(~is0)[0][0])                                   # (its row lists itself with code 0 already)
        code[e] = 0
    if reserve:
        col[col == n_cols - 1] = n_cols - 2
    deg = np.bincount(row[keep], minlength=n_rows)
    rowptr = np.zeros(n_rows + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(deg)
    return rowptr, col[keep].astype(np.int32), code[keep].astype(np.uint8)


def narrow_operand(rng, family, n_cols, W):
    """float32 ``[n_cols, W]``.  'unit' 3 N(0,1); 'range' every row times 2^k, k uniform in [-40, 10]; 'outlier' the unit operand with
    2^60 in the row no pair lists (absmax is taken over the WHOLE operand: the small rows may lose every digit — that is the
    contract); 'same-sign' every entry the float just below 2 (row sums L max |S|, the most the headroom must hold — it cannot
    see a headroom one bit short: the accumulators are scaled to 2^62 and an int64 has one more bit) and its negated copy;
    'zeros'; 'integers' in [-4, 4]."""
    S = (rng.standard_normal((n_cols, W)) * 3.0).astype(np.float32)
    if family == "range":
        S = (S * np.exp2(rng.integers(-40, 11, (n_cols, 1)).astype(np.float64))).astype(np.float32)
    elif family == "outlier":
        S[n_cols - 1] = np.float32(2.0 ** 60)
    elif family in ("same-sign", "same-sign-neg"):
        S[:] = np.nextafter(np.float32(2.0), np.float32(0.0))
        S = -S if family.endswith("neg") else S
    elif family == "zeros":
        S[:] = 0.0
    elif family == "integers":
        S = rng.integers(-4, 5, (n_cols, W)).astype(np.float32)
    elif family != "unit":
        raise ValueError(family)
    return S
