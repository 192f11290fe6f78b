"""TEST INFRASTRUCTURE ONLY (never imported by the product path).

References and inputs for the bootstrap of the per-group metrics: fr_bootstrap_group_sums (csrc/bootstrap.hip), fr_topk_user_terms
and fr_gauc_user_terms (csrc/metrics.hip), fairrec.evaluator.bootstrap_intervals and the `group_bootstrap` keys of the Evaluator.
tests/test_bootstrap_ref.py pins what is here on the CPU; tests/test_bootstrap_hip.py compares the kernels with it.

  philox4x32_10   Philox4x32-10 (Salmon et al., SC'11) in numpy uint64 arithmetic
  T, weight_of    the twelve thresholds floor(2^32 e^-1 sum_{i <= j} 1 / i!) and w = #{j : word >= T[j]}
  weights         w(r, b) int64 [len(rows), B] by the contract of include/fairrec_hip.h
  group_sums_ref  the weighted sums per (group, replicate, column), each the EXACT sum rounded once: w x = the sum of x 2^i over
                  the set bits of w, every term exact in float64, added by math.fsum; with the sums of w |x| a tolerance needs
  topk_user_terms_ref / gauc_user_terms_ref   the per-user terms, restated from metrics_ref / group_metrics_ref
  replicate_stats, intervals_ref              the statistic of every replicate and the percentile intervals, the quantile
                  written out (sorted values, linear interpolation) instead of called

Tolerances (u = 2^-53, gamma_n = n u / (1 - n u)):
  * weight sums: exact integers.
  * sums: the kernel rounds every product into its accumulator (a fused multiply-add, or a multiplication and an addition) and adds
    per-chunk partials: no summand passes through more than n_g roundings, whatever the order, and the reference rounds once:
    gamma_(n_g + 1) * sum w |x| per (group, replicate, column).  NaN positions and entries with a zero bound: exact.
  * a replicate statistic sum / weight (non-negative terms, an exact integer weight): gamma_(n_g + 2) relative -- the sum, the
    division, the reference.  GAUC's quotient of two such sums, the numerator's terms auc_u * pos_len carrying the kernel's
    division and multiplication against the reference's one rounding: gamma_(2 n_g + 6) relative.  A quantile moves by at most
    the largest bound among its usable replicates plus 2 u |q| (the interpolation); a gap by the sum of two groups' bounds.
"""
import math
from decimal import Decimal, getcontext

import numpy as np

import group_metrics_ref as GR
import metrics_ref as R

U64 = R.U64
NAN = float("nan")
M32 = np.uint64(0xFFFFFFFF)

# the kernel's shape constants (csrc/bootstrap.hip), which the GPU shapes are chosen around
ROW_TILE = 64                # BS_ROWS: positions staged in LDS at a time
REP_TILE = 1024              # BS_REP_TILE: replicates of one workgroup (256 lanes x 4)
COL_TILE = 8                 # BS_COLS
MAX_CHUNKS = 2048            # BS_MAX_CHUNKS
MAX_COLS, MAX_REP = 64, 65536

T = (0x5e2d58d8, 0xbc5ab1b1, 0xeb715e1d, 0xfb239797, 0xff1025f5, 0xffd90f3b, 0xfffa8b71, 0xffff540c, 0xffffed1f, 0xfffffe21,
     0xffffffd4, 0xfffffffc)


def chunk_len(n_rows):
    """positions per chunk: 64 * ceil(n_rows / (64 * MAX_CHUNKS))"""
    return 64 * ((n_rows + 64 * MAX_CHUNKS - 1) // (64 * MAX_CHUNKS))


def workspace_bytes(n_rows, n_cols, n_groups, n_rep):
    """the formula include/fairrec_hip.h states"""
    L = chunk_len(n_rows)
    blocks = (n_rows + L - 1) // L + n_groups
    return (blocks * n_rep * (n_cols + 1) + n_groups + 1) * 8


def thresholds_from_decimal():
    """T[j] = floor(2^32 e^-1 sum_{i <= j} 1 / i!) with 50 significant digits"""
    getcontext().prec = 50
    e_inv = 1 / Decimal(1).exp()
    out, cdf, fact = [], Decimal(0), Decimal(1)
    for j in range(12):
        if j:
            fact *= j
        cdf += 1 / fact
        out.append(int((Decimal(2) ** 32 * e_inv * cdf).to_integral_value(rounding="ROUND_FLOOR")))
    return tuple(out)


def philox4x32_10(counter, key):
    """counter: four arrays (or integers) of 32-bit words, key: two -> the four output words as uint64 arrays below 2^32"""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = (np.uint64(int(x) & 0xFFFFFFFF) for x in key)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M32, p1 >> np.uint64(32), p1 & M32
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0 = (k0 + np.uint64(0x9E3779B9)) & M32
        k1 = (k1 + np.uint64(0xBB67AE85)) & M32
    return c


def weight_of(word):
    """w = the number of j with word >= T[j]"""
    word = np.asarray(word, dtype=np.uint64)
    return sum((word >= np.uint64(t)).astype(np.int64) for t in T)


def weights(rows, n_rep, seed):
    """int64 [len(rows), n_rep]: w(r, b) from word b & 3 of philox(counter = (r, 0, b >> 2, 0), key = (seed low, seed high))"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1, 1)
    quads = np.arange((n_rep + 3) // 4, dtype=np.uint64).reshape(1, -1)
    words = philox4x32_10((rows, 0, quads, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack([weight_of(x) for x in words], axis=2).reshape(rows.shape[0], -1)       # [rows, quads * 4], b = 4 quad + word
    return np.ascontiguousarray(w[:, :n_rep])


def _exact_weighted_sum(w, x):
    """sum_r w[r] x[r] rounded once (w integers in 0..15, x finite float64): x 2^i is exact, fsum adds exactly"""
    terms = [x[(w >> i) & 1 == 1] * float(1 << i) for i in range(4)]
    return math.fsum(np.concatenate(terms).tolist())


def group_sums_ref(values, perm, start, n_rep, seed, with_abs=True):
    """(sums float64 [G, B, C], weight int64 [G, B], absw float64 [G, B, C] = sum w |x|, sizes [G]); a non-finite value makes its
    (group, column) NaN in every replicate.  with_abs=False (non-negative values: absw = sums) leaves absw None."""
    values = np.asarray(values, dtype=np.float64)
    G, C = len(start) - 1, values.shape[1]
    sums, absw = np.zeros((G, n_rep, C)), np.zeros((G, n_rep, C))
    weight = np.zeros((G, n_rep), dtype=np.int64)
    for g in range(G):
        rows = GR.members(perm, start, g)
        if not len(rows):
            continue
        w = weights(rows, n_rep, seed)
        weight[g] = w.sum(axis=0)
        for c in range(C):
            x = values[rows, c]
            if not np.isfinite(x).all():
                sums[g, :, c] = absw[g, :, c] = NAN
                continue
            for b in range(n_rep):
                sums[g, b, c] = _exact_weighted_sum(w[:, b], x)
                if with_abs:
                    absw[g, b, c] = _exact_weighted_sum(w[:, b], np.abs(x))
    return sums, weight, absw if with_abs else None, np.diff(np.asarray(start))


def sums_tolerance(absw, sizes):
    """gamma_(n_g + 1) * sum w |x|"""
    return np.array([R.gamma(int(n) + 1) for n in sizes])[:, None, None] * absw


# ---- the per-user terms ----------------------------------------------------------------------------------------------------------

TOPK_NAMES = ("hit", "mrr", "ndcg", "recall", "precision", "map")


def topk_user_terms_ref(rec, columns):
    """float64 [U, C]: row u's term of metric columns[j][0] at cut-off columns[j][1] = metrics_ref.topk_metrics_ref of that one
    row (a mean over one row)"""
    rec = np.asarray(rec)
    out = np.zeros((rec.shape[0], len(columns)))
    for u in range(rec.shape[0]):
        one = R.topk_metrics_ref(rec[u:u + 1])
        out[u] = [one[TOPK_NAMES.index(m), k - 1] for m, k in columns]
    return out


def gauc_user_terms_ref(meanrank):
    """float64 [U, 2]: (auc_u * pos_len, pos_len) of a kept user from the exact rational of group_metrics_ref.gauc_user, (0, 0) of a
    user without a positive or without a negative"""
    out = np.zeros((len(meanrank), 2))
    for u, row in enumerate(np.asarray(meanrank)):
        two_rank, user_len, pos_len = (int(x) for x in row)
        if pos_len != 0 and user_len != pos_len:
            out[u] = float(GR.gauc_user(two_rank, user_len, pos_len) * pos_len), float(pos_len)
    return out


# ---- statistics and intervals ----------------------------------------------------------------------------------------------------

def replicate_stats(num, den):
    """num / den per (group, replicate), NaN where the denominator is zero"""
    num, den = np.asarray(num, dtype=np.float64), np.asarray(den, dtype=np.float64)
    out = np.full(num.shape, NAN)
    nz = den != 0
    out[nz] = num[nz] / den[nz]
    return out


def quantile_linear(x, q):
    """the q-quantile of the values x by linear interpolation between the order statistics at floor and ceil of q (n - 1)"""
    x = sorted(float(v) for v in x)
    pos = q * (len(x) - 1)
    lo = int(math.floor(pos))
    hi = min(lo + 1, len(x) - 1)
    return x[lo] + (x[hi] - x[lo]) * (pos - lo)


def intervals_ref(stat, level):
    """(low [G], high [G], gap_low, gap_high, usable [G], gap_usable) as fairrec.evaluator.bootstrap_intervals documents them"""
    stat = np.asarray(stat, dtype=np.float64)
    G, B = stat.shape
    ql, qh = (1 - level) / 2, (1 + level) / 2
    low, high, usable = [], [], []
    for g in range(G):
        vals = [v for v in stat[g] if math.isfinite(v)]
        usable.append(len(vals))
        ok = 2 * len(vals) >= B
        low.append(quantile_linear(vals, ql) if ok else NAN)
        high.append(quantile_linear(vals, qh) if ok else NAN)
    gaps = [max(col) - min(col) for col in stat.T if all(math.isfinite(v) for v in col)]
    ok = 2 * len(gaps) >= B
    return (np.array(low), np.array(high), quantile_linear(gaps, ql) if ok else NAN, quantile_linear(gaps, qh) if ok else NAN,
            np.array(usable), len(gaps))


# ---- the inputs of the tests -----------------------------------------------------------------------------------------------------

N_REPS = [1, 3, 4, 5, 63, 64, 65, 257, REP_TILE + 1]         # the Philox quad, the wave, the replicate tile of a workgroup
N_COLS = [1, 7, 8, 9, 64]                                    # the column tile
GROUP_COUNTS = [(1, 65), (2, 129), (9, 200), (70, 70)]       # (G, U)
LONG_ROWS = 64 * MAX_CHUNKS + 1                              # the smallest n_rows whose chunks are 128 positions = two row tiles
LONG_SIZES = [127, 128, 129, 257]                            # CH - 1, CH, CH + 1, 2 CH + 1 at that chunk length; the rest: one group


def values_case(n_rows, n_cols, seed=0):
    """float64 [n_rows, n_cols]: both signs, magnitudes over six decades, exact zeros"""
    rng = np.random.default_rng([n_rows, n_cols, seed, 53])
    v = rng.standard_normal((n_rows, n_cols)) * 10.0 ** rng.integers(-3, 4, (n_rows, n_cols))
    v[rng.random((n_rows, n_cols)) < 0.05] = 0.0
    return v
