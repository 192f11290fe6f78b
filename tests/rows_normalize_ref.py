"""float64 restatement of fr_rows_l2_normalize (include/fairrec_hip.h, csrc/rows_normalize.hip), for the tests.

    n = sqrt(sum_c x[c]^2),  d = fmax(n, eps),  y = x / d,  norm_out = n

with fmax as C's fmaxf (a NaN norm gives d = eps) and a sum of squares beyond fp32's range taken as infinite, as the fp32
entry finds it.  `eps` is used as given: a caller that compares against the fp32 entry passes float(np.float32(eps)), the
value the entry receives.

The rounding bounds come from the entry's contract, to first order in u = 2^-24: a lane's fmaf chain over its E =
ceil(D / 64) columns rounds E times and the butterfly sum six more, each relative to a partial sum of non-negative terms
that is at most the total, so the sum of squares is off by at most (E + 6) u.  The square root halves that and rounds once;
the quotient carries the norm's error and rounds once more: ((E + 6) / 2 + 2) u <= 7 u for D <= 256.  The tests assert
8 u |y| + 2^-149 for the rows (the last term: an output in the subnormal range is a multiple of 2^-149) and, for the norm,
(E + 7) / 2 u -- half a unit below the worst case (E + 6) / 2 + 1, which every one of the E + 7 roundings would have to hit
at its extreme and with one sign.
"""
import numpy as np

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)


def frags(D):
    return (int(D) + 63) // 64


def normalize64(x, eps=1e-8):
    """(y [M, D], n [M]) in float64 of an fp32 (or any) matrix."""
    x64 = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        s = (x64 * x64).sum(axis=1)
        s = np.where(s > FLT_MAX, np.inf, s)         # (NaN compares false and stays)
        n = np.sqrt(s)
        d = np.fmax(n, float(eps))                   # fmaxf: the operand that is not NaN
        y = x64 / d[:, None]
    return y, n


def y_bound(y_ref):
    """|y - y_ref| allowed per element (finite y_ref)."""
    return 8.0 * U * np.abs(y_ref) + 2.0 ** -149


def norm_bound(n_ref, D):
    """|n - n_ref| allowed per row (finite n_ref)."""
    return (frags(D) + 7) / 2.0 * U * np.abs(n_ref)
