"""CPU reference of fr_exposure_grouped (csrc/exposure.hip) and of evaluator.group_exposure_metrics: per group of users the
counts of every item by np.bincount over the group's rows, the five integer sums as Python integers, the entropy sum cell by
cell in np.longdouble; the case builders of tests/test_exposure_by_group_hip.py; the entropy bound.

Per (group g, cut-off k): the entries are the first min(k, K) columns of the group's rows of `items` [U, K]; c[i] = how often item
i occurs among them (a padded list repeats item 0: every occurrence counts); n_g = the group's users, T = n_g * k (k as given,
also beyond K).
  m   = #{i: c[i] > 0}
  S   = sum over the N items sorted ascending by c of (2 idx - N - 1) c, idx 1-based (GiniIndex's numerator)
  pop = sum over the entries of popular[item], tl with tail, cnt with count_items
  entropy = sum over the items with c > 0 of -(c / T) log(c / T)

The entropy bound.  The kernel adds, per DISTINCT count value c of the (g, k), one term h[c] * (-(q log q)), q = c / T, in double:
a quotient, a logarithm, two products -- and then D - 1 additions of non-negative terms, D = the distinct counts (the cells above
n_g, which the kernel adds one by one, counted one each).  With every term non-negative the additions cost at most (D - 1) u of
the sum, and each term's own chain (the quotient, the two products), the final division of the host and the reference's rounding
to double one u each: 5 u; the logarithm E_LOG u.  Bound: (D + 5 + E_LOG) * 2^-53 * sum |term|.
E_LOG: the double-precision logarithm of the device has no accuracy statement at hand; it was measured on an MI355X over the
arguments q of these very cases (torch.log on the device against np.longdouble): E_LOG_MEASURED ulp, rounded up to the next integer
plus one ulp, because the library's logarithm is compiled apart from torch's kernel.

The three per-entry means against `_mean_at_k` (cumsum / k per user, then a mean over users): the prefix sums are exact integers,
the division by k rounds once per user and k, the mean of n_g non-negative terms adds n_g - 1 roundings and one division:
|mean - exact| <= gamma_(n_g + 1) |exact|, and float(Fraction(sum, n_g k)) is within u / 2 of exact: mean_tolerance = gamma_(n_g + 2).
"""
import functools
from fractions import Fraction

import numpy as np

U64 = 2.0 ** -53
E_LOG_MEASURED = 0.5034  # ulp, at q = 0.08444444444444445, over the 928 distinct arguments of kernel_cases() (numpy on the host: 0.4995)
E_LOG = 2                # ceil(E_LOG_MEASURED) + 1
C0 = 5

CHUNK_SIZES = [1, 63, 64, 65, 129, 257]          # group sizes: counts, hence histogram slots, at and across any chunk up to 256
CHUNK_SHAPES = [(1, [1]), (20, [5, 10, 20]), (62, [1, 2, 31, 62])]       # (K, ks)
GROUP_COUNTS = [(1, 70), (2, 100), (3, 120), (9, 200), (70, 70)]         # (G, U), K = 10
GROUP_K, GROUP_KS = 10, [5, 10]
N_ITEMS = 97


def gamma(n):
    return n * U64 / (1 - n * U64)


def mean_tolerance(n_g):
    return gamma(n_g + 2)


def segments(gidx, G):
    """group_start [G + 1]: the users per group, cumulative"""
    return np.concatenate(([0], np.cumsum(np.bincount(gidx, minlength=G)[:G]))).astype(np.int64)


def sorted_keys(items, gidx, N):
    """the keys (g * N + item) * K + rank of every list entry, ascending"""
    U, K = items.shape
    keys = (gidx.astype(np.int64)[:, None] * N + items.astype(np.int64)) * K + np.arange(K, dtype=np.int64)
    return np.sort(keys.reshape(-1))


def item_tables(N, seed=5):
    """popular / tail flags (uint8) and training counts (int64) over the catalogue; item 0 ([PAD]) has count 0"""
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 4000, N).astype(np.int64)
    counts[0] = 0
    order = np.argsort(counts)
    popular, tail = np.zeros(N, dtype=np.uint8), np.zeros(N, dtype=np.uint8)
    popular[order[-max(N // 10, 1):]] = 1
    tail[order[1:1 + max(N // 5, 1)]] = 1
    return popular, tail, counts


def group_ref(items, gidx, G, N, ks, popular=None, tail=None, counts=None):
    """-> out_i [G][n_k][5] Python integers, entropy [G][n_k] np.longdouble (NaN for an empty group), info [G][n_k] = (D, sum of
    |term| as float): what the entropy bound needs"""
    U, K = items.shape
    out_i, ent, info = [], [], []
    for g in range(G):
        rows = items[gidx == g]
        n_g = rows.shape[0]
        oi, oe, oinfo = [], [], []
        for k in ks:
            if n_g == 0:
                oi.append([0, 0, 0, 0, 0])
                oe.append(np.longdouble("nan"))
                oinfo.append((0, 0.0))
                continue
            part = rows[:, :min(k, K)].reshape(-1)
            c = np.bincount(part, minlength=N)
            assert c.shape[0] == N
            srt = sorted(int(x) for x in c)
            S = sum((2 * idx - N - 1) * x for idx, x in enumerate(srt, 1))
            m = int((c > 0).sum())
            pop = int(popular[part].astype(np.int64).sum()) if popular is not None else 0
            tl = int(tail[part].astype(np.int64).sum()) if tail is not None else 0
            cnt = int(counts[part].sum()) if counts is not None else 0
            T = np.longdouble(n_g * k)
            p = c[c > 0].astype(np.longdouble) / T
            terms = -p * np.log(p)
            inside = c[(c > 0) & (c <= n_g)]
            D = len(set(inside.tolist())) + int((c > n_g).sum())
            oi.append([m, S, pop, tl, cnt])
            oe.append(terms.sum(dtype=np.longdouble))
            oinfo.append((D, float(np.abs(terms).sum(dtype=np.longdouble))))
        out_i.append(oi)
        ent.append(oe)
        info.append(oinfo)
    return out_i, np.array(ent, dtype=np.longdouble), info


def entropy_bound(info):
    """[G][n_k] doubles: (D + C0 + E_LOG) 2^-53 sum |term|"""
    return np.array([[(D + C0 + E_LOG) * U64 * s for D, s in row] for row in info])


def log_arguments(items, gidx, G, N, ks):
    """the arguments q = c / T of every logarithm the kernel takes for this case (doubles)"""
    K = items.shape[1]
    qs = []
    for g in range(G):
        rows = items[gidx == g]
        for k in ks:
            if rows.shape[0]:
                c = np.bincount(rows[:, :min(k, K)].reshape(-1), minlength=N)
                qs.append(np.unique(c[c > 0]).astype(np.float64) / (float(rows.shape[0]) * float(k)))
    return np.concatenate(qs) if qs else np.zeros(0)


def exact_means(out_i, sizes, ks):
    """[G][n_k][3] floats: float(Fraction(sum, n_g k)) of pop, tl, cnt (NaN for an empty group)"""
    return np.array([[[float(Fraction(v, int(sizes[g]) * k)) if sizes[g] else float("nan") for v in out_i[g][j][2:5]]
                      for j, k in enumerate(ks)] for g in range(len(out_i))])


# ---- case builders -------------------------------------------------------------------------------------------------------------------

def zipf_lists(rng, U, K, N, everyone=None):
    """[U, K] item ids in [1, N): popularity-skewed draws, repeats inside a list allowed; `everyone`: that item at rank 0 of every
    list"""
    w = 1.0 / np.arange(1, N) ** 1.1
    items = rng.choice(np.arange(1, N), size=(U, K), p=w / w.sum()).astype(np.int64)
    if everyone is not None:
        items[:, 0] = everyone
    return items


def interleave(rng, items, gidx):
    perm = rng.permutation(items.shape[0])
    return items[perm], gidx[perm]


@functools.lru_cache(maxsize=None)
def chunk_case(K, interleaved):
    """groups of 1 / 63 / 64 / 65 / 129 / 257 users, item 3 at rank 0 of every list (its count is n_g in every group: the last slot
    of each histogram segment); contiguous in row order or interleaved"""
    rng = np.random.default_rng(100 + K)
    gidx = np.repeat(np.arange(len(CHUNK_SIZES)), CHUNK_SIZES)
    items = zipf_lists(rng, gidx.shape[0], K, N_ITEMS, everyone=3)
    if interleaved:
        items, gidx = interleave(rng, items, gidx)
    return items, gidx, len(CHUNK_SIZES), N_ITEMS


def assignment(U, G):
    """every group present, sizes uneven for 1 < G < U, groups interleaved in row order"""
    rng = np.random.default_rng(7 * G + U)
    gidx = np.concatenate((np.arange(G), rng.integers(0, G, U - G) if U > G else np.zeros(0, dtype=np.int64))).astype(np.int64)
    return rng.permutation(gidx)


@functools.lru_cache(maxsize=None)
def count_case(G, U):
    rng = np.random.default_rng(300 + G)
    return zipf_lists(rng, U, GROUP_K, N_ITEMS), assignment(U, G), G, N_ITEMS


def heads_case():
    """one group, K = 1, so entry = user and the sorted keys are the sorted items: cells [0, 50) [50, 63) [63] [64] [65, 200)
    [200, 259) [259]: heads at the entry positions 0, 63, 64, 65 and at the last entry, the cell from 65 spans the wave boundaries
    at 128 and 192"""
    runs = [(5, 50), (9, 13), (11, 1), (12, 1), (20, 135), (31, 59), (40, 1)]
    items = np.concatenate([np.full(n, i, dtype=np.int64) for i, n in runs]).reshape(-1, 1)
    assert items.shape[0] == 260
    heads = np.concatenate(([0], np.cumsum([n for _, n in runs])[:-1]))
    assert heads.tolist() == [0, 50, 63, 64, 65, 200, 259]
    return np.random.default_rng(3).permutation(items), np.zeros(260, dtype=np.int64), 1, N_ITEMS


def heads_case_two_groups():
    """two groups of 64 and 66 users, K = 1: the group boundary falls on the wave boundary at entry 64, a head at 63 (last lane
    of a wave), at 64 (first lane of the next), and a cell [65, 129) over the wave boundary at 128; the last entry is a head"""
    a = np.concatenate([np.full(63, 4), np.full(1, 8)])
    b = np.concatenate([np.full(1, 2), np.full(64, 6), np.full(1, 9)])
    items = np.concatenate([a, b]).astype(np.int64).reshape(-1, 1)
    gidx = np.concatenate([np.zeros(64), np.ones(66)]).astype(np.int64)
    return items, gidx, 2, N_ITEMS


def padded_case():
    """candidate-style lists: a few real items, the rest padded with item 0.  Group 0: 30 users whose lists hold 2 .. 6 real items
    (cell (0, 0) has more than 4 n_g entries), and item 7 at TWO ranks of every list (a second cell above n_g); group 1: one user
    whose whole list is item 0; group 2: 12 users, padded from rank 5 on"""
    rng = np.random.default_rng(17)
    K = 10
    a = np.zeros((30, K), dtype=np.int64)
    for u in range(30):
        n = 2 + u % 5
        a[u, :2] = 7
        a[u, 2:n] = rng.choice(np.arange(8, N_ITEMS), n - 2, replace=False)
    b = np.zeros((1, K), dtype=np.int64)
    c = np.zeros((12, K), dtype=np.int64)
    c[:, :5] = zipf_lists(rng, 12, 5, N_ITEMS)
    items = np.concatenate([a, b, c])
    gidx = np.repeat(np.arange(3), [30, 1, 12])
    items, gidx = interleave(rng, items, gidx)
    return items, gidx, 3, N_ITEMS


def empty_group_case():
    """four groups over 90 users, group 2 has no user"""
    rng = np.random.default_rng(23)
    gidx = rng.permutation(np.repeat([0, 1, 3], [40, 17, 33])).astype(np.int64)
    return zipf_lists(rng, 90, GROUP_K, N_ITEMS), gidx, 4, N_ITEMS


def kernel_cases():
    """every (tag, items, gidx, G, N, ks) the kernel tests run: the arguments of the device logarithm are taken over these"""
    out = []
    for K, ks in CHUNK_SHAPES:
        for inter in (False, True):
            out.append((f"chunk K={K} {'interleaved' if inter else 'contiguous'}", *chunk_case(K, inter), ks))
    for G, U in GROUP_COUNTS:
        out.append((f"G={G} U={U}", *count_case(G, U), GROUP_KS))
    out.append(("heads", *heads_case(), [1]))
    out.append(("heads, two groups", *heads_case_two_groups(), [1]))
    out.append(("padded", *padded_case(), [1, 5, 10]))
    out.append(("ks beyond K", *count_case(3, 120), [5, 99]))
    out.append(("empty group", *empty_group_case(), GROUP_KS))
    return out
