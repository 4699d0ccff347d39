"""numpy restatement of kge_topk (include/kge_amd.h; DESIGN.md "Filtered top-k prediction"): the result from a score
matrix, the 64-bit key and the merge of per-group lists.  Every element of the result is determined: scores are
canonicalised (NaN -> -inf, -0.0 -> +0.0), filtered columns dropped (except the row's `keep`), the rest ordered by
descending value and, among equal values, ascending entity id; rows with fewer than k columns are padded with (-inf, -1).
"""
import numpy as np

NEG_INF = np.float32(-np.inf)


def canonical(scores):
    s = np.array(scores, dtype=np.float32, copy=True)
    s[np.isnan(s)] = NEG_INF
    s[s == 0] = np.float32(0.0)  # -0.0 -> +0.0
    return s


def dropped_columns(n, m, filters, keep, col_begin):
    """bool [n, m]: column j of the slice is listed for row i in ANY set (global ids; ids outside the slice are ignored;
    the row's keep id never)."""
    drop = np.zeros((n, m), dtype=bool)
    for begin, end, col in filters or []:
        begin, end, col = (np.asarray(x, dtype=np.int64) for x in (begin, end, col))
        for i in range(n):
            g = col[begin[i]:end[i]]
            if keep is not None:
                g = g[g != int(keep[i])]
            j = g - col_begin
            j = j[(j >= 0) & (j < m)]
            drop[i, j] = True
    return drop


def topk_ref(scores, k, filters=None, keep=None, col_begin=0):
    """(values [n, k] float32, ids [n, k] int64) from scores [n, m] whose column j is entity col_begin + j."""
    s = canonical(scores)
    n, m = s.shape
    drop = dropped_columns(n, m, filters, keep, col_begin)
    val = np.full((n, k), NEG_INF, dtype=np.float32)
    idx = np.full((n, k), -1, dtype=np.int64)
    ids = np.arange(m, dtype=np.int64)
    for i in range(n):
        live = ids[~drop[i]]
        v = s[i, live]
        order = np.lexsort((live, -v.astype(np.float64)))  # stable: primary -value, then id (float64 negation is exact)
        top = live[order[:k]]
        val[i, :len(top)] = s[i, top]
        idx[i, :len(top)] = top + col_begin
    return val, idx


# ---- the 64-bit key ----------------------------------------------------------------------------------------------
def pack_keys(scores, j):
    """uint64 keys: high word = the order-preserving unsigned image of the canonical score, low word = 0xFFFFFFFF - j."""
    s = canonical(np.asarray(scores, dtype=np.float32).reshape(-1))
    u = s.view(np.uint32).astype(np.uint64)
    neg = (u & np.uint64(0x80000000)) != 0
    hi = np.where(neg, (~u) & np.uint64(0xFFFFFFFF), u | np.uint64(0x80000000))
    lo = np.uint64(0xFFFFFFFF) - np.asarray(j, dtype=np.uint64).reshape(-1)
    return (hi << np.uint64(32)) | lo


def unpack_keys(keys, col_begin=0):
    """(values float32, ids int64); key 0 ("empty") -> (-inf, -1)."""
    keys = np.asarray(keys, dtype=np.uint64)
    hi = (keys >> np.uint64(32)).astype(np.uint32)
    lo = (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    neg = (hi & np.uint32(0x80000000)) == 0  # (the image of a negative float has its top bit clear)
    u = np.where(neg, ~hi, hi & np.uint32(0x7FFFFFFF)).astype(np.uint32)
    val = u.view(np.float32).copy()
    idx = (np.uint32(0xFFFFFFFF) - lo).astype(np.int64) + col_begin
    empty = keys == 0
    val[empty] = NEG_INF
    idx[empty] = -1
    return val, idx


def group_list(score_row, drop_row, j0, j1, k):
    """The sorted list (descending keys, zero-padded to k) a workgroup keeps for the columns [j0, j1) of one row."""
    j = np.arange(j0, j1, dtype=np.int64)
    j = j[~drop_row[j0:j1]]
    keys = np.sort(pack_keys(score_row[j], j))[::-1][:k]
    out = np.zeros(k, dtype=np.uint64)
    out[:len(keys)] = keys
    return out


def merge_lists(lists, k):
    """The best k keys of the groups' lists (zeros = empty slots stay behind)."""
    allk = np.sort(np.concatenate([np.asarray(x, dtype=np.uint64) for x in lists]))[::-1][:k]
    out = np.zeros(k, dtype=np.uint64)
    out[:len(allk)] = allk
    return out


def topk_by_groups(scores, k, cuts, filters=None, keep=None, col_begin=0):
    """topk_ref computed the kernels' way: per-group key lists over the column ranges between `cuts`, merged."""
    s = np.asarray(scores, dtype=np.float32)
    n, m = s.shape
    drop = dropped_columns(n, m, filters, keep, col_begin)
    edges = [0] + [c for c in sorted(set(cuts)) if 0 < c < m] + [m]
    val = np.empty((n, k), dtype=np.float32)
    idx = np.empty((n, k), dtype=np.int64)
    for i in range(n):
        lists = [group_list(s[i], drop[i], a, b, k) for a, b in zip(edges[:-1], edges[1:])]
        val[i], idx[i] = unpack_keys(merge_lists(lists, k), col_begin)
    return val, idx
