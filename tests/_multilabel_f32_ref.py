"""float64 references of the fused KvsAll losses of float32 ComplEx / DistMult tables (kge_kl_f32_* / kge_bce_f32_*),
numpy only: the kl forward (weighted and unweighted), the bce forward, the CHUNKED backward with the library's structure
-- per chunk an explicit bit mask of n x C bits set from the CSR, G from the mask, dT[chunk] = G^T Q overwritten,
dQ += G T[chunk], the chain rule once after the last chunk, label_bias inside G -- and the label generator of the GPU
tests.  Queries and the chain rule are those of tests/_ce_f32_ref.py."""
import numpy as np

from _ce_f32_ref import chain, queries


def scores(name, direction, ent, rel, a, p):
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    return queries(name, direction, ent[a], rel[p]) @ ent.T


def lse64(x):
    x = np.asarray(x, np.float64)
    mx = x.max(axis=1)
    return mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))


def dense(rowptr, col, n, E):
    y = np.zeros((n, E))
    y[np.repeat(np.arange(n), np.diff(rowptr)), col] = 1.0
    return y


def kl_rows(x, rowptr, col, label_weight=None):
    """(loss_rows, lse) from scores x [n, E]: kge_kl_fwd's definition (0 for a row without labels) or, with
    label_weight, kge_kl_weighted_fwd's (lse_i - w_i sum of the label scores: every row)"""
    x = np.asarray(x, np.float64)
    n, E = x.shape
    k = np.diff(rowptr).astype(np.float64)
    lab = (x * dense(rowptr, col, n, E)).sum(axis=1)
    lse = lse64(x)
    if label_weight is not None:
        return lse - np.asarray(label_weight, np.float64) * lab, lse
    kk = np.maximum(k, 1.0)
    return np.where(k > 0, lse - lab / kk - np.log(kk), 0.0), lse


def bce_rows(x, rowptr, col, offset=0.0):
    """sum_j softplus(x_ij + offset) - sum over the labels of (x_ij + offset): kge_bce_fwd's definition"""
    z = np.asarray(x, np.float64) + offset
    n, E = z.shape
    sp = np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))
    return sp.sum(axis=1) - (z * dense(rowptr, col, n, E)).sum(axis=1)


def kl_forward(name, direction, ent, rel, a, p, rowptr, col, label_weight=None):
    return kl_rows(scores(name, direction, ent, rel, a, p), rowptr, col, label_weight)


def bce_forward(name, direction, ent, rel, a, p, rowptr, col, offset=0.0):
    return bce_rows(scores(name, direction, ent, rel, a, p), rowptr, col, offset)


def chunk_mask(rowptr, col, n, c0, mc, C):
    """the chunk's label bits as the library keeps them: [n, C / 32] uint32 words, bit y & 31 of word y >> 5 for every CSR
    entry with c0 <= col < c0 + mc (labels outside the table set nothing)"""
    mask = np.zeros((n, C // 32), dtype=np.uint32)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    y = np.asarray(col, np.int64) - c0
    ok = (y >= 0) & (y < mc)
    np.bitwise_or.at(mask, (rows[ok], y[ok] >> 5), (np.uint32(1) << (y[ok] & 31).astype(np.uint32)))
    return mask


def chunked_backward(kind, name, direction, ent, rel, a, p, rowptr, col, g, chunk_cols, label_weight=None,
                     label_bias=None, offset=0.0):
    """(g_a [n, d], g_p [n, d], g_tgt [E, d]) of sum_i g_i loss_rows_i, float64, walking the entity columns in chunks of
    `chunk_cols` (a multiple of 128; 0: one chunk of E rounded up).  kind "kl": G = g_i (softmax - b_i - w_i [label]),
    w_i = label_weight or 1 / k_i (then g_i = 0 for k_i = 0); "bce": G = g_i (sigmoid(score + offset) - [label])."""
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    E, n = ent.shape[0], len(a)
    k = np.diff(rowptr).astype(np.float64)
    gi = np.asarray(g, np.float64).copy()
    w = np.ones(n)
    if kind == "kl":
        if label_weight is not None:
            w = np.asarray(label_weight, np.float64)
        else:
            w = 1.0 / np.maximum(k, 1.0)
            gi[k == 0] = 0.0
    b = np.zeros(n) if label_bias is None else np.asarray(label_bias, np.float64)
    Q = queries(name, direction, ent[a], rel[p])
    lse = lse64(Q @ ent.T)
    C = chunk_cols or -(-E // 128) * 128
    assert C % 128 == 0
    dq = np.zeros_like(Q)
    g_tgt = np.full_like(ent, np.nan)
    for c0 in range(0, E, C):
        T = ent[c0:c0 + C]
        mc = T.shape[0]
        mask = chunk_mask(rowptr, col, n, c0, mc, C)
        y = np.arange(mc)
        hit = ((mask[:, y >> 5] >> (y & 31).astype(np.uint32)) & 1).astype(np.float64)
        S = Q @ T.T
        if kind == "kl":
            G = np.exp(S - lse[:, None]) - b[:, None] - w[:, None] * hit
        else:
            G = 1.0 / (1.0 + np.exp(-(S + offset))) - hit
        G *= gi[:, None]
        g_tgt[c0:c0 + C] = G.T @ Q
        dq += G @ T
    g_a, g_p = chain(name, direction, dq, ent[a], rel[p])
    return g_a, g_p, g_tgt


def smoothing_terms(rowptr, E, eps):
    """(w, b, const) of label smoothing `eps` (include/kge_amd.h at kge_kl_weighted_fwd): Z_i = (1 - eps) k_i + 1,
    a_i = (1 - eps + 1/E) / Z_i, b_i = (1/E) / Z_i, w_i = a_i - b_i, const_i = k_i a_i log a_i + (E - k_i) b_i log b_i"""
    k = np.diff(rowptr).astype(np.float64)
    Z = (1.0 - eps) * k + 1.0
    a_w, b_w = (1.0 - eps + 1.0 / E) / Z, (1.0 / E) / Z
    return a_w - b_w, b_w, k * a_w * np.log(a_w) + (E - k) * b_w * np.log(b_w)


# ---- the label sets of the GPU tests ----------------------------------------------------------------------------------
ROW_COUNTS = (0, 1, 2, 63, 64, 65, 130)   # the finish kernel scores 64 labels per round: none, one round +- 1, three rounds


def edge_columns(E):
    """labels at the table's ends, on either side of a mask word and of a tile edge, and in the last tile but one"""
    cols = [0, E - 1, 31, 32, 127, 128, (E - 1) // 128 * 128 - 121]
    return sorted({c for c in cols if 0 <= c < E})


def labels(rng, n, E):
    """CSR label sets of n rows over E entities, ids unique per row and SHUFFLED within the rows.  Rows 0..6 have
    min(ROW_COUNTS[i], E) labels; row 5 (65 labels) holds every edge column (edge_columns); where E == 129 row 6 is
    labelled with EVERY entity; the further rows have 1..12 random labels, every seventh exactly one, every fifth one
    edge column among them.  n < 7: the rows cycle through the kinds from the largest down, so that a single row is the
    big one with the edge columns."""
    rows = []
    edges = edge_columns(E)
    for i in range(n):
        kind = i if n >= len(ROW_COUNTS) else len(ROW_COUNTS) - 1 - i % len(ROW_COUNTS)
        if kind < len(ROW_COUNTS):
            k = min(ROW_COUNTS[kind], E)
            if kind == 6 and E == 129:
                k = E
            must = edges if (kind == 5 or (n < len(ROW_COUNTS) and kind == 6)) and k >= len(edges) else []
            rest = [c for c in rng.permutation(E) if c not in set(must)]
            ids = list(must) + rest[:k - len(must)]
        else:
            k = 1 if i % 7 == 0 else int(rng.integers(1, 13))
            ids = list(rng.choice(E, size=min(k, E), replace=False))
            if i % 5 == 0:
                e = edges[(i // 5) % len(edges)]
                if e not in ids:
                    ids[0] = e
        ids = np.asarray(ids, dtype=np.int64)
        for _ in range(8):  # (a permutation of more than one id that came back sorted is drawn again)
            ids = rng.permutation(ids)
            if len(ids) < 2 or not np.array_equal(ids, np.sort(ids)):
                break
        rows.append(ids)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows).astype(np.int64) if rowptr[-1] else np.zeros(0, dtype=np.int64)
    return rowptr, col


def dense_backward(name, direction, ent, rel, a, p, G):
    """(g_a, g_p, g_tgt) from a dense d loss / d score G [n, E]: the two products and the chain rule in one piece (the
    linear label-smoothing terms of the bce loss, which the model composes around the kernel)"""
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    Q = queries(name, direction, ent[a], rel[p])
    g_a, g_p = chain(name, direction, G @ ent, ent[a], rel[p])
    return g_a, g_p, G.T @ Q
