"""float64 references of the fused 1vsAll loss of float32 ComplEx / DistMult tables (kge_ce_f32_*), numpy only: the
query vectors, the scores, and the CHUNKED backward with the library's structure -- per chunk G = g (softmax - onehot),
dT[chunk] = G^T Q overwritten, dQ += G T[chunk] accumulated, the chain rule once after the last chunk."""
import numpy as np


def queries(name, direction, a_rows, r_rows):
    """Q [n, d] with score = Q T^T (complex.py:30-39, distmult.py:15-21)"""
    if name == "distmult":
        return a_rows * r_rows
    h = a_rows.shape[1] // 2
    are, aim, rre, rim = a_rows[:, :h], a_rows[:, h:], r_rows[:, :h], r_rows[:, h:]
    if direction == "sp":
        return np.concatenate([are * rre - aim * rim, aim * rre + are * rim], 1)
    return np.concatenate([rre * are + rim * aim, rre * aim - rim * are], 1)


def chain(name, direction, dq, a_rows, r_rows):
    """(d loss / d a_rows, d loss / d r_rows) from dQ"""
    if name == "distmult":
        return dq * r_rows, dq * a_rows
    h = a_rows.shape[1] // 2
    are, aim, rre, rim = a_rows[:, :h], a_rows[:, h:], r_rows[:, :h], r_rows[:, h:]
    dre, dim = dq[:, :h], dq[:, h:]
    if direction == "sp":
        return (np.concatenate([dre * rre + dim * rim, dim * rre - dre * rim], 1),
                np.concatenate([dre * are + dim * aim, dim * are - dre * aim], 1))
    return (np.concatenate([dre * rre - dim * rim, dre * rim + dim * rre], 1),
            np.concatenate([dre * are + dim * aim, dre * aim - dim * are], 1))


def forward(name, direction, ent, rel, a, p, label):
    """(loss_rows, lse) in float64"""
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    x = queries(name, direction, ent[a], rel[p]) @ ent.T
    mx = x.max(axis=1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    return lse - x[np.arange(len(label)), label], lse


def chunked_backward(name, direction, ent, rel, a, p, label, g, chunk_cols):
    """(g_a [n, d], g_p [n, d], g_tgt [E, d]) of sum_i g_i loss_rows_i, float64, walking the entity columns in chunks of
    `chunk_cols` (0: one chunk)"""
    ent, rel = np.asarray(ent, np.float64), np.asarray(rel, np.float64)
    E, n = ent.shape[0], len(a)
    _, lse = forward(name, direction, ent, rel, a, p, label)
    Q = queries(name, direction, ent[a], rel[p])
    C = chunk_cols or E
    dq = np.zeros_like(Q)
    g_tgt = np.full_like(ent, np.nan)
    for c0 in range(0, E, C):
        T = ent[c0:c0 + C]
        G = np.exp(Q @ T.T - lse[:, None])
        hit = (label >= c0) & (label < c0 + T.shape[0])
        G[np.arange(n)[hit], label[hit] - c0] -= 1.0
        G *= np.asarray(g, np.float64)[:, None]
        g_tgt[c0:c0 + C] = G.T @ Q
        dq += G @ T
    g_a, g_p = chain(name, direction, dq, ent[a], rel[p])
    return g_a, g_p, g_tgt
