"""kge_kvsall_collate restated in plain numpy / Python, one example at a time: the batch form (what the reference's
collate function returns, kge/job/train_KvsAll.py:118-201), the typed form (the per-type CSR of the fused KvsAll
losses, exact or padded as the captured step wants it) and the counts.  Deliberately naive: loops, no scans.

An index is (keys int64 [M, 2], offsets int64 [M + 1], values int64 [.]); `types` is a list of (index, query type) in
the job's order, example numbers run through the types one after the other."""
import numpy as np

TARGET_COL = {"sp_": 2, "s_o": 1, "_po": 0}


def last_examples(types):
    return np.cumsum([len(ix[0]) for ix, _ in types]).astype(np.int64)


def locate(types, example):
    """example number -> (type index, the example's number within its type)"""
    start = 0
    for t, (ix, _) in enumerate(types):
        end = start + len(ix[0])
        if example < end:
            return t, example - start
        start = end
    raise IndexError(example)


def batch_form(types, examples):
    n = len(examples)
    queries = np.zeros((n, 2), dtype=np.int64)
    qtype = np.zeros(n, dtype=np.int64)
    coords, triples = [], []
    for i, example in enumerate(examples):
        t, e = locate(types, int(example))
        (keys, offsets, values), query_type = types[t]
        queries[i] = keys[e]
        qtype[i] = t
        target = TARGET_COL[query_type]
        q_cols = [c for c in (0, 1, 2) if c != target]  # the key columns, in S, P, O order
        for v in values[offsets[e]:offsets[e + 1]]:
            coords.append((i, v))
            tri = [0, 0, 0]
            tri[q_cols[0]], tri[q_cols[1]], tri[target] = keys[e][0], keys[e][1], v
            triples.append(tri)
    return {"queries": queries, "query_type_indexes": qtype,
            "label_coords": np.asarray(coords, dtype=np.int32).reshape(-1, 2),
            "triples": np.asarray(triples, dtype=np.int64).reshape(-1, 3)}


def counts(types, examples, caps=None):
    """int64 [T, 3]: n_t, nnz_t, fits (1 without capacities)"""
    out = np.zeros((len(types), 3), dtype=np.int64)
    for example in examples:
        t, e = locate(types, int(example))
        offsets = types[t][0][1]
        out[t, 0] += 1
        out[t, 1] += offsets[e + 1] - offsets[e]
    for t in range(len(types)):
        if caps is None:
            out[t, 2] = 1
        else:
            rows_cap, lab_cap = caps[t]
            out[t, 2] = int(out[t, 0] <= rows_cap and out[t, 1] + (rows_cap - out[t, 0]) <= lab_cap)
    return out


def typed_form(types, examples, caps=None, weight=1.0):
    """-> per type (ids [rows_cap, 2], rowptr [rows_cap + 1], col [lab_cap], weight float32 [rows_cap], rows [rows_cap]),
    or None for a type that does not fit its capacities.  caps None: rows_cap = n_t, lab_cap = nnz_t."""
    cnt = counts(types, examples, caps)
    out = []
    for t, ((keys, offsets, values), _) in enumerate(types):
        rows_cap, lab_cap = (int(cnt[t, 0]), int(cnt[t, 1])) if caps is None else caps[t]
        if not cnt[t, 2]:
            out.append(None)
            continue
        ids = np.zeros((rows_cap, 2), dtype=np.int64)
        rowptr = np.zeros(rows_cap + 1, dtype=np.int64)
        col = np.zeros(lab_cap, dtype=np.int64)
        w = np.zeros(rows_cap, dtype=np.float32)
        rows = np.full(rows_cap, -1, dtype=np.int64)
        r = z = 0
        for i, example in enumerate(examples):
            tt, e = locate(types, int(example))
            if tt != t:
                continue
            labels = values[offsets[e]:offsets[e + 1]]
            ids[r], w[r], rows[r] = keys[e], np.float32(weight), i
            col[z:z + len(labels)] = labels
            z += len(labels)
            r += 1
            rowptr[r] = z
        for r in range(r, rows_cap):  # padding rows: query (0, 0), the single label 0, weight 0, batch row -1
            z += 1
            rowptr[r + 1] = z
        out.append((ids, rowptr, col, w, rows))
    return out


def random_index(rng, num_keys, max_value, degrees):
    """An index with the given label counts per key: distinct sorted labels below max_value per key."""
    keys = np.stack([rng.integers(0, max_value, num_keys), rng.integers(0, 7, num_keys)], axis=1).astype(np.int64)
    offsets = np.concatenate([[0], np.cumsum(degrees)]).astype(np.int64)
    values = np.concatenate([np.sort(rng.choice(max_value, size=int(d), replace=False)) for d in degrees]
                            + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
    return keys, offsets, values
