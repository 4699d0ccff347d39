"""KvsAll kl and bce losses of TransE / RotatE on float32 tables without a score matrix (kge_kl_dist_* / kge_bce_dist_*,
ce_dist.hip) on the MI355X: the forward against float64 losses of the project's own stored scores and of the oracle's,
the label scores bit for bit against the stored matrix, the backward against float64 autograd of the reference's op
sequence and against the unfused device path, chunkings against each other, the label mask left zero, guards, and the
model level with its memory bound.  Shapes, tables and queries are those of test_gpu_ce_dist.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import torch_port as tp
import test_gpu_ce_dist as ce

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ce.CASES
DIRECTIONS = ce.DIRECTIONS
OFFSET = 3.0
_t, _close, _tables, _table_grads = ce._t, ce._close, ce._tables, ce._table_grads


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _labels(rng, n, E):
    """CSR label sets of n rows over E entities, ids unique per row and in SHUFFLED order.  Row 0 has no label; rows 1-3
    exactly one (columns 0, min(63, E - 1) and E - 1); row 4 at least 65 (all E where E < 65) with columns 0, 63, 64, 127,
    128 and E - 1 among them where they exist: labels on both sides of the chunk borders of chunk_cols 64 and 128; every
    further row 1..12 random labels, every seventh exactly one.  n = 1: the single row is the big one."""
    rows = []
    for i in range(n):
        kind = i if n > 4 else 4
        if kind == 0:
            ids = []
        elif kind in (1, 2, 3):
            ids = [(0, min(63, E - 1), E - 1)[kind - 1]]
        elif kind == 4:
            must = {c for c in (0, 63, 64, 127, 128, E - 1) if c < E}
            rest = [c for c in rng.permutation(E) if c not in must]
            ids = list(must) + rest[:max(0, min(65 + int(rng.integers(0, 8)), E) - len(must))]
        else:
            k = 1 if i % 7 == 0 else int(rng.integers(1, 13))
            ids = list(rng.choice(E, size=min(k, E), replace=False))
        rows.append(rng.permutation(np.asarray(ids, dtype=np.int64)))
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows) if rowptr[-1] else np.zeros(0, dtype=np.int64)
    return rowptr, col.astype(np.int64)


def _dense(rowptr, col, n, E):
    y = np.zeros((n, E))
    y[np.repeat(np.arange(n), np.diff(rowptr)), col] = 1.0
    return y


def _loss64(kind, scores, y, offset=0.0):
    """float64 per-row loss of the reference's loss functions on a dense label matrix"""
    x, yy = torch.as_tensor(scores, dtype=torch.float64), torch.as_tensor(y, dtype=torch.float64)
    if kind == "kl":
        return tp.kl_loss(x, yy, reduction="rows")
    return tp.bce_loss(x, yy, offset, reduction="rows")


def _lse64(x):
    x = np.asarray(x, dtype=np.float64)
    mx = x.max(axis=1)
    return mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))


@functools.lru_cache(maxsize=None)
def _case(name, l_norm, d, E, R, n):
    """test_gpu_ce_dist's case (tables, queries, oracle scores, g_rows) + label sets per direction + the float64
    autograd gradients of both losses: computed once and shared, never modified."""
    c = dict(ce._case(name, l_norm, d, E, R, n))
    rng = np.random.default_rng(11 + 1000 * d + n + int(l_norm))
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        rowptr, col = _labels(rng, n, E)
        y = _dense(rowptr, col, n, E)
        c["csr_" + direction], c["y_" + direction] = (rowptr, col), y
        e64 = torch.from_numpy(c["ent"]).double().requires_grad_()
        r64 = torch.from_numpy(c["rel"]).double().requires_grad_()
        ai, pi = torch.from_numpy(a), torch.from_numpy(c["p"])
        sc = tp.score_sp(name, e64, r64, ai, pi, None, l_norm) if direction == "sp" else \
            tp.score_po(name, e64, r64, pi, ai, None, l_norm)
        for kind in ("kl", "bce"):
            rows = _loss64(kind, sc, y, OFFSET)
            for gname, g in (("rows", c["g_rows"].astype(np.float64)), ("scalar", np.full(n, np.float64(np.float32(0.37))))):
                ge, gr = torch.autograd.grad((rows * torch.from_numpy(g)).sum(), (e64, r64), retain_graph=True)
                c[f"grad64_{kind}_{direction}_{gname}"] = (ge.numpy(), gr.numpy())
        # the weighted kl loss (kge_kl_weighted_fwd's definition): lse_i - w_i sum_labels score, every row
        w = _label_weight(n)
        rows = torch.logsumexp(sc, dim=1) - torch.from_numpy(w.astype(np.float64)) * (sc * torch.from_numpy(y)).sum(dim=1)
        ge, gr = torch.autograd.grad((rows * torch.from_numpy(c["g_rows"].astype(np.float64))).sum(), (e64, r64))
        c[f"grad64_klw_{direction}_rows"] = (ge.numpy(), gr.numpy())
    return c


def _label_weight(n):
    return np.random.default_rng(6).uniform(0.05, 1.0, n).astype(np.float32)


def test_label_sets_cover_what_they_should():
    for name, l_norm, d, E, R, n in CASES:
        if name != "transe" or l_norm != 1.0:
            continue
        rng = np.random.default_rng(11 + 1000 * d + n + int(l_norm))
        rowptr, col = _labels(rng, n, E)
        k = np.diff(rowptr)
        big = int(np.argmax(k))
        ids = set(col[rowptr[big]:rowptr[big + 1]].tolist())
        assert k.max() >= min(65, E) and {c for c in (0, 63, 64, 127, 128, E - 1) if c < E} <= ids
        assert all(len(set(col[rowptr[i]:rowptr[i + 1]].tolist())) == k[i] for i in range(n)), "ids unique per row"
        assert not np.array_equal(np.sort(col[rowptr[big]:rowptr[big + 1]]), col[rowptr[big]:rowptr[big + 1]]), "shuffled"
        if n > 4:
            assert k[0] == 0 and (k[1:4] == 1).all() and (k == 1).sum() >= 3


def _fwd(eng, kind, T, direction, ai, pi, csr, offset=0.0, label_weight=None, **kw):
    """(loss_rows, lse or None)"""
    if kind == "kl":
        return eng.kl_dist_fwd(T, direction, ai, pi, csr[0], csr[1], label_weight, **kw)
    return eng.bce_dist_fwd(T, direction, ai, pi, csr[0], csr[1], offset, **kw), None


def _bwd(eng, kind, T, direction, ai, pi, csr, lse, offset=0.0, **kw):
    if kind == "kl":
        return eng.kl_dist_bwd(T, direction, ai, pi, csr[0], csr[1], lse, **kw)
    return eng.bce_dist_bwd(T, direction, ai, pi, csr[0], csr[1], offset, **kw)


@pytest.mark.parametrize("name,l_norm,d,E,R,n", CASES)
def test_forward_against_stored_scores_and_oracle(eng, name, l_norm, d, E, R, n):
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        ai, pi = _t(a), _t(c["p"])
        rowptr, col = c["csr_" + direction]
        csr, y, k = (_t(rowptr), _t(col)), c["y_" + direction], np.diff(rowptr)
        sc = (eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)).cpu().numpy()
        assert np.array_equal(sc, c["oracle_" + direction]), "stored scores differ from the oracle's"
        w = np.random.default_rng(5).uniform(0.05, 1.0, n).astype(np.float32)
        runs = [("kl", 0.0, None), ("kl", 0.0, w), ("bce", 0.0, None), ("bce", OFFSET, None)]
        for kind, offset, lw in runs:
            lwt = None if lw is None else _t(lw)
            loss, lse = _fwd(eng, kind, T, direction, ai, pi, csr, offset, lwt)
            loss2, lse2 = _fwd(eng, kind, T, direction, ai, pi, csr, offset, lwt)
            assert torch.equal(loss, loss2) and (lse is None or torch.equal(lse, lse2)), "two runs differ"
            got = {"loss": loss.cpu().numpy().astype(np.float64)}
            if lse is not None:
                got["lse"] = lse.cpu().numpy().astype(np.float64)
            assert all(np.isfinite(v).all() for v in got.values()), (kind, direction)
            for ref_name, ref in (("stored", sc), ("oracle", c["oracle_" + direction])):
                x = ref.astype(np.float64)
                if kind == "kl" and lw is not None:  # kge_kl_weighted_fwd's definition: lse - w_i sum_labels score
                    want_loss = _lse64(x) - lw.astype(np.float64) * (x * y).sum(axis=1)
                else:
                    want_loss = _loss64(kind, x, y, offset).numpy()
                want = {"loss": want_loss, "lse": _lse64(x)}
                for nm, g in got.items():
                    err, tol = np.abs(g - want[nm]), 1e-5 + 1e-5 * np.abs(want[nm])
                    print(f"{name} L{l_norm:g} {direction} {kind} offset {offset:g} weight {lw is not None} {nm} vs "
                          f"{ref_name}: max err {err.max():.3e} min tol {tol.min():.3e}")
                    assert (err <= tol).all(), (kind, direction, ref_name, nm, float(err.max()), int((err > tol).sum()))
            if kind == "kl" and lw is None and n > 4:
                assert (got["loss"][k == 0] == 0.0).all(), "kl: a row without labels has loss 0"
            if kind == "kl" and lw is not None and n > 4:
                assert np.array_equal(got["loss"][k == 0], got["lse"][k == 0]), "weighted kl: a row without labels has lse"


@pytest.mark.parametrize("name,l_norm,d,E,R,n", CASES)
def test_label_scores_have_the_bits_of_the_score_matrix(eng, name, l_norm, d, E, R, n):
    """On the rows with exactly one label the label score is read back out of the loss and compared with
    score_sp(...)[i, label_i] bit for bit.  With weight 1: loss_rows = fl(lse - s), and lse - loss_rows gives s back
    exactly where the first subtraction is exact -- by Sterbenz's lemma where |s| / 2 <= |lse| <= 2 |s| (same sign); on the
    other rows (an lse closer to 0 than half the score: most rows of some cases) the float32 subtraction itself rounds, so
    there the identity asserted is the kernel's own expression, loss_rows == fl(lse - s).  To read the bits back on EVERY
    row, a second run takes per-row weights 2^e_i (exact products) chosen so that 2^e_i s lies within a factor 2 of lse:
    then (lse - loss_rows) / 2^e_i is s exactly."""
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    checked = 0
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        ai, pi = _t(a), _t(c["p"])
        rowptr, col = c["csr_" + direction]
        sc = eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)
        loss, lse = eng.kl_dist_fwd(T, direction, ai, pi, _t(rowptr), _t(col), torch.ones(n, device=DEV))
        one = np.flatnonzero(np.diff(rowptr) == 1)
        if len(one) == 0:
            continue
        rows = _t(one)
        want, l1, z1 = sc[rows, _t(col[rowptr[one]])], loss[rows], lse[rows]
        assert torch.equal(l1, z1 - want), (direction, "loss_rows != fl(lse - score)")
        exact = (z1 * want > 0) & (z1.abs() >= want.abs() / 2) & (z1.abs() <= want.abs() * 2)
        print(f"{name} L{l_norm:g} {direction}: {int(exact.sum())} of {len(one)} single-label rows with an exact lse - s")
        assert torch.equal((z1 - l1)[exact], want[exact]), (direction, int(((z1 - l1) != want)[exact].sum()), len(one))
        # every row: power-of-two weights that make the subtraction exact
        usable = (z1 * want > 0)
        e = torch.round(torch.log2((z1 / want).abs().clamp_min(1e-30)))
        w_rows = torch.where(usable, torch.exp2(e), torch.ones_like(e))
        w = torch.ones(n, device=DEV)
        w[rows] = w_rows
        loss_w, lse_w = eng.kl_dist_fwd(T, direction, ai, pi, _t(rowptr), _t(col), w)
        assert torch.equal(lse_w, lse)
        got = (z1 - loss_w[rows]) / w_rows
        assert torch.equal(got[usable], want[usable]), (direction, int((got != want)[usable].sum()), len(one))
        assert int(usable.sum()) >= len(one) - 1, (int(usable.sum()), len(one))
        checked += int(usable.sum())
    assert checked > 0 or n == 1


@pytest.mark.parametrize("name,l_norm,d,E,R,n", CASES)
def test_backward_against_float64_autograd_and_the_unfused_path(eng, name, l_norm, d, E, R, n):
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction in DIRECTIONS:
        assert ce._nonzero_differences(c, name, direction)
        a = c["s"] if direction == "sp" else c["o"]
        ai, pi = _t(a), _t(c["p"])
        rowptr, col = c["csr_" + direction]
        csr, y, k = (_t(rowptr), _t(col)), c["y_" + direction], np.diff(rowptr)
        sc = eng.score_sp(T, ai, pi) if direction == "sp" else eng.score_po(T, pi, ai)
        x = sc.double().cpu().numpy()
        for kind in ("kl", "bce"):
            lse = _fwd(eng, kind, T, direction, ai, pi, csr, OFFSET)[1]
            # d loss / d score in float64 from the kernel's own scores
            if kind == "kl":
                dls = np.exp(x - _lse64(x)[:, None]) - y / np.maximum(k, 1)[:, None]
                dls[k == 0] = 0.0
            else:
                dls = 1.0 / (1.0 + np.exp(-(x + OFFSET))) - y
            for gname, kw, g in (("rows", {"g_rows": _t(c["g_rows"])}, c["g_rows"].astype(np.float64)),
                                 ("scalar", {"g_scalar": 0.37}, np.full(n, np.float64(np.float32(0.37))))):
                g_a, g_p, g_t = _bwd(eng, kind, T, direction, ai, pi, csr, lse, OFFSET, **kw)
                ge, gr = _table_grads(c, direction, g_a, g_p, g_t)
                want_e, want_r = c[f"grad64_{kind}_{direction}_{gname}"]
                what = f"{name} L{l_norm:g} {kind} {direction} {gname}"
                _close(ge, want_e, what + " entity vs float64 autograd")
                _close(gr, want_r, what + " relation vs float64 autograd")
                gout = (dls * g[:, None]).astype(np.float32)
                u_a, u_p, u_t = eng.score_pairs_bwd(T, direction, ai, pi, None, _t(gout), sc)
                for nm, got, want in (("g_a", g_a, u_a), ("g_p", g_p, u_p), ("g_tgt", g_t, u_t)):
                    _close(got.double().cpu().numpy(), want.double().cpu().numpy(), f"{what} {nm} vs score_pairs_bwd")
        # kl with a label weight: d loss / d score = g_i (softmax_ij - w_i y_ij), on every row (k_i = 0 too)
        w = _label_weight(n)
        _, lse = eng.kl_dist_fwd(T, direction, ai, pi, csr[0], csr[1], _t(w))
        g_a, g_p, g_t = eng.kl_dist_bwd(T, direction, ai, pi, csr[0], csr[1], lse, g_rows=_t(c["g_rows"]), label_weight=_t(w))
        ge, gr = _table_grads(c, direction, g_a, g_p, g_t)
        want_e, want_r = c[f"grad64_klw_{direction}_rows"]
        what = f"{name} L{l_norm:g} weighted kl {direction}"
        _close(ge, want_e, what + " entity vs float64 autograd")
        _close(gr, want_r, what + " relation vs float64 autograd")
        dls = np.exp(x - _lse64(x)[:, None]) - w.astype(np.float64)[:, None] * y
        gout = (dls * c["g_rows"].astype(np.float64)[:, None]).astype(np.float32)
        u_a, u_p, u_t = eng.score_pairs_bwd(T, direction, ai, pi, None, _t(gout), sc)
        for nm, got, want in (("g_a", g_a, u_a), ("g_p", g_p, u_p), ("g_tgt", g_t, u_t)):
            _close(got.double().cpu().numpy(), want.double().cpu().numpy(), f"{what} {nm} vs score_pairs_bwd")


@pytest.mark.parametrize("name,l_norm", [("transe", 1.0), ("transe", 2.0), ("rotate", 1.0), ("rotate", 2.0)])
@pytest.mark.parametrize("d,E,R,n", [(128, 1037, 13, 203), (64, 64 * 14 + 1, 5, 130)])
def test_chunkings_agree(eng, name, l_norm, d, E, R, n):
    """chunk_cols 64, 128 and E rounded up (one chunk): every output within 2e-4 max(1, |want|max) of the single-chunk
    result; g_tgt BIT-equal (the label mask keeps a target row's gradient one chain over the query rows in order)."""
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    w = _t(np.random.default_rng(6).uniform(0.05, 1.0, n).astype(np.float32))
    for direction in DIRECTIONS:
        a = c["s"] if direction == "sp" else c["o"]
        ai, pi = _t(a), _t(c["p"])
        csr = tuple(_t(x) for x in c["csr_" + direction])
        for kind, extra in (("kl", {}), ("kl", {"label_weight": w}), ("bce", {})):
            lse = _fwd(eng, kind, T, direction, ai, pi, csr, OFFSET, extra.get("label_weight"))[1]
            one = _bwd(eng, kind, T, direction, ai, pi, csr, lse, OFFSET, g_rows=_t(c["g_rows"]),
                       chunk_cols=(E + 63) // 64 * 64, **extra)
            for cc in (64, 128):
                got = _bwd(eng, kind, T, direction, ai, pi, csr, lse, OFFSET, g_rows=_t(c["g_rows"]), chunk_cols=cc, **extra)
                for nm, x, wnt in zip(("g_a", "g_p", "g_tgt"), got, one):
                    _close(x.double().cpu().numpy(), wnt.double().cpu().numpy(), f"{name} {kind} {direction} chunk {cc} {nm}")
                assert torch.equal(got[2], one[2]), f"g_tgt differs between chunk_cols {cc} and one chunk"


def _raw_call(eng, kind, T, direction, a, p, csr, n, E, d, dr, chunk_cols, g_rows, ws=None):
    """forward + backward through ctypes on outputs and a workspace with guards; returns the guarded buffers."""
    from kge_amd import _lib
    from kge_amd._lib import PO_, SP_
    lib = _lib.lib()
    tc = T.c()
    keep = []
    ai, pi = (eng._index(x, T.device, keep) for x in (a, p))
    need = lib.kge_multilabel_dist_workspace_bytes(ctypes.byref(tc), n, chunk_cols)
    assert need > 0 and need % 256 == 0
    S = 7.25  # sentinel
    if ws is None:
        ws = torch.full((need + 4096,), 0x5A, dtype=torch.uint8, device=DEV)
    rows = torch.full((2, n + 2), S, device=DEV)                    # loss_rows, lse with a guard on either side
    gt = torch.full((E + 2, d), S, device=DEV)                      # g_tgt is dense [E, d]: guard rows
    ga, gp = torch.full((n + 2, d), S, device=DEV), torch.full((n + 2, dr), S, device=DEV)
    st = eng._stream(T.device)
    dirc = SP_ if direction == "sp" else PO_
    rp, cl = csr[0].data_ptr(), csr[1].data_ptr()
    if kind == "kl":
        _lib.check(lib.kge_kl_dist_fwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, None, rows[0, 1:].data_ptr(),
                                       rows[1, 1:].data_ptr(), ws.data_ptr(), need, st), "fwd")
        _lib.check(lib.kge_kl_dist_bwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, None, rows[1, 1:].data_ptr(),
                                       g_rows.data_ptr(), 1.0, ga[1:].data_ptr(), gp[1:].data_ptr(), gt[1:].data_ptr(),
                                       ws.data_ptr(), need, st), "bwd")
    else:
        _lib.check(lib.kge_bce_dist_fwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, OFFSET, rows[0, 1:].data_ptr(),
                                        ws.data_ptr(), need, st), "fwd")
        _lib.check(lib.kge_bce_dist_bwd(ctypes.byref(tc), dirc, ai, pi, n, rp, cl, OFFSET, g_rows.data_ptr(), 1.0,
                                        ga[1:].data_ptr(), gp[1:].data_ptr(), gt[1:].data_ptr(), ws.data_ptr(), need, st),
                   "bwd")
    torch.cuda.synchronize()
    return S, ws, need, rows, ga, gp, gt


def _chunk_and_mask_offset(T, n, E, ws_bytes):
    """(C, byte offset of the label mask) as the backward derives them from `ws_bytes` (include/kge_amd.h: records |
    [n, dim] | [n, C] scores | n C / 8 bytes of bits, each part on 256 bytes; C the largest multiple of 64 that fits, at
    most E rounded up).  The first two parts are those of kge_ce_dist_workspace_bytes."""
    from kge_amd import _lib
    al = lambda b: -(-b // 256) * 256
    head = _lib.lib().kge_ce_dist_workspace_bytes(ctypes.byref(T.c()), n, 64) - al(4 * n * 64)
    left = ws_bytes - head
    C = min(left // n * 8 // 33 // 64 * 64, (E + 63) // 64 * 64)
    while C >= 64 and al(4 * n * C) + al(n * C // 8) > left:
        C -= 64
    return C, head + al(4 * n * C)


@pytest.mark.parametrize("kind", ["kl", "bce"])
@pytest.mark.parametrize("name,l_norm,d,E,R,n", [("transe", 1.0, 33, 150, 5, 37), ("rotate", 2.0, 64, 64 * 14 + 1, 5, 130),
                                                 ("transe", 2.0, 32, 70, 3, 1)])
def test_guards_workspace_tail_and_the_mask(eng, kind, name, l_norm, d, E, R, n):
    """Guard rows of every output and the workspace tail stay untouched; the label mask (n C / 8 bytes behind the score
    block, C as the backward derives it) is all zero after the call; a second call on the SAME workspace gives the forward
    bit for bit and the backward within _close."""
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    for direction, cc in (("sp", 0), ("po", 64)):
        a = c["s"] if direction == "sp" else c["o"]
        csr = tuple(_t(x) for x in c["csr_" + direction])
        args = (eng, kind, T, direction, _t(a), _t(c["p"]), csr, n, E, d, c["dr"], cc, _t(c["g_rows"]))
        S, ws, need, rows, ga, gp, gt = _raw_call(*args)
        assert bool((ws[need:] == 0x5A).all()), "workspace tail written"
        C, mask0 = _chunk_and_mask_offset(T, n, E, need)
        assert C >= (cc or 64) and C % 64 == 0 and mask0 + n * C // 8 <= need
        assert bool((ws[mask0:mask0 + n * C // 8] == 0).all()), "label mask not left zero"
        # (the 0x5A fill is gone from the whole mask, so it was written, and the padding behind it kept the fill)
        assert bool((ws[mask0 + n * C // 8:need] == 0x5A).all()), "padding behind the mask written"
        assert bool((rows[0, 0] == S)) and bool((rows[:, n + 1] == S).all()), "loss_rows / lse guards"
        if kind == "bce":
            assert bool((rows[1] == S).all()), "bce writes no lse"
        for nm, x, r in (("g_a", ga, n), ("g_p", gp, n), ("g_tgt", gt, E)):
            assert bool((x[0] == S).all()) and bool((x[r + 1] == S).all()), nm + " guard rows"
            assert bool(torch.isfinite(x[1:r + 1]).all()) and not bool((x[1:r + 1] == S).any()), nm + ": not written"
        lse = rows[1, 1:n + 1].contiguous()
        want = _bwd(eng, kind, T, direction, _t(a), _t(c["p"]), csr, lse, OFFSET, g_rows=_t(c["g_rows"]), chunk_cols=cc)
        assert torch.equal(gt[1:E + 1], want[2])
        _close(ga[1:n + 1].double().cpu().numpy(), want[0].double().cpu().numpy(), "g_a raw vs engine")
        _close(gp[1:n + 1].double().cpu().numpy(), want[1].double().cpu().numpy(), "g_p raw vs engine")
        again = _raw_call(*args, ws=ws)
        assert torch.equal(again[3], rows), "forward on a reused workspace differs"
        assert torch.equal(again[6], gt), "g_tgt on a reused workspace differs"
        _close(again[4][1:n + 1].double().cpu().numpy(), ga[1:n + 1].double().cpu().numpy(), "g_a on a reused workspace")
        _close(again[5][1:n + 1].double().cpu().numpy(), gp[1:n + 1].double().cpu().numpy(), "g_p on a reused workspace")
    # too small a workspace is refused
    from kge_amd import _lib
    lib, tc, keep = _lib.lib(), T.c(), []
    ix = [eng._index(x, T.device, keep) for x in (_t(c["s"]), _t(c["p"]))]
    small = lib.kge_multilabel_dist_workspace_bytes(ctypes.byref(tc), n, 64) - 256
    P = ws.data_ptr()
    assert lib.kge_bce_dist_bwd(ctypes.byref(tc), _lib.SP_, *ix, n, csr[0].data_ptr(), csr[1].data_ptr(), 0.0, None, 1.0,
                                ga.data_ptr(), gp.data_ptr(), gt.data_ptr(), P, small, eng._stream(T.device)) == -5


def test_int32_strided_empty_and_bad_labels(eng):
    name, l_norm, d, E, R, n = "rotate", 2.0, 40, 150, 5, 37
    c = _case(name, l_norm, d, E, R, n)
    T = _tables(eng, name, l_norm, c)
    rowptr, col = c["csr_sp"]
    csr = (_t(rowptr), _t(col))
    tri = np.stack([c["s"], c["p"], c["o"]], 1)
    t32, t64 = _t(tri.astype(np.int32)), _t(tri)
    for kind in ("kl", "bce"):
        loss, lse = _fwd(eng, kind, T, "sp", t32[:, 0], t32[:, 1], (csr[0].int(), csr[1].int()), OFFSET)
        loss64, lse64 = _fwd(eng, kind, T, "sp", t64[:, 0].contiguous(), t64[:, 1].contiguous(), csr, OFFSET)
        assert torch.equal(loss, loss64) and (lse is None or torch.equal(lse, lse64))
        g32 = _bwd(eng, kind, T, "sp", t32[:, 0], t32[:, 1], csr, lse, OFFSET, g_rows=_t(c["g_rows"]))
        g64 = _bwd(eng, kind, T, "sp", t64[:, 0].contiguous(), t64[:, 1].contiguous(), csr, lse64, OFFSET,
                   g_rows=_t(c["g_rows"]))
        assert torch.equal(g32[2], g64[2])
        for x, w in zip(g32[:2], g64[:2]):
            _close(x.double().cpu().numpy(), w.double().cpu().numpy(), kind + " int32 strided vs int64")
        # n = 0
        e, rp0 = torch.zeros(0, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        l0, s0 = _fwd(eng, kind, T, "po", e, e, (rp0, e), OFFSET)
        assert l0.shape == (0,) and (s0 is None or s0.shape == (0,))
        g0 = _bwd(eng, kind, T, "po", e, e, (rp0, e), s0, OFFSET)
        assert g0[0].shape == (0, d) and g0[1].shape == (0, c["dr"]) and g0[2].shape == (E, d)
        assert float(g0[2].abs().max()) == 0.0
        # labels out of range: NaN in those rows only, lse and the other rows untouched; the backward ignores them
        bad = col.copy()
        bad[rowptr[4] + 2], bad[rowptr[9]] = E, -1
        lb, sb = _fwd(eng, kind, T, "sp", t64[:, 0].contiguous(), t64[:, 1].contiguous(), (csr[0], _t(bad)), OFFSET)
        nan = torch.isnan(lb).cpu().numpy()
        assert nan.tolist() == [i in (4, 9) for i in range(n)]
        assert sb is None or torch.equal(sb, lse64)
        assert torch.equal(lb[~torch.isnan(lb)], loss64[torch.from_numpy(~nan).to(DEV)])
        gb = _bwd(eng, kind, T, "sp", t64[:, 0].contiguous(), t64[:, 1].contiguous(), (csr[0], _t(bad)), lse64, OFFSET)
        assert all(bool(torch.isfinite(x).all()) for x in gb)


def test_unsupported_tables_are_refused(eng):
    ent, rel = torch.randn(70, 64, device=DEV), torch.randn(3, 64, device=DEV)
    ix = torch.zeros(4, dtype=torch.int64, device=DEV)
    rp, cl = torch.arange(5, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV)
    from kge_amd import _lib
    lib = _lib.lib()
    for T in (eng.Tables("complex", ent, rel), eng.Tables("transe", ent.bfloat16(), rel.bfloat16()),
              eng.Tables("transe", ent, rel, 3.0)):
        assert lib.kge_multilabel_dist_workspace_bytes(ctypes.byref(T.c()), 4, 0) == 0
        with pytest.raises(RuntimeError):
            eng.kl_dist_fwd(T, "sp", ix, ix, rp, cl)
        with pytest.raises(RuntimeError):
            eng.bce_dist_bwd(T, "sp", ix, ix, rp, cl)
        # the C entries themselves: refused with nothing written
        keep, out = [], torch.full((3, 8), 7.25, device=DEV)
        ai = eng._index(ix, T.device, keep)
        ws = torch.full((1 << 16,), 0x5A, dtype=torch.uint8, device=DEV)
        assert lib.kge_kl_dist_fwd(ctypes.byref(T.c()), 1, ai, ai, 4, rp.data_ptr(), cl.data_ptr(), None, out[0].data_ptr(),
                                   out[1].data_ptr(), ws.data_ptr(), 1 << 16, eng._stream(T.device)) == -2
        assert lib.kge_bce_dist_fwd(ctypes.byref(T.c()), 1, ai, ai, 4, rp.data_ptr(), cl.data_ptr(), 0.0, out[2].data_ptr(),
                                    ws.data_ptr(), 1 << 16, eng._stream(T.device)) == -2
        torch.cuda.synchronize()
        assert bool((out == 7.25).all()) and bool((ws == 0x5A).all())
    assert lib.kge_multilabel_dist_workspace_bytes(ctypes.byref(eng.Tables("transe", ent, rel, 2.0).c()), 4, 0) > 0


def _random_csr(n, E, gen, mean=8):
    k = torch.randint(0, 2 * mean + 1, (n,), generator=gen)
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(k, 0)
    col = torch.cat([torch.randperm(E, generator=gen)[:int(x)] for x in k])
    return rowptr.to(DEV), col.to(DEV)


@pytest.mark.parametrize("kind", ["kl", "bce"])
def test_memory_bound_and_agreement_of_a_model_step(kind):
    """n = 256, E = 131,072, d = 16: one [n, E] float32 matrix is 128 MB (the composed path holds several).  The fused
    KvsAll step raises max_memory_allocated by less than 64 MB over what is held after a warm-up step (the cached
    workspace, .grad).  The same step fused and composed: per-row losses and parameter gradients within
    2e-4 max(1, |want|max), the bound of the backward tests; the fused rows also within 1e-5 + 1e-5 |want| of the composed
    loss taken in float64 on the stored scores.  (The composed float32 bce is the less exact of the two where every
    softplus term is near 1e-7: on a row without labels, loss 0.0147, fused and composed float32 differed by 1.8e-3.)"""
    from kge_amd import model as km
    E, R, d, n = 131072, 7, 16, 256
    torch.manual_seed(0)
    m = km.create("transe", E, R, d, device=DEV, fused_dist_loss=True).train()
    g = torch.Generator().manual_seed(1)
    s, p = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R))
    rowptr, col = _random_csr(n, E, g)
    step = (lambda: m.kl_loss_sp(s, p, rowptr, col)) if kind == "kl" else (lambda: m.bce_loss_sp(s, p, rowptr, col, 2.0))
    assert m._ce_dist_tables() is not None
    step().sum().backward()  # warm-up: workspace and .grad exist from here on
    torch.cuda.synchronize()
    m.zero_grad(set_to_none=False)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    rows = step()
    rows.sum().backward()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"fused {kind} step: peak rise {rise / 2**20:.1f} MB over {base / 2**20:.1f} MB held")
    assert bool(torch.isfinite(rows).all()) and rise < 64 * 2**20, rise
    we, wr = m.get_s_embedder().weight, m.get_p_embedder().weight
    fused = (rows.detach().clone(), we.grad.clone(), wr.grad.clone())
    m.fused_dist_loss = False
    assert m._ce_dist_tables() is None
    m.zero_grad(set_to_none=False)
    rows_c = step()
    rows_c.sum().backward()
    _close(fused[0].double().cpu().numpy(), rows_c.detach().double().cpu().numpy(), kind + " loss rows fused vs composed")
    # the fused rows against the composed loss in float64 on the stored float32 scores: 1e-5 + 1e-5 |want|
    with torch.no_grad():
        sc64 = m.score_sp(s, p).double()
        want = (km.KgeModel._kl_composed(sc64, rowptr, col) if kind == "kl"
                else km.KgeModel._bce_composed(sc64, rowptr, col, 2.0))
    err, tol = (fused[0].double() - want).abs(), 1e-5 + 1e-5 * want.abs()
    print(f"{kind} loss rows fused vs float64 composed: max err {float(err.max()):.3e} min tol {float(tol.min()):.3e}")
    assert bool((err <= tol).all()), (float(err.max()), int((err > tol).sum()))
    _close(fused[1].double().cpu().numpy(), we.grad.double().cpu().numpy(), kind + " entity gradient fused vs composed")
    _close(fused[2].double().cpu().numpy(), wr.grad.double().cpu().numpy(), kind + " relation gradient fused vs composed")


def test_model_po_direction_and_label_smoothing_declines(monkeypatch):
    """kl_loss_po / bce_loss_po take the fused functions too; label smoothing declines to the composed path"""
    from kge_amd import model as km
    E, R, d, n = 515, 5, 32, 70
    torch.manual_seed(0)
    m = km.create("rotate", E, R, d, l_norm=2.0, device=DEV, fused_dist_loss=True).train()
    g = torch.Generator().manual_seed(3)
    o, p = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R))
    rowptr, col = _random_csr(n, E, g, mean=4)
    entered = []
    for cls in (km._FusedKLDist, km._FusedBCEDist):
        def forward(ctx, *a, _orig=cls.forward, _name=cls.__name__):
            entered.append(_name)
            return _orig(ctx, *a)
        monkeypatch.setattr(cls, "forward", staticmethod(forward))
    res = {}
    for fused in (True, False):
        m.fused_dist_loss = fused
        res[fused] = (m.kl_loss_po(p, o, rowptr, col), m.bce_loss_po(p, o, rowptr, col, 1.5))
    assert entered == ["_FusedKLDist", "_FusedBCEDist"], entered
    for a, b in zip(res[True], res[False]):
        assert bool(((a - b).abs() <= 1e-5 + 1e-5 * b.abs()).all())
    m.fused_dist_loss = True
    m.kl_loss_sp(o, p, rowptr, col, 0.1), m.bce_loss_sp(o, p, rowptr, col, 0.0, 0.1)
    assert len(entered) == 2, "label smoothing must take the composed path"
