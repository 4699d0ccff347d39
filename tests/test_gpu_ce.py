"""Fused 1vsAll loss (kge_ce_fwd / kge_ce_bwd) on the GPU, through the C ABI.

What is compared (tolerances stated at each assert):
  * forward against float64 cross entropy of the scores kge_score_sp / kge_score_po write for the
    same inputs (the kernel's scores are bit-identical inside both; what differs is f32 exp / log /
    summation): |diff| <= 1e-5 + 1e-5 |ref|;
  * forward against float64 cross entropy of the ORACLE's bf16-semantics scores: the bf16 score
    tolerance of test_gpu_parity.py (1e-5 * max(1, rms) + 1e-4 |score|), which a log-sum-exp
    propagates at most 1:1, twice (lse and the label's score);
  * backward against float64 gradients of the same loss on the same (bf16-valued) tables:
    d loss / d score and the query matrix are rounded to bf16 before the two products (the
    mixed-precision backward), so relative error in the Frobenius norm <= 1e-2; and
    against the unfused mixed-precision backward (kge_score_pairs_bwd on the softmax gradient
    computed by torch from the written scores), which rounds the same way: <= 2e-3.
"""
import numpy as np
import pytest
import torch

import oracle as ko

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _tables(eng, model, ent, rel):
    return eng.Tables(model, torch.from_numpy(ent).to(torch.bfloat16).to(DEV),
                      torch.from_numpy(rel).to(torch.bfloat16).to(DEV), 1.0)


def _ce64(scores, label):
    """float64 (loss_rows, lse) of scores [n, E] with index labels"""
    x = np.asarray(scores, dtype=np.float64)
    mx = x.max(axis=1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    return lse - x[np.arange(len(label)), label], lse


def _case(seed, model, d, E, R, n, scale=1.0):
    rng = np.random.default_rng(seed)
    ent = (rng.standard_normal((E, d)) * scale).astype(np.float32)
    rel = (rng.standard_normal((R, d)) * scale).astype(np.float32)
    s, p, o = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    return ent, rel, s, p, o


CASES = [
    ("complex", 512, 1037, 13, 203, 0.3),     # ragged rows and columns
    ("distmult", 256, 1037, 13, 203, 0.5),
    ("complex", 128, 70, 3, 1, 1.0),          # one row, one column group, one ragged tile
    ("distmult", 128, 64, 3, 33, 1.0),        # exactly one full tile
    ("complex", 512, 14541, 237, 512, 0.1),   # BASELINE configs[1] shape (C2)
    ("complex", 256, 20000, 50, 700, 0.2),    # six row groups
    # m % 64 <= 4 with one tile per column group: half the lanes of the last workgroup see nothing but padding
    # (their running max stays -inf; this was a NaN loss for every row until round 2)
    ("complex", 256, 900, 5, 64, 0.3),
    ("distmult", 512, 14 * 64 + 1, 5, 130, 0.3),
]


@pytest.mark.parametrize("model,d,E,R,n,scale", CASES)
def test_ce_fwd(eng, model, d, E, R, n, scale):
    """Tolerances on random, near-uniform rows (module docstring).  The elementwise claim -- lse and loss_rows inside a
    bound counted from the epilogues, on rows whose max rises late, spikes, ties and |score| >= 100 -- is asserted in
    tests/test_gpu_ce16_bound.py."""
    ent, rel, s, p, o = _case(d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    O = ko.Tables(model, ko.f32_to_bf16(ent), ko.f32_to_bf16(rel), 1.0)
    for direction, a, lab in (("sp", s, o), ("po", o, s)):
        loss, lse = eng.ce_fwd(T, direction, _t(a), _t(p), _t(lab))
        loss, lse = loss.cpu().numpy().astype(np.float64), lse.cpu().numpy().astype(np.float64)
        assert np.isfinite(loss).all() and (loss >= 0).all(), direction
        # (1) the kernel's own scores
        sc = (eng.score_sp(T, _t(a), _t(p)) if direction == "sp" else eng.score_po(T, _t(p), _t(a))).cpu().numpy()
        want_loss, want_lse = _ce64(sc, lab)
        for nm, got, want in (("lse", lse, want_lse), ("loss", loss, want_loss)):
            err = np.abs(got - want)
            tol = 1e-5 + 1e-5 * np.abs(want)
            assert (err <= tol).all(), (direction, nm, float(err.max()), int((err > tol).sum()))
        # (2) the oracle's scores (bf16 semantics of the matrix-core path)
        osc = ko.score_sp(O, a, p) if direction == "sp" else ko.score_po(O, p, a)
        o_loss, o_lse = _ce64(osc, lab)
        rms = max(1.0, float(np.sqrt(np.mean(np.square(osc.astype(np.float64))))))
        stol = 1e-5 * rms + 1e-4 * np.abs(osc).max(axis=1)   # per-row bound on a score's tolerance
        assert (np.abs(lse - o_lse) <= stol + 1e-5).all(), (direction, float(np.abs(lse - o_lse).max()))
        assert (np.abs(loss - o_loss) <= 2 * stol + 1e-5).all(), (direction, float(np.abs(loss - o_loss).max()))


def test_ce_fwd_strided_int32_indices_and_repeats(eng):
    """indices as the reference passes them: columns of an int32 [n, 3] triple tensor
    (train_1vsAll.py:64: triples[:, 0], triples[:, 1]); repeated calls give identical bits."""
    ent, rel, s, p, o = _case(7, "complex", 256, 3000, 11, 300, 0.3)
    T = _tables(eng, "complex", ent, rel)
    tri = torch.from_numpy(np.stack([s, p, o], axis=1)).to(torch.int32).to(DEV)
    a = eng.ce_fwd(T, "sp", tri[:, 0], tri[:, 1], tri[:, 2])
    b = eng.ce_fwd(T, "sp", _t(s), _t(p), _t(o))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for _ in range(5):
        c = eng.ce_fwd(T, "sp", tri[:, 0], tri[:, 1], tri[:, 2])
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])


def _grads64(model, ent16, rel16, a, p, lab, direction, g):
    """float64 autograd of sum_i g_i * CE_i on the bf16-valued tables (torch CPU)."""
    e = ent16.double().requires_grad_(True)
    r = rel16.double().requires_grad_(True)
    ea, rp = e[a], r[p]
    h = e.shape[1] // 2
    if model == "distmult":
        q = ea * rp
    else:
        are, aim, rre, rim = ea[:, :h], ea[:, h:], rp[:, :h], rp[:, h:]
        if direction == "sp":   # Re<s, r, conj(o)>: q = s * r
            q = torch.cat([are * rre - aim * rim, are * rim + aim * rre], dim=1)
        else:                   # as a function of s: q = conj(r) * o
            q = torch.cat([are * rre + aim * rim, aim * rre - are * rim], dim=1)
    sc = q @ e.t()
    loss = (torch.nn.functional.cross_entropy(sc, lab, reduction="none") * g).sum()
    loss.backward()
    return e.grad, r.grad


@pytest.mark.parametrize("model,d,E,R,n,scale", CASES[:2] + CASES[4:5] + CASES[6:8])
def test_ce_bwd(eng, model, d, E, R, n, scale):
    """kge_ce_bwd against float64 autograd (norm-wise) and against the unfused mixed-precision backward,
    score_pairs_bwd on bf16 tables.  Both are coarse: the ELEMENTWISE claim -- G16 as the V3_DS epilogues write it (not
    the cast of a given gout that tests/test_gpu_pairs_bwd16.py feeds) and the three gradients, against float64 inside a
    derived bound on planted inputs -- is asserted in tests/test_gpu_ce16_bound.py."""
    ent, rel, s, p, o = _case(3 * d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    rng = np.random.default_rng(1)
    g_rows = (rng.random(n).astype(np.float32) + 0.5) / n
    for direction, a, lab in (("sp", s, o), ("po", o, s)):
        ta, tp, tl = _t(a), _t(p), _t(lab)
        loss, lse = eng.ce_fwd(T, direction, ta, tp, tl)
        g_a, g_p, g_t = eng.ce_bwd(T, direction, ta, tp, tl, lse, g_rows=_t(g_rows))
        ge = g_t.clone()
        ge.index_add_(0, ta, g_a)
        gr = torch.zeros(R, d, device=DEV).index_add_(0, tp, g_p)
        # float64 reference
        we, wr = _grads64(model, T.ent.cpu(), T.rel.cpu(), torch.from_numpy(a), torch.from_numpy(p),
                          torch.from_numpy(lab), direction, torch.from_numpy(g_rows).double())
        for nm, got, want in (("ent", ge, we), ("rel", gr, wr)):
            got = got.cpu().double()
            rel_err = float((got - want).norm() / want.norm())
            assert rel_err <= 1e-2, (direction, nm, rel_err)
        # the unfused mixed-precision backward on torch's softmax gradient of the written scores
        sc = eng.score_sp(T, ta, tp) if direction == "sp" else eng.score_po(T, tp, ta)
        ds = torch.softmax(sc, dim=1)
        ds[torch.arange(n, device=DEV), tl] -= 1.0
        ds *= _t(g_rows)[:, None]
        u_a, u_p, u_t = eng.score_pairs_bwd(T, direction, ta, tp, None, ds)
        for nm, got, want in (("g_a", g_a, u_a), ("g_p", g_p, u_p), ("g_t", g_t, u_t)):
            rel_err = float((got - want).norm() / want.norm())
            assert rel_err <= 2e-3, (direction, nm, rel_err)
        # scalar upstream gradient == a constant row vector
        c_a, c_p, c_t = eng.ce_bwd(T, direction, ta, tp, tl, lse, g_scalar=1.0 / n)
        v_a, v_p, v_t = eng.ce_bwd(T, direction, ta, tp, tl, lse, g_rows=torch.full((n,), 1.0 / n, device=DEV))
        assert torch.equal(c_a, v_a) and torch.equal(c_p, v_p) and torch.equal(c_t, v_t)


@pytest.mark.parametrize("model,d,E,R,n,scale", CASES[:2] + CASES[4:5] + CASES[6:8])
def test_fused_loss_on_both_kernel_generations(eng, monkeypatch, model, d, E, R, n, scale, kge_switch):
    """The forward (V3_LSE) and the gradient pass (V3_DS / V3_DSIG) run on the loader/consumer kernel for
    d in {256, 512} and on the single-role kernel otherwise; KGE_CE_V3=1 forces the latter.  Same tiles, same
    chains, same per-lane order: the two must agree to float32 rounding of the merged row statistics, one-
    and two-sided, cross entropy and BCE."""
    ent, rel, s, p, o = _case(7 * d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    ts, tp, to = _t(s), _t(p), _t(o)
    rowptr = torch.arange(n + 1, device=DEV, dtype=torch.int64)

    def run():
        loss, lse = eng.ce_fwd(T, "sp", ts, tp, to)
        grads = eng.ce_bwd(T, "sp", ts, tp, to, lse, g_scalar=1.0 / n)
        l2, z2 = eng.ce_sp_po_fwd(T, ts, tp, to)
        g2 = eng.ce_sp_po_bwd(T, ts, tp, to, z2, g_scalar=1.0 / n)
        bl = eng.bce_fwd(T, "po", to, tp, rowptr, ts, -0.25)
        bg = eng.bce_bwd(T, "po", to, tp, rowptr, ts, -0.25, g_scalar=1.0 / n)
        return [loss, lse, *grads, l2, z2, *g2, bl, *bg]

    kge_switch.set("CE_V3", "0")
    new = run()
    kge_switch.set("CE_V3", "1")
    old = run()
    # (round 6: for more than 128 rows at d in {256, 512} the default is pairs_bf16_v8_ce_kernel, whose exponentials are
    # taken in the log2 domain -- values that were rounded to bf16 (the gradients' G16) then differ in a few elements per
    # row by one bf16 step: 2e-4 of the largest entry; see test_persistent_loss_kernel_equals_the_loader_consumer_kernel)
    v8 = n > 128 and d in (256, 512)
    for k, (a_, b_) in enumerate(zip(new, old)):
        assert a_.shape == b_.shape and not torch.isnan(a_).any(), k
        den = float(b_.abs().max()) + 1e-30
        grad = a_.dim() == 2
        tol = (2e-4 * den if grad else 3e-6 * den + 2e-6) if v8 else 2e-6 * den + 1e-7
        assert float((a_ - b_).abs().max()) <= tol, (k, float((a_ - b_).abs().max()), den)


V8_CASES = [
    ("complex", 512, 14541, 237, 512, 0.1),   # BASELINE configs[1] shape: 4 (side, chunk) pairs x 64 column groups
    ("complex", 512, 1037, 13, 203, 0.3),     # a table of 33 units: most workgroups' ranges are empty
    ("distmult", 256, 1037, 13, 203, 0.5),    # d = 256: two sub-units per unit, ragged second sub-unit
    ("complex", 256, 20000, 50, 700, 0.2),    # three chunks per side
    ("distmult", 512, 14 * 64 + 1, 5, 130, 0.3),
    ("complex", 512, 100, 3, 40, 0.5),        # (forced) four units, 40 of a chunk's 256 rows
    ("complex", 256, 33, 3, 300, 0.5),        # (forced) ONE ragged unit, two chunks
    ("distmult", 512, 4097, 7, 1100, 0.2),    # more pairs than workgroups per XCD would be n > 4096: here 10 pairs
]


@pytest.mark.parametrize("model,d,E,R,n,scale", V8_CASES)
def test_persistent_loss_kernel_equals_the_loader_consumer_kernel(eng, model, d, E, R, n, scale, kge_switch):
    """Round 6: the forward (V3_LSE) and gradient (V3_DS) passes of the fused 1vsAll / KvsAll losses on
    pairs_bf16_v8_ce_kernel (ce_pairs_v8.hip: prepared query fragments, persistent grid, two consumer waves per SIMD,
    online softmax in the log2 domain) against pairs_bf16_v4_kernel's (switch CE_V8 = 0): the same score bits inside
    both; the row statistics differ by float32 rounding of exp2 / the merge order of the column groups (<= 3e-6
    relative), d loss / d score by that before its rounding to bf16 -- a few elements per row land on the other side
    of a bf16 rounding boundary (2^-8 of ONE element of a sum over all entities): gradients to 2e-4 of their largest
    entry.  One- and two-sided, index labels at the table's first and last column, multi-label (KvsAll) rows."""
    ent, rel, s, p, o = _case(11 * d + n + E, model, d, E, R, n, scale)
    o[0], o[-1], s[0], s[-1] = 0, E - 1, E - 1, 0  # labels at both ends of the table
    T = _tables(eng, model, ent, rel)
    ts, tp, to = _t(s), _t(p), _t(o)
    rng = np.random.default_rng(n)
    cnt = rng.integers(0, 4, n)
    cnt[0] = 0  # a row without labels
    rowptr = torch.from_numpy(np.concatenate([[0], np.cumsum(cnt)])).to(DEV)
    col = torch.from_numpy(np.concatenate([np.sort(rng.choice(E, c, replace=False)) for c in cnt] + [np.zeros(0, int)])
                           .astype(np.int64)).to(DEV)

    def run():
        loss, lse = eng.ce_fwd(T, "sp", ts, tp, to)
        grads = eng.ce_bwd(T, "sp", ts, tp, to, lse, g_scalar=1.0 / n)
        lp, zp = eng.ce_fwd(T, "po", to, tp, ts)
        l2, z2 = eng.ce_sp_po_fwd(T, ts, tp, to)
        g2 = eng.ce_sp_po_bwd(T, ts, tp, to, z2, g_rows=torch.linspace(0.5, 1.5, 2 * n, device=DEV) / n)
        kl, kz = eng.kl_fwd(T, "sp", ts, tp, rowptr, col)
        kg = eng.kl_bwd(T, "sp", ts, tp, rowptr, col, kz, g_scalar=1.0 / n)
        return [loss, lse, lp, zp, l2, z2, kl, kz], [*grads, *g2, *kg]

    kge_switch.set("CE_V8", 1)
    new_f, new_g = run()
    kge_switch.set("CE_V8", 0)
    old_f, old_g = run()
    for k, (a_, b_) in enumerate(zip(new_f, old_f)):
        assert a_.shape == b_.shape and torch.isfinite(a_).all(), k
        err = (a_.double() - b_.double()).abs()
        assert bool((err <= 3e-6 * b_.double().abs() + 2e-6).all()), (k, float(err.max()))
    for k, (a_, b_) in enumerate(zip(new_g, old_g)):
        assert a_.shape == b_.shape and torch.isfinite(a_).all(), k
        den = float(b_.abs().max()) + 1e-30
        assert float((a_ - b_).abs().max()) <= 2e-4 * den, (k, float((a_ - b_).abs().max()), den)
    assert torch.equal(new_f[1][:n], new_f[5][:n]) or float((new_f[1] - new_f[5][:n]).abs().max()) <= 3e-6 * float(new_f[1].abs().max()) + 2e-6


def test_ce_unsupported_tables_fail_loudly(eng):
    ent, rel, s, p, o = _case(11, "complex", 128, 100, 3, 10)
    Tf = eng.Tables("complex", torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV), 1.0)
    assert not eng.ce_supported(Tf)
    with pytest.raises(RuntimeError):
        eng.ce_fwd(Tf, "sp", _t(s), _t(p), _t(o))
    Tt = eng.Tables("transe", torch.from_numpy(ent).to(torch.bfloat16).to(DEV),
                    torch.from_numpy(rel).to(torch.bfloat16).to(DEV), 1.0)
    assert not eng.ce_supported(Tt)
    with pytest.raises(RuntimeError):
        eng.ce_fwd(Tt, "sp", _t(s), _t(p), _t(o))


@pytest.mark.parametrize("name", ["complex", "distmult"])
def test_model_level_fused_loss_against_composed_loss(name):
    """KgeModel.loss_sp / loss_po (mixed precision: f32 parameters, bf16 scoring) against the same
    model's score_sp / score_po + CrossEntropyLoss(reduction="sum") / batch_size, the reference's
    1vsAll step (train_1vsAll.py:64-81): loss values to f32 rounding (the scores inside are the same
    bits), parameter gradients within the bf16 rounding both backward paths apply."""
    from kge_amd import model as km
    E, R, d, n = 3000 + 5, 11, 256, 300
    torch.manual_seed(0)
    m = km.create(name, E, R, d, device=DEV, score_dtype=torch.bfloat16)
    assert m._ce_tables() is not None
    g = torch.Generator().manual_seed(2)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    for fused, composed in ((lambda: m.loss_sp(s, p, o), lambda: torch.nn.functional.cross_entropy(m.score_sp(s, p), o, reduction="sum")),
                            (lambda: m.loss_po(p, o, s), lambda: torch.nn.functional.cross_entropy(m.score_po(p, o), s, reduction="sum"))):
        m.zero_grad()
        lf = fused().sum() / n
        lf.backward()
        gf = [x.grad.clone() for x in m.parameters()]
        m.zero_grad()
        lc = composed() / n
        lc.backward()
        gc = [x.grad.clone() for x in m.parameters()]
        assert abs(float(lf.detach()) - float(lc.detach())) <= 1e-5 * max(1.0, abs(float(lc.detach())))
        for a, b in zip(gf, gc):
            assert a.dtype == b.dtype and a.shape == b.shape
            rel_err = float((a - b).norm() / b.norm())
            assert rel_err <= 2e-3, rel_err
    # f32 scoring (no bf16 copies): the fused path does not apply, the loss is composed
    m32 = km.create(name, E, R, d, device=DEV)
    assert m32._ce_tables() is None
    rows = m32.loss_sp(s, p, o)
    want = torch.nn.functional.cross_entropy(m32.score_sp(s, p), o, reduction="none")
    assert torch.equal(rows, want)


# ---- KvsAll: KL divergence from normalised multi-hot labels (kge_kl_fwd / kge_kl_bwd) --------------
def _kl_case(seed, model, d, E, R, n, scale):
    ent, rel, s, p, o = _case(seed, model, d, E, R, n, scale)
    rng = np.random.default_rng(seed + 1)
    cnt = rng.integers(1, 8, n)
    cnt[rng.integers(0, n)] = min(E, 70)          # one row with many labels
    if n > 2:
        cnt[1] = 0                                # one row without labels: loss 0, gradient 0
    col = np.concatenate([np.sort(rng.choice(E, c, replace=False)) for c in cnt] + [np.zeros(0, np.int64)])
    rowptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return ent, rel, s, p, o, rowptr, col.astype(np.int64)


def _kl64(scores, rowptr, col):
    x = np.asarray(scores, dtype=np.float64)
    mx = x.max(axis=1)
    lse = mx + np.log(np.exp(x - mx[:, None]).sum(axis=1))
    loss = np.zeros(len(x))
    for i in range(len(x)):
        js = col[rowptr[i]:rowptr[i + 1]]
        if len(js):
            loss[i] = lse[i] - x[i, js].mean() - np.log(len(js))
    return loss, lse


@pytest.mark.parametrize("model,d,E,R,n,scale", CASES[:2] + CASES[4:5] + CASES[6:8])
def test_kl_fwd_bwd(eng, model, d, E, R, n, scale):
    """Forward against float64 KL of the written scores (the label scores are re-evaluated in a
    different f32 summation order: + 2e-6 * max|score| per row on top of the CE tolerance) and
    against torch's KLDivLoss(log_softmax, normalize(labels)); backward against float64 autograd of
    that composition (<= 1e-2, bf16 operands) -- the checks of test_ce_bwd, multi-label."""
    ent, rel, s, p, o, rowptr, col = _kl_case(5 * d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    trp, tcl = _t(rowptr), _t(col)
    rng = np.random.default_rng(2)
    g_rows = (rng.random(n).astype(np.float32) + 0.5) / n
    for direction, a in (("sp", s), ("po", o)):
        ta, tp = _t(a), _t(p)
        loss, lse = eng.kl_fwd(T, direction, ta, tp, trp, tcl)
        sc = (eng.score_sp(T, ta, tp) if direction == "sp" else eng.score_po(T, tp, ta)).cpu().numpy()
        want, want_lse = _kl64(sc, rowptr, col)
        got = loss.cpu().numpy().astype(np.float64)
        tol = 1e-5 + 1e-5 * np.abs(want_lse) + 2e-6 * np.abs(sc).max(axis=1)
        assert (np.abs(got - want) <= tol).all(), (direction, float(np.abs(got - want).max()))
        assert (np.abs(lse.cpu().numpy() - want_lse) <= 1e-5 + 1e-5 * np.abs(want_lse)).all()
        if n > 2:
            assert got[1] == 0.0
        # torch's own composition on the written scores (loss.py:208-213)
        tsc = torch.from_numpy(sc).double()
        lab = torch.zeros_like(tsc)
        rows = np.repeat(np.arange(n), np.diff(rowptr))
        lab[torch.from_numpy(rows), torch.from_numpy(col)] = 1.0
        ref = torch.nn.functional.kl_div(torch.log_softmax(tsc, 1), torch.nn.functional.normalize(lab, p=1, dim=1),
                                         reduction="none").sum(1).numpy()
        assert (np.abs(got - ref) <= tol).all(), (direction, float(np.abs(got - ref).max()))
        # backward
        g_a, g_p, g_t = eng.kl_bwd(T, direction, ta, tp, trp, tcl, lse, g_rows=_t(g_rows))
        ge = g_t.clone()
        ge.index_add_(0, ta, g_a)
        gr = torch.zeros(R, d, device=DEV).index_add_(0, tp, g_p)
        e = T.ent.cpu().double().requires_grad_(True)
        r = T.rel.cpu().double().requires_grad_(True)
        ea, rp_ = e[torch.from_numpy(a)], r[torch.from_numpy(p)]
        h = d // 2
        if model == "distmult":
            q = ea * rp_
        elif direction == "sp":
            q = torch.cat([ea[:, :h] * rp_[:, :h] - ea[:, h:] * rp_[:, h:], ea[:, :h] * rp_[:, h:] + ea[:, h:] * rp_[:, :h]], 1)
        else:
            q = torch.cat([ea[:, :h] * rp_[:, :h] + ea[:, h:] * rp_[:, h:], ea[:, h:] * rp_[:, :h] - ea[:, :h] * rp_[:, h:]], 1)
        s64 = q @ e.t()
        l64 = torch.nn.functional.kl_div(torch.log_softmax(s64, 1), torch.nn.functional.normalize(lab, p=1, dim=1),
                                         reduction="none").sum(1)
        (l64 * torch.from_numpy(g_rows).double()).sum().backward()
        for nm, gotg, wantg in (("ent", ge, e.grad), ("rel", gr, r.grad)):
            rel_err = float((gotg.cpu().double() - wantg).norm() / wantg.norm())
            assert rel_err <= 1e-2, (direction, nm, rel_err)
        if n > 2:  # the row without labels contributes nothing
            assert float(g_p[1].abs().max()) == 0.0 and float(g_a[1].abs().max()) == 0.0


@pytest.mark.parametrize("name,ls", [("distmult", 0.0), ("distmult", 0.1), ("complex", 0.3)])
def test_model_level_kl_loss_against_composed(name, ls):
    """Fused KvsAll KL loss (and, ls > 0, its label-smoothed form: train_KvsAll.py:260-266 -- the fused
    kernel's per-row label weight + one linear [n, 1] score + a constant) against the composed
    score -> smooth -> normalise -> KLDivLoss path on the same model; rows without labels included."""
    from kge_amd import model as km
    E, R, d, n = 2000 + 3, 7, 256, 150
    torch.manual_seed(0)
    m = km.create(name, E, R, d, device=DEV, score_dtype=torch.bfloat16)
    ent, rel, s, p, o, rowptr, col = _kl_case(9, name, d, E, R, n, 0.3)
    ts, tp, to, trp, tcl = _t(s), _t(p), _t(o), _t(rowptr), _t(col)
    for fused, composed in ((lambda: m.kl_loss_sp(ts, tp, trp, tcl, ls),
                             lambda: m._kl_composed(m.score_sp(ts, tp), trp, tcl, ls)),
                            (lambda: m.kl_loss_po(tp, to, trp, tcl, ls),
                             lambda: m._kl_composed(m.score_po(tp, to), trp, tcl, ls))):
        m.zero_grad()
        lf = fused().sum() / n
        lf.backward()
        gf = [x.grad.clone() for x in m.parameters()]
        m.zero_grad()
        lc = composed().sum() / n
        lc.backward()
        gc = [x.grad.clone() for x in m.parameters()]
        assert abs(float(lf.detach()) - float(lc.detach())) <= 2e-5 * max(1.0, abs(float(lc.detach())))
        for a_, b_ in zip(gf, gc):
            assert float((a_ - b_).norm() / b_.norm()) <= 2e-3


def test_ce_label_out_of_range_gives_nan_and_empty_batch(eng):
    ent, rel, s, p, o = _case(13, "distmult", 128, 300, 5, 40, 0.5)
    T = _tables(eng, "distmult", ent, rel)
    bad = o.copy()
    bad[3] = 300          # == num_ent: no lane owns this column
    loss, lse = eng.ce_fwd(T, "sp", _t(s), _t(p), _t(bad))
    loss = loss.cpu().numpy()
    assert np.isnan(loss[3]) and np.isfinite(np.delete(loss, 3)).all() and np.isfinite(lse.cpu().numpy()).all()
    e = torch.zeros(0, dtype=torch.int64, device=DEV)
    l0, z0 = eng.ce_fwd(T, "sp", e, e, e)
    assert l0.numel() == 0 and z0.numel() == 0


# ---- both directions at once (kge_ce_sp_po_fwd / _bwd) ---------------------------------------------
@pytest.mark.parametrize("model,d,E,R,n,scale", CASES)
def test_ce_sp_po_equals_the_two_one_sided_calls(eng, model, d, E, R, n, scale):
    """Forward: the [2n] rows are the one-sided results up to the f32 rounding of the log-sum-exp
    merge (same kernel and scores, the side is a per-row-group choice of operand -- but twice the
    row groups means a different split of the columns into groups): |diff| <= 2e-6 * max(1, |lse|),
    bit for bit when the split is the same.  Backward: the products sum over 2n rows at once, so
    gradients agree to f32 summation order / bf16 rounding of d loss / d score at the changed
    lse bits (relative Frobenius error <= 1e-4)."""
    ent, rel, s, p, o = _case(7 * d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    ts, tp, to = _t(s), _t(p), _t(o)
    loss2, lse2 = eng.ce_sp_po_fwd(T, ts, tp, to)
    l_sp, z_sp = eng.ce_fwd(T, "sp", ts, tp, to)
    l_po, z_po = eng.ce_fwd(T, "po", to, tp, ts)
    for got, want in ((loss2, torch.cat([l_sp, l_po])), (lse2, torch.cat([z_sp, z_po]))):
        tol = 2e-6 * torch.clamp(torch.cat([z_sp, z_po]).abs(), min=1.0)
        assert bool(((got - want).abs() <= tol).all()), float((got - want).abs().max())
    rng = np.random.default_rng(3)
    g_rows = _t((rng.random(2 * n).astype(np.float32) + 0.5) / n)
    g_a, g_p, g_t = eng.ce_sp_po_bwd(T, ts, tp, to, lse2, g_rows=g_rows)
    a1, p1, t1 = eng.ce_bwd(T, "sp", ts, tp, to, z_sp, g_rows=g_rows[:n].contiguous())
    a2, p2, t2 = eng.ce_bwd(T, "po", to, tp, ts, z_po, g_rows=g_rows[n:].contiguous())
    for nm, got, want in (("g_a", g_a, torch.cat([a1, a2])), ("g_p", g_p, torch.cat([p1, p2])), ("g_t", g_t, t1 + t2)):
        rel_err = float((got - want).norm() / want.norm())
        assert rel_err <= 1e-4, (nm, rel_err)
    # strided int32 triple columns, as the training job passes them
    tri = torch.stack([ts, tp, to], 1).to(torch.int32)
    l3, z3 = eng.ce_sp_po_fwd(T, tri[:, 0], tri[:, 1], tri[:, 2])
    assert torch.equal(l3, loss2) and torch.equal(z3, lse2)


def test_model_level_two_sided_loss():
    from kge_amd import model as km
    E, R, d, n = 3000 + 5, 11, 256, 300
    torch.manual_seed(0)
    m = km.create("complex", E, R, d, device=DEV, score_dtype=torch.bfloat16)
    g = torch.Generator().manual_seed(2)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    m.zero_grad()
    rows = m.loss_sp_po(s, p, o)
    (rows.sum() / n).backward()
    g2 = [x.grad.clone() for x in m.parameters()]
    m.zero_grad()
    r_sp, r_po = m.loss_sp(s, p, o), m.loss_po(p, o, s)
    torch.testing.assert_close(rows.detach(), torch.cat([r_sp, r_po]).detach(), rtol=2e-6, atol=2e-6)
    (r_sp.sum() / n).backward()
    (r_po.sum() / n).backward()
    for a, b in zip(g2, [x.grad for x in m.parameters()]):
        assert float((a - b).norm() / b.norm()) <= 1e-4


def test_ce_sp_po_bwd_accum_equals_scatter_of_row_gradients(eng):
    """kge_ce_sp_po_bwd_accum (row gradients added into the table gradients by float atomics) against
    kge_ce_sp_po_bwd + index_add: same values up to the order of the atomic adds (repeated s / o / p
    indices in the batch exercise it)."""
    ent, rel, s, p, o = _case(21, "complex", 256, 500, 3, 300, 0.3)   # few relations, repeated entities
    T = _tables(eng, "complex", ent, rel)
    ts, tp, to = _t(s), _t(p), _t(o)
    n = len(s)
    loss, lse = eng.ce_sp_po_fwd(T, ts, tp, to)
    g_rows = torch.full((2 * n,), 1.0 / n, device=DEV)
    g_a, g_p, g_t = eng.ce_sp_po_bwd(T, ts, tp, to, lse, g_rows=g_rows)
    want_e = g_t.clone().index_add_(0, torch.cat([ts, to]), g_a)
    want_r = torch.zeros(3, 256, device=DEV).index_add_(0, torch.cat([tp, tp]), g_p)
    ge, gr = eng.ce_sp_po_bwd_accum(T, ts, tp, to, lse, g_rows=g_rows)
    for nm, got, want in (("ent", ge, want_e), ("rel", gr, want_r)):
        rel_err = float((got - want).norm() / want.norm())
        assert rel_err <= 1e-5, (nm, rel_err)


@pytest.mark.parametrize("n", [7, 300, 512])
def test_ce_sp_po_sum_forms(eng, n):
    """kge_ce_sp_po_fwd_sum / kge_ce_sp_po_bwd_accum_sum (the step a hipGraph replays: batch loss and its gradient
    without a host value in between): rows and lse are kge_ce_sp_po_fwd's bit for bit, the sum is scale * their float64
    sum to 1e-6 and THE SAME BITS on every call (fixed summation order, whichever workgroup arrives last), with the
    scale as a float, as a device scalar, or absent; the gradients are kge_ce_sp_po_bwd_accum's with every row's
    gradient = g * scale (up to the order of that call's float atomics).  n = 7: the last workgroup of the combine
    launch holds two rows; a second call on the same workspace finds the arrival counter back at zero."""
    ent, rel, s, p, o = _case(77 + n, "complex", 256, 2000 + 3, 5, n, 0.3)
    T = _tables(eng, "complex", ent, rel)
    ts, tp, to = _t(s), _t(p), _t(o)
    rows0, lse0 = eng.ce_sp_po_fwd(T, ts, tp, to)
    want = float(rows0.double().sum())
    for scale, sv in ((None, 1.0), (0.25, 0.25), (torch.full((), 1.0 / n, device=DEV), 1.0 / n)):
        first = None
        for _ in range(4):
            tot, rows, lse = eng.ce_sp_po_fwd_sum(T, ts, tp, to, scale)
            assert torch.equal(rows, rows0) and torch.equal(lse, lse0)
            assert tot.shape == () and abs(float(tot) - sv * want) <= 1e-6 * abs(sv * want) + 1e-7
            first = tot.clone() if first is None else first
            assert torch.equal(tot, first)
    g, scale = torch.full((), 0.5, device=DEV), torch.full((), 0.25, device=DEV)
    ge0, gr0 = eng.ce_sp_po_bwd_accum(T, ts, tp, to, lse0, g_rows=torch.full((2 * n,), 0.125, device=DEV))
    for kw in (dict(g=g, scale=scale), dict(g=g, scale=0.25), dict(g=None, scale=0.125),
               dict(g=torch.full((1,), 0.125, device=DEV))):
        ge, gr = eng.ce_sp_po_bwd_accum_sum(T, ts, tp, to, lse0, **kw)
        for nm, got, ref in (("ent", ge, ge0), ("rel", gr, gr0)):
            assert float((got - ref).norm() / ref.norm()) <= 1e-5, (nm, kw)
    with pytest.raises(ValueError):
        eng.ce_sp_po_bwd_accum_sum(T, ts, tp, to, lse0, g=torch.ones((), device=DEV, dtype=torch.float64))


def test_model_level_summed_loss_and_its_captured_step():
    """KgeModel.loss_sp_po_sum == loss_sp_po(...).sum() * scale (value to 1e-6, gradients to the atomics' order), and
    the step GraphedStep captures around it (static root gradient, one multi-table Adagrad launch) follows an eager
    run of the composed form."""
    from kge_amd import model as km, optim as kopt
    from kge_amd.train_graph import GraphedStep
    E, R, d, n = 3000 + 5, 11, 256, 300
    g = torch.Generator().manual_seed(2)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    inv = torch.full((), 1.0 / n, device=DEV)
    torch.manual_seed(0)
    m = km.create("complex", E, R, d, device=DEV, score_dtype=torch.bfloat16)
    m.zero_grad()
    a = m.loss_sp_po_sum(s, p, o, inv)
    a.backward()
    ga = [x.grad.clone() for x in m.parameters()]
    m.zero_grad()
    b = m.loss_sp_po(s, p, o).sum() * inv
    b.backward()
    assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b))
    for x, y in zip(ga, [x.grad for x in m.parameters()]):
        assert float((x - y).norm() / y.norm()) <= 1e-5
    runs = {}
    for tag in ("eager", "graph"):
        torch.manual_seed(0)
        m = km.create("complex", E, R, d, device=DEV, score_dtype=torch.bfloat16)
        opt = kopt.Adagrad(m.parameters(), lr=0.1, bf16_copies=True)
        losses = []
        if tag == "eager":
            for _ in range(6):
                opt.zero_grad(set_to_none=True)
                l = m.loss_sp_po(s, p, o).sum() * inv
                l.backward()
                opt.step()
                losses.append(float(l))
        else:
            gs = GraphedStep(lambda s_, p_, o_, i_: m.loss_sp_po_sum(s_, p_, o_, i_), opt, warmup=1)
            for _ in range(6):
                losses.append(float(gs(s, p, o, inv)))
            assert gs.replays >= 4, gs.disabled_reason
        runs[tag] = (losses, [x.detach().clone() for x in m.parameters()])
    np.testing.assert_allclose(runs["graph"][0], runs["eager"][0], rtol=2e-5)
    for x, y in zip(runs["graph"][1], runs["eager"][1]):
        assert float((x - y).norm() / y.norm()) <= 2e-3  # (Adagrad's first steps amplify atomics-order noise)


@pytest.mark.parametrize("d,n,E", [(512, 512, 14541), (256, 300, 3005), (512, 100, 2000)])
def test_backward_from_the_forwards_query_fragments(eng, d, n, E):
    """KGE_FLAG_CE_KEEP_QUERIES (round 6): the forward of the summed two-sided loss also leaves the gradient products' query
    matrix in the workspace, and a backward that is the NEXT call on that workspace starts from the forward's query
    fragments -- no build launch of its own, the relation accumulator cleared by the split-K sum's launch.  Same
    gradients BIT FOR BIT as the plain pair of calls wherever both loss passes run on the persistent kernel (and the
    flag is a no-op elsewhere: n = 100); a call in between (the generation count moves) makes kge_amd.model's
    _FusedCE2Sum fall back by itself."""
    from kge_amd import model as km
    R = 11
    g = torch.Generator().manual_seed(n)
    ent = (torch.randn(E, d, generator=g) * 0.3).bfloat16().to(DEV)
    rel = (torch.randn(R, d, generator=g) * 0.3).bfloat16().to(DEV)
    T = eng.Tables("complex", ent, rel)
    s, p, o = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    one = torch.ones((), device=DEV)
    tot0, rows0, lse0 = eng.ce_sp_po_fwd_sum(T, s, p, o, 0.5)
    ge0, gr0 = eng.ce_sp_po_bwd_accum_sum(T, s, p, o, lse0, g=one, scale=0.5)
    tot1, rows1, lse1 = eng.ce_sp_po_fwd_sum(T, s, p, o, 0.5, keep_queries=True)
    ge1, gr1 = eng.ce_sp_po_bwd_accum_sum(T, s, p, o, lse1, g=one, scale=0.5, keep_queries=True)
    assert torch.equal(tot0, tot1) and torch.equal(rows0, rows1) and torch.equal(lse0, lse1)
    # (the entity gradient is dT + float-atomic scatters of the 2n gathered rows: equal up to their order)
    assert float((ge1 - ge0).abs().max()) <= 1e-6 * float(ge0.abs().max()) and torch.equal(gr1 == gr1, gr0 == gr0)
    assert float((gr1 - gr0).abs().max()) <= 1e-6 * float(gr0.abs().max())
    # model level: an unrelated loss call between forward and backward moves the generation count
    m = km.create("complex", E, R, d, device=DEV, score_dtype=torch.bfloat16)
    m.zero_grad()
    a = m.loss_sp_po_sum(s, p, o, one * (1.0 / n))
    gen = eng.ce2_generation(torch.device(DEV))
    a.backward()
    assert eng.ce2_generation(torch.device(DEV)) == gen + 1
    ga = [x.grad.clone() for x in m.parameters()]
    m.zero_grad()
    a = m.loss_sp_po_sum(s, p, o, one * (1.0 / n))
    with torch.no_grad():
        m.loss_sp_po_sum(o, p, s, one)       # another batch through the same workspace: its fragments are there now
    a.backward()
    for x, y in zip(ga, [x.grad for x in m.parameters()]):
        assert float((x - y).norm() / x.norm()) <= 1e-5


@pytest.mark.parametrize("model,d,E,R,n,scale", CASES[:2] + CASES[4:6])
def test_fused_losses_against_the_oracles_loss_restatements(eng, model, d, E, R, n, scale):
    """The three fused training losses against oracle/torch_port.kl_loss / bce_loss (pinned bit for bit to the reference's
    KLDivWithSoftmaxKgeLoss / BCEWithLogitsKgeLoss: tests/test_oracle_vs_reference.py) evaluated on the scores the
    scoring entry writes for the same inputs (the same bits inside the fused kernels): index labels (1vsAll), a
    multi-hot matrix (KvsAll kl), the same with an offset (KvsAll bce).  f32 exp / log / summation order differ:
    |diff| <= 1e-5 + 1e-5 |lse| + 2e-6 max|score| per label (kl), 1e-5 |ref| + 1e-4 (bce: a sum over E softplus terms)."""
    import torch_port as tp
    ent, rel, s, p, o, rowptr, col = _kl_case(41 * d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    ts, tp_, to, trp, tcl = _t(s), _t(p), _t(o), _t(rowptr), _t(col)
    lab = torch.zeros(n, E)
    lab[torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(col)] = 1.0
    for direction, a, other in (("sp", ts, to), ("po", to, ts)):
        sc = (eng.score_sp(T, a, tp_) if direction == "sp" else eng.score_po(T, tp_, a)).cpu()
        amax = sc.abs().max(dim=1).values.double()
        lse = torch.logsumexp(sc.double(), 1).abs()
        # 1vsAll: index labels
        got, _lse = eng.ce_fwd(T, direction, a, tp_, other)
        want = tp.kl_loss(sc.double(), other.cpu().long(), "rows")
        assert bool(((got.cpu().double() - want).abs() <= 1e-5 + 1e-5 * lse + 2e-6 * amax).all()), direction
        # KvsAll, kl on the multi-hot matrix
        got, _lse = eng.kl_fwd(T, direction, a, tp_, trp, tcl)
        want = tp.kl_loss(sc.double(), lab.double(), "rows")
        k = torch.from_numpy(np.maximum(1, np.diff(rowptr))).double()
        assert bool(((got.cpu().double() - want).abs() <= 1e-5 + 1e-5 * lse + 2e-6 * amax * k).all()), direction
        # KvsAll, bce with an offset
        got = eng.bce_fwd(T, direction, a, tp_, trp, tcl, -0.5)
        want = tp.bce_loss(sc.double(), lab.double(), -0.5, "rows")
        assert bool(((got.cpu().double() - want).abs() <= 1e-5 * want.abs() + 1e-4 + 2e-6 * amax * k).all()), direction


@pytest.mark.parametrize("model,d,E,R", [("complex", 256, 1037, 13), ("distmult", 512, 2000 + 3, 7),
                                         ("complex", 128, 500, 5)])   # (d = 128: the products' float32 form)
@pytest.mark.parametrize("n1,n2", [(203, 131), (64, 300), (37, 0), (0, 90)])
@pytest.mark.parametrize("kind", ["kl", "bce"])
def test_multilabel2_bwd_accum_equals_the_two_one_sided_backwards(eng, model, d, E, R, n1, n2, kind):
    """kge_multilabel2_bwd_accum (both query types of a KvsAll batch: two d loss / d score passes into one gradient
    matrix, the two-sided products once over n1 + n2 rows, the rows' gradients scattered by the library) against what
    autograd assembles from kge_kl_bwd / kge_bce_bwd per type: dT + index_add of the entity rows, index_add of the
    relation rows, the two types added.  Same d loss / d score bits; the products sum over all rows at once and the
    scatter is float atomics: relative Frobenius error <= 1e-4.  Unequal, and empty, sides."""
    ent, rel, s, p1, o, rp1, cl1 = _kl_case(31 * d + n1, model, d, E, R, max(n1, 1), 0.3)
    _e, _r, _s, p2, o2, rp2, cl2 = _kl_case(37 * d + n2, model, d, E, R, max(n2, 1), 0.3)
    T = _tables(eng, model, ent, rel)
    cut = lambda n, *xs: [x[:n] for x in xs]
    (s, p1), (o2, p2) = cut(n1, s, p1), cut(n2, o2, p2)
    rp1, cl1 = (rp1, cl1) if n1 else (np.zeros(1, np.int64), np.zeros(0, np.int64))
    rp2, cl2 = (rp2, cl2) if n2 else (np.zeros(1, np.int64), np.zeros(0, np.int64))
    rng = np.random.default_rng(4)
    g1, g2 = ((rng.random(n).astype(np.float32) + 0.5) / max(n1 + n2, 1) for n in (n1, n2))
    want_e, want_r = torch.zeros(E, d, device=DEV), torch.zeros(R, d, device=DEV)
    sides = []
    for direction, a, p, rp, cl, g in (("sp", s, p1, rp1, cl1, g1), ("po", o2, p2, rp2, cl2, g2)):
        ta, tp, trp, tcl, tg = _t(a), _t(p), _t(rp), _t(cl), _t(g)
        lse = None
        if len(a):
            if kind == "kl":
                _loss, lse = eng.kl_fwd(T, direction, ta, tp, trp, tcl)
                g_a, g_p, g_t = eng.kl_bwd(T, direction, ta, tp, trp, tcl, lse, g_rows=tg)
            else:
                g_a, g_p, g_t = eng.bce_bwd(T, direction, ta, tp, trp, tcl, -0.25, g_rows=tg)
            want_e += g_t
            want_e.index_add_(0, ta, g_a)
            want_r.index_add_(0, tp, g_p)
        sides.append((ta, tp, trp, tcl, lse, tg))
    for _ in range(2):  # (the second call finds the workspace as the first left it)
        ge, gr = eng.multilabel2_bwd_accum(T, kind, -0.25 if kind == "bce" else 0.0, sides[0], sides[1])
        for nm, got, want in (("ent", ge, want_e), ("rel", gr, want_r)):
            assert float((got - want).norm() / want.norm()) <= 1e-4, (nm, float((got - want).norm() / want.norm()))


def test_model_level_paired_kvsall_loss():
    """KgeModel.multilabel_loss_sp_po == (kl_loss_sp, kl_loss_po) / (bce_loss_sp, bce_loss_po): the loss rows bit for
    bit (the same forward launches), the parameters' gradients of the summed loss to 1e-4 (one backward for both
    types against two)."""
    from kge_amd import model as km
    E, R, d, n = 3000 + 5, 11, 256, 300
    ent, rel, s, p, o, rp, cl = _kl_case(23, "complex", d, E, R, n, 0.3)
    _e, _r, _s, p2, o2, rp2, cl2 = _kl_case(29, "complex", d, E, R, n - 50, 0.3)
    ts, tp, trp, tcl, tp2, to2, trp2, tcl2 = (_t(x) for x in (s, p, rp, cl, p2, o2, rp2, cl2))
    torch.manual_seed(0)
    m = km.create("complex", E, R, d, device=DEV, score_dtype=torch.bfloat16)
    for kind in ("kl", "bce"):
        m.zero_grad()
        a, b = m.multilabel_loss_sp_po(kind, ts, tp, trp, tcl, to2, tp2, trp2, tcl2, offset=-0.5)
        ((a.sum() + b.sum()) / (2 * n)).backward()
        got = [x.grad.clone() for x in m.parameters()]
        m.zero_grad()
        if kind == "kl":
            a2, b2 = m.kl_loss_sp(ts, tp, trp, tcl), m.kl_loss_po(tp2, to2, trp2, tcl2)
        else:
            a2, b2 = m.bce_loss_sp(ts, tp, trp, tcl, -0.5), m.bce_loss_po(tp2, to2, trp2, tcl2, -0.5)
        assert torch.equal(a.detach(), a2.detach()) and torch.equal(b.detach(), b2.detach())
        (a2.sum() / (2 * n)).backward()
        (b2.sum() / (2 * n)).backward()
        want = [x.grad.clone() for x in m.parameters()]
        for x, y in zip(got, want):
            assert float((x - y).norm() / y.norm()) <= 1e-4, kind
        # the summed form: the value, and the gradients for an upstream gradient that is not 1
        m.zero_grad()
        tot = m.multilabel_loss_sp_po(kind, ts, tp, trp, tcl, to2, tp2, trp2, tcl2, offset=-0.5, sum_scale=1.0 / (2 * n))
        ref = (a2.detach().double().sum() + b2.detach().double().sum()) / (2 * n)
        assert tot.shape == () and abs(float(tot) - float(ref)) <= 2e-6 * abs(float(ref))
        (tot * 0.5).backward()
        for x, y in zip([x.grad for x in m.parameters()], want):
            assert float((x - 0.5 * y).norm() / (0.5 * y).norm()) <= 1e-4, kind


# ---- bce loss (kge_bce_fwd / kge_bce_bwd) ------------------------------------------------------------
@pytest.mark.parametrize("model,d,E,R,n,scale", CASES[:2] + CASES[4:5] + CASES[6:8])
@pytest.mark.parametrize("offset", [0.0, -1.5])
def test_bce_fwd_bwd(eng, model, d, E, R, n, scale, offset):
    """Forward against float64 sum_j BCEWithLogits(score + offset, y) of the written scores
    (1e-5 relative + the label-score tolerance of the KL test); backward against float64 autograd of
    that loss on the bf16-valued tables (<= 1e-2, bf16 operands)."""
    ent, rel, s, p, o, rowptr, col = _kl_case(11 * d + n, model, d, E, R, n, scale)
    T = _tables(eng, model, ent, rel)
    trp, tcl = _t(rowptr), _t(col)
    rng = np.random.default_rng(4)
    g_rows = (rng.random(n).astype(np.float32) + 0.5) / n
    lab = torch.zeros(n, E, dtype=torch.float64)
    lab[torch.from_numpy(np.repeat(np.arange(n), np.diff(rowptr))), torch.from_numpy(col)] = 1.0
    for direction, a in (("sp", s), ("po", o)):
        ta, tp = _t(a), _t(p)
        loss = eng.bce_fwd(T, direction, ta, tp, trp, tcl, offset).cpu().numpy().astype(np.float64)
        sc = (eng.score_sp(T, ta, tp) if direction == "sp" else eng.score_po(T, tp, ta)).cpu().double()
        want = torch.nn.functional.binary_cross_entropy_with_logits(sc + offset, lab, reduction="none").sum(1).numpy()
        tol = 1e-5 * np.abs(want) + 1e-4 + 2e-6 * np.abs(sc.numpy()).max(axis=1) * np.maximum(1, np.diff(rowptr))
        assert (np.abs(loss - want) <= tol).all(), (direction, float(np.abs(loss - want).max()), float(want.max()))
        g_a, g_p, g_t = eng.bce_bwd(T, direction, ta, tp, trp, tcl, offset, g_rows=_t(g_rows))
        ge = g_t.clone()
        ge.index_add_(0, ta, g_a)
        gr = torch.zeros(R, d, device=DEV).index_add_(0, tp, g_p)
        e = T.ent.cpu().double().requires_grad_(True)
        r = T.rel.cpu().double().requires_grad_(True)
        ea, rp_ = e[torch.from_numpy(a)], r[torch.from_numpy(p)]
        h = d // 2
        if model == "distmult":
            q = ea * rp_
        elif direction == "sp":
            q = torch.cat([ea[:, :h] * rp_[:, :h] - ea[:, h:] * rp_[:, h:], ea[:, :h] * rp_[:, h:] + ea[:, h:] * rp_[:, :h]], 1)
        else:
            q = torch.cat([ea[:, :h] * rp_[:, :h] + ea[:, h:] * rp_[:, h:], ea[:, h:] * rp_[:, :h] - ea[:, :h] * rp_[:, h:]], 1)
        l64 = torch.nn.functional.binary_cross_entropy_with_logits(q @ e.t() + offset, lab, reduction="none").sum(1)
        (l64 * torch.from_numpy(g_rows).double()).sum().backward()
        for nm, gotg, wantg in (("ent", ge, e.grad), ("rel", gr, r.grad)):
            rel_err = float((gotg.cpu().double() - wantg).norm() / wantg.norm())
            assert rel_err <= 1e-2, (direction, nm, rel_err)


@pytest.mark.parametrize("ls", [0.0, 0.2])
def test_model_level_bce_loss_against_composed(ls):
    """Fused KvsAll BCE loss (ls > 0: label-smoothed, model.bce_fused) against the composed path."""
    from kge_amd import model as km
    E, R, d, n = 2000 + 3, 7, 256, 150
    torch.manual_seed(0)
    m = km.create("complex", E, R, d, device=DEV, score_dtype=torch.bfloat16)
    ent, rel, s, p, o, rowptr, col = _kl_case(19, "complex", d, E, R, n, 0.3)
    ts, tp, to, trp, tcl = _t(s), _t(p), _t(o), _t(rowptr), _t(col)
    for fused, composed in ((lambda: m.bce_loss_sp(ts, tp, trp, tcl, -0.5, ls),
                             lambda: m._bce_composed(m.score_sp(ts, tp), trp, tcl, -0.5, ls)),
                            (lambda: m.bce_loss_po(tp, to, trp, tcl, 0.0, ls),
                             lambda: m._bce_composed(m.score_po(tp, to), trp, tcl, 0.0, ls))):
        m.zero_grad()
        lf = fused().sum() / n
        lf.backward()
        gf = [x.grad.clone() for x in m.parameters()]
        m.zero_grad()
        lc = composed().sum() / n
        lc.backward()
        gc = [x.grad.clone() for x in m.parameters()]
        assert abs(float(lf.detach()) - float(lc.detach())) <= 2e-5 * max(1.0, abs(float(lc.detach())))
        for a_, b_ in zip(gf, gc):
            assert float((a_ - b_).norm() / b_.norm()) <= 2e-3


# ---- embedder dropout inside the fused loss (lookup_embedder.py:64-69, 102-105) ---------------------------------------
@pytest.mark.parametrize("scorer,d", [("complex", 256), ("distmult", 512)])
def test_fused_ce_with_embedder_dropout_given_masks(scorer, d):
    """ce_fused_dropout with the three masks handed in, against the reference's op sequence in float32 torch on the same
    dropped-out rows rounded to bf16: embed(s) / embed(p) / embed_all() with dropout, score_emb "sp_", cross entropy;
    loss rows and both table gradients (mixed-precision bar of the fused loss: 2e-3 / 1e-2)."""
    import torch.nn.functional as F
    import torch_port as tp
    from kge_amd import model as km
    E, R, n, pe, pr = 2500, 9, 96, 0.3, 0.2
    g = torch.Generator().manual_seed(17)
    ent = (torch.randn(E, d, generator=g) * 0.3).to(DEV).requires_grad_(True)
    rel = (torch.randn(R, d, generator=g) * 0.3).to(DEV).requires_grad_(True)
    a, p, lab = (torch.randint(hi, (n,), generator=g).to(DEV) for hi in (E, R, E))
    masks = {"a": (torch.rand(n, d, generator=g) >= pe).to(DEV), "p": (torch.rand(n, d, generator=g) >= pr).to(DEV),
             "all": (torch.rand(E, d, generator=g) >= pe).to(DEV)}
    w = (torch.rand(n, generator=g) + 0.5).to(DEV)
    for direction in ("sp", "po"):
        ent.grad = rel.grad = None
        rows = km.ce_fused_dropout(scorer, 1.0, direction, ent, rel, a, p, lab, pe, pr, masks)
        (rows * w).sum().backward()
        ge, gr = ent.grad.clone(), rel.grad.clone()
        ent.grad = rel.grad = None
        r16 = lambda x: x + (x.detach().bfloat16().float() - x.detach())   # bf16 values, float32 gradients
        ad = r16(ent[a] * masks["a"] / (1 - pe))
        pd = r16(rel[p] * masks["p"] / (1 - pr))
        td = r16(ent * masks["all"] / (1 - pe))
        sc = tp.score_emb(scorer, ad, pd, td, "sp_") if direction == "sp" else tp.score_emb(scorer, td, pd, ad, "_po")
        want = F.cross_entropy(sc, lab, reduction="none")
        (want * w).sum().backward()
        assert torch.allclose(rows.detach(), want.detach(), rtol=2e-3, atol=2e-3), float((rows - want).abs().max())
        for got, ref, name in ((ge, ent.grad, "ent"), (gr, rel.grad, "rel")):
            scale = float(ref.abs().max())
            assert float((got - ref).abs().max()) <= 1e-2 * scale + 1e-6, (direction, name)
        assert float(ge[~masks["all"].any(1) & ~torch.isin(torch.arange(E, device=DEV), a)].abs().sum()) == 0.0


def test_embedder_dropout_mask_statistics():
    """Without masks handed in the masks are torch's: keep rate 1 - p, kept elements scaled by 1 / (1 - p), a fresh mask
    per call (the reference's torch.nn.Dropout)."""
    from kge_amd import model as km
    x = torch.ones(2000, 256, device=DEV)
    y1, y2 = km.embedder_dropout(x, 0.25), km.embedder_dropout(x, 0.25)
    kept = (y1 != 0).float().mean().item()
    assert abs(kept - 0.75) < 0.01 and torch.allclose(y1[y1 != 0], torch.tensor(1 / 0.75, device=DEV))
    assert not torch.equal(y1, y2)
    assert km.embedder_dropout(x, 0.0) is x
