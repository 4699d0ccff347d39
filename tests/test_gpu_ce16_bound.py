"""The fused bf16 ComplEx / DistMult losses (kge_ce_*, kge_ce_sp_po_*, kge_kl_*, kge_kl_weighted_*, kge_bce_*) on all three
kernel generations against the float64 reference of tests/_ce16_ref.py, inside its derived bounds -- elementwise, forward
and backward, over the fixed planted cases CASES_CE (scores up to |x| >= 100, maxima that rise in every sub-unit, spikes in
the first column and in the ragged last sub-unit, exact ties, labels on the listed columns; tests/test_ce16_ref_cpu.py
asserts those properties and shows ten planted defects exceeding these bounds on these very inputs).

  tier A  independent of every kernel: lse and loss_rows against float64 of x64 = Q16 @ T^T, inside B_x + the arithmetic bound
  tier B  tight: the score bits of the store entry that runs the same single-pass chain (eng.score_sp / score_po on the same
          Tables, as tests/test_gpu_ce.py uses) lie inside x64 +- B_x; then lse / loss within the arithmetic bound ALONE of
          float64 on those bits, and g_a, g_p, g_tgt elementwise inside the interval bound ([G_lo, G_hi] from the bits and
          the float32 lse the backward was given, pushed through the float64 products).  The label scores of kl / bce come
          from kl_label_sum (float32 fma chains, not the matrix core): they are held to x64 with their own bound.
Forced routes (CE_V8 = 0 / 1, CE_V3 = 1) get the same bounds, not a kernel-to-kernel tolerance.

C_ACC = 2 and C_TR = 2 are assumptions about instructions (tests/_ce16_ref.py), not measurements: every case prints its
largest err / bound per output (profiles/ce16_bound.txt is one such run).  A ratio above 1 is a finding about a kernel or
about an assumption -- told apart by forcing the other kernel generation --, never a reason to raise a constant."""
import ctypes

import numpy as np
import pytest
import torch

import _ce16_ref as C

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PAD = 1024
NAN_BITS = 0x7FC00000

_REF = {}


def _ref(case, direction):
    """inputs and the float64 scores / score bound of one case and direction: computed once, shared, never modified"""
    key = (C.case_id(case), direction)
    if key not in _REF:
        k = C.make_case(case, direction)
        x64, bx = C.scores64(k), C.score_bound(k)
        for v in (k["ent"], k["rel"], x64, bx):
            v.setflags(write=False)
        _REF[key] = (k, x64, bx)
    return _REF[key]


def _t(x, dtype=None):
    x = torch.from_numpy(np.array(x))
    return x.to(DEV) if dtype is None else x.to(DEV, dtype)


def _np(x):
    return x.double().cpu().numpy()


def _ratio(tag, case, direction, name, got, want, bound):
    got = np.asarray(got, np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), (tag, name)
    err = np.abs(got - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    worst = float(r.max()) if r.size else 0.0
    print(f"ce16 {C.case_id(case)} {direction} {tag} {name}: max err / bound {worst:.4f}")
    return worst, (err > bound)


def _run(eng, k, T, lse32):
    """-> (bits [rows, m], lse or None, loss_rows, (g_a, g_p, g_tgt))"""
    kind, dr = k["kind"], k["direction"]
    a, p = _t(k["a"]), _t(k["p"])
    gr = None if k["g_rows"] is None else _t(k["g_rows"])
    gs = float(k["g_scalar"])
    z = _t(lse32) if lse32 is not None else None
    if kind == "ce2":
        o = _t(k["o"])
        bits = torch.cat([eng.score_sp(T, a, p), eng.score_po(T, p, o)], 0)
        loss, lse = eng.ce_sp_po_fwd(T, a, p, o)
        return bits, lse, loss, eng.ce_sp_po_bwd(T, a, p, o, z, g_rows=gr, g_scalar=gs)
    bits = eng.score_sp(T, a, p) if dr == "sp" else eng.score_po(T, p, a)
    if kind == "ce":
        lab = _t(k["label"])
        loss, lse = eng.ce_fwd(T, dr, a, p, lab)
        return bits, lse, loss, eng.ce_bwd(T, dr, a, p, lab, z, g_rows=gr, g_scalar=gs)
    rp, col = _t(k["rowptr"]), _t(k["col"])
    if kind == "kl":
        lw = None if k.get("label_weight") is None else _t(k["label_weight"])
        lb = None if k.get("label_bias") is None else _t(k["label_bias"])
        loss, lse = eng.kl_fwd(T, dr, a, p, rp, col, label_weight=lw)
        return bits, lse, loss, eng.kl_bwd(T, dr, a, p, rp, col, z, g_rows=gr, g_scalar=gs, label_weight=lw, label_bias=lb)
    loss = eng.bce_fwd(T, dr, a, p, rp, col, k["offset"])
    return bits, None, loss, eng.bce_bwd(T, dr, a, p, rp, col, k["offset"], g_rows=gr, g_scalar=gs)


def _tables(eng, k):
    ent = _t(k["ent"], torch.bfloat16)
    assert torch.equal(ent.float().cpu(), torch.from_numpy(np.array(k["ent"])))  # bf16-valued: the conversion is exact
    return eng.Tables(k["name"], ent, _t(k["rel"], torch.bfloat16))


def _loss_ref(k, x, x_label=None):
    """(float64 loss rows, arithmetic bound) from the scores x; label scores of kl / bce from x_label"""
    kind = k["kind"]
    if kind in ("ce", "ce2"):
        lab = C.labels_of(k)
        return C.ce64(x, lab)[0], C.ce_bound(x, lab)
    if kind == "kl":
        return C.kl64(x, k, x_label)[0], C.kl_bound(x, k, x_label)
    return C.bce64(x, k, x_label), C.bce_bound(x, k, x_label)


@pytest.mark.parametrize("case", C.CASES_CE, ids=C.case_id)
def test_fused_loss_within_bounds(case, kge_switch):
    from kge_amd import engine as eng
    for name, val in (case.get("switch") or {}).items():
        kge_switch.set(name, val)
    bad = []
    for direction in C.directions(case):
        k, x64, bx = _ref(case, direction)
        T = _tables(eng, k)
        lse32 = None if k["kind"] == "bce" else C.ref_lse32(k, x64)
        bits, lse, loss, grads = _run(eng, k, T, lse32)
        torch.cuda.synchronize()
        bits = _np(bits)
        checks = []
        # tier B first: the score bits themselves
        checks.append(("B", "scores", bits, x64, bx))
        bxmax = bx.max(axis=1)
        if lse is not None:
            checks.append(("A", "lse", _np(lse), C.lse64(x64), bxmax + C.lse_bound(bits)))
            checks.append(("B", "lse", _np(lse), C.lse64(bits), C.lse_bound(bits)))
        # loss rows: tier A from x64 (+ B_x of the label columns and of the lse), tier B from the bits
        wantA, arA = _loss_ref(k, x64)
        if k["kind"] in ("ce", "ce2"):
            lab = C.labels_of(k)
            bl = bx[np.arange(k["rows"]), lab]
        else:
            bl = np.array([bx[i, k["col"][k["rowptr"][i]:k["rowptr"][i + 1]]].sum() *
                           (abs(float(k["label_weight"][i])) if k.get("label_weight") is not None else
                            1.0 / max(1, k["rowptr"][i + 1] - k["rowptr"][i]) if k["kind"] == "kl" else 1.0)
                           for i in range(k["rows"])])
        lsum = bx.sum(axis=1) if k["kind"] == "bce" else bxmax  # softplus is 1-Lipschitz per column, lse in the sup norm
        _, arB = _loss_ref(k, bits, x64)
        checks.append(("A", "loss", _np(loss), wantA, lsum + bl + np.maximum(arA, arB)))
        wantB, _ = _loss_ref(k, bits, x64)
        checks.append(("B", "loss", _np(loss), wantB, arB))
        # gradients: the interval bound from the bits and the lse the backward was given
        G_lo, G_hi = C.g16_interval(k, bits.astype(np.float32), lse32)
        und = float((G_lo != G_hi).mean())
        print(f"ce16 {C.case_id(case)} {direction}: undecided share of G16 on the kernel's bits {und:.5f}")
        want, bound = C.grads_and_bound(k, G_lo, G_hi)
        for nm, g, w, b in zip(("g_a", "g_p", "g_tgt"), grads, want, bound):
            checks.append(("B", nm, _np(g), w, b))
        for tier, nm, got, w, b in checks:
            worst, over = _ratio(tier, case, direction, nm, got, w, b)
            if over.any():
                bad.append((direction, tier, nm, worst, int(over.sum()), np.argwhere(over)[:4].tolist()))
    assert not bad, (C.case_id(case), bad)


# ---- guards: every element written, nothing outside ---------------------------------------------------------------------
GUARD_CASES = [c for cid in ("ce-complex-n129-E1037-d512-ascending", "ce-distmult-n300-E1037-d512-ascending")
               for c in C.CASES_CE if C.case_id(c) == cid]


@pytest.mark.parametrize("case", GUARD_CASES, ids=C.case_id)
def test_backward_writes_every_element_and_no_margin(case):
    """One v8 case and one v4 case: kge_ce_bwd through the C ABI with g_a, g_p and g_tgt inside one NaN-filled arena, PAD
    floats of NaN in front of, between and behind them: every output element is written (finite, inside the bound), every
    margin word keeps the NaN's bits."""
    from kge_amd import _lib
    from kge_amd import engine as eng
    assert len(GUARD_CASES) == 2
    assert C.route(GUARD_CASES[0], "ds") == "v8" and C.route(GUARD_CASES[1], "ds") == "v4"
    k, x64, bx = _ref(case, "sp")
    T = _tables(eng, k)
    n, d, E = k["n"], k["d"], k["E"]
    a, p, lab = _t(k["a"]), _t(k["p"]), _t(k["label"])
    lse32 = C.ref_lse32(k, x64)
    z = _t(lse32)
    gr = None if k["g_rows"] is None else _t(k["g_rows"])
    sizes = [n * d, n * d, E * d]
    total = PAD + sum(s + PAD for s in sizes)
    arena = torch.full((total,), float("nan"), device=DEV)
    offs, off = [], PAD
    for s in sizes:
        offs.append(off)
        off += s + PAD
    ptrs = [arena.data_ptr() + 4 * o for o in offs]
    keep = []
    ai, pi, li = (eng._index(v, DEV, keep) for v in (a, p, lab))
    tc = T.c()
    st = eng._stream_handle(DEV)
    ws, wsb = eng._ce_workspace(tc, n, DEV, st)
    rc = _lib.lib().kge_ce_bwd(ctypes.byref(tc), _lib.SP_, ai, pi, li, n, z.data_ptr(), None if gr is None else gr.data_ptr(),
                               float(k["g_scalar"]), ptrs[0], ptrs[1], ptrs[2], ws, wsb, st)
    torch.cuda.synchronize()
    assert rc == 0
    outside = torch.ones(total, dtype=torch.bool, device=DEV)
    for o, s in zip(offs, sizes):
        outside[o:o + s] = False
    assert bool((arena.view(torch.int32)[outside] == NAN_BITS).all()), "a margin was written"
    bits = _np(eng.score_sp(T, a, p))
    want, bound = C.grads_and_bound(k, *C.g16_interval(k, bits.astype(np.float32), lse32))
    for nm, o, s, w, b in zip(("g_a", "g_p", "g_tgt"), offs, sizes, want, bound):
        worst, over = _ratio("guard", case, "sp", nm, _np(arena[o:o + s]), w, b)
        assert not over.any(), (nm, worst)
