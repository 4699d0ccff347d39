"""tests/_ce16_ref.py checked without a GPU: the float64 reference of the fused bf16 losses against brute-force loops and
torch float64, its interval construction against a float32 restatement of the epilogue arithmetic of both kernel forms,
the CONDITIONS under which the GPU file's bounds mean something, and ten PLANTED DEFECTS that must exceed those bounds on
the very inputs tests/test_gpu_ce16_bound.py runs.

The seeds of CASES_CE (SEED0) were tried on the CPU until the reference alone met the conditions below -- the first base
tried did; nothing here or there was ever fitted to a kernel's output.  Where the GPU file uses the kernel's score bits, this
file uses float32(x64)."""
import numpy as np
import pytest
import torch

import _ce16_ref as C
import _pairs_bwd16_ref as R16

_K = {}


def _case(case, direction):
    key = (C.case_id(case), direction)
    if key not in _K:
        k = C.make_case(case, direction)
        x64 = C.scores64(k)
        x32 = x64.astype(np.float32)
        lse32 = C.ref_lse32(k, x64)
        lo, hi = C.g16_interval(k, x32, lse32)
        want, bound = C.grads_and_bound(k, lo, hi)
        _K[key] = dict(k=k, x64=x64, x32=x32, lse32=lse32, lo=lo, hi=hi, want=want, bound=bound)
    return _K[key]


ALL = [(c, d) for c in C.CASES_CE for d in C.directions(c)]
IDS = [f"{C.case_id(c)}-{d}" for c, d in ALL]


# ---- the reference against brute force ---------------------------------------------------------------------------------
def test_scores_and_losses_against_loops_and_torch():
    c = dict(C.CASES_CE[1], n=5, E=9)
    for kind, extra in (("ce", {}), ("kl", {}), ("klw", {}), ("bce", {})):
        cc = dict(c, kind=kind)
        for direction in ("sp", "po"):
            k = C.make_case(cc, direction, seed=3)
            x = C.scores64(k)
            ent, rel = k["ent"].astype(np.float64), k["rel"].astype(np.float64)
            for i in range(k["n"]):  # DistMult: q = RNE_bf16(a r)
                q = R16.bf16_rne((k["ent"][k["a"][i]] * k["rel"][k["p"][i]]).astype(np.float32)).astype(np.float64)
                for j in range(k["E"]):
                    assert abs(x[i, j] - sum(q[t] * ent[j, t] for t in range(k["d"]))) <= 1e-12 * (1 + abs(x[i, j]))
            z = np.array([np.log(sum(np.exp(v - row.max()) for v in row)) + row.max() for row in x])
            assert np.allclose(C.lse64(x), z, rtol=1e-14, atol=0)
            assert np.allclose(C.lse64(x), torch.logsumexp(torch.from_numpy(x), 1).numpy(), rtol=1e-14, atol=0)
            if kind == "ce":
                want = torch.nn.functional.cross_entropy(torch.from_numpy(x), torch.from_numpy(k["label"]), reduction="none")
                assert np.allclose(C.ce64(x, k["label"])[0], want.numpy(), rtol=1e-12, atol=1e-12)
            elif k["kind"] == "kl":
                got = C.kl64(x, k)[0]
                for i in range(k["n"]):
                    js = k["col"][k["rowptr"][i]:k["rowptr"][i + 1]]
                    if k.get("label_weight") is not None:
                        w = z[i] - float(k["label_weight"][i]) * sum(x[i, j] for j in js)
                    elif len(js) == 0:
                        w = 0.0
                    else:  # sum_j y (log y - log softmax), y = 1 / k
                        w = sum((1 / len(js)) * (np.log(1 / len(js)) - (x[i, j] - z[i])) for j in js)
                    assert abs(got[i] - w) <= 1e-11 * (1 + abs(w))
            else:
                y = np.zeros_like(x)
                for i in range(k["n"]):
                    y[i, k["col"][k["rowptr"][i]:k["rowptr"][i + 1]]] = 1.0
                want = torch.nn.functional.binary_cross_entropy_with_logits(
                    torch.from_numpy(x + k["offset"]), torch.from_numpy(y), reduction="none").sum(1).numpy()
                assert np.allclose(C.bce64(x, k), want, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("case,direction", ALL, ids=IDS)
def test_float64_coefficients_and_products(case, direction):
    """p in float64 by an independent formula (torch autograd of the loss w.r.t. the scores) rounds into [G_lo, G_hi]; the
    products of grads_from_g16 are pairs_bwd16's on the same bf16 coefficient matrix."""
    r = _case(case, direction)
    k = r["k"]
    x = torch.from_numpy(r["x32"].astype(np.float64)).requires_grad_(True)
    g = torch.from_numpy(C.row_gradients(k)[0].astype(np.float64))
    if k["kind"] == "bce":
        loss = torch.nn.functional.softplus(x + k["offset"]).sum(1)  # the all-zero-label part: g sigmoid(x + offset)
        (loss * g).sum().backward()
        p = x.grad.numpy()
    else:  # the softmax against the GIVEN float32 lse, as the backward takes it
        z = torch.from_numpy(r["lse32"].astype(np.float64))
        p = (torch.exp(x.detach() - z[:, None]) * g[:, None]).numpy()
        if k.get("label_bias") is not None:
            p -= (C.row_gradients(k)[1].astype(np.float64))[:, None]
    if k["kind"] in ("ce", "ce2"):
        p[np.arange(k["rows"]), C.labels_of(k)] -= g.numpy()
    else:  # the label term leaves the ROUNDED coefficient, and the difference is rounded again
        y = C._sub_y(k).astype(np.float64)
        for i in range(k["rows"]):
            js = k["col"][k["rowptr"][i]:k["rowptr"][i + 1]]
            p[i, js] = R16.bf16_rne(p[i, js].astype(np.float32)).astype(np.float64) - y[i]
    G = R16.bf16_rne(p.astype(np.float32))
    assert ((G >= r["lo"]) & (G <= r["hi"])).all()
    if k["kind"] != "ce2":
        mine = C.grads_from_g16(k, G)
        theirs = R16.pairs_bwd16(k["name"], direction, k["ent"], k["rel"], k["a"], k["p"], None, G)
        for a_, b_ in zip(mine, theirs):
            assert np.allclose(a_, b_, rtol=1e-12, atol=1e-300)


# ---- the interval against the float32 restatement ------------------------------------------------------------------------
@pytest.mark.parametrize("case,direction", ALL, ids=IDS)
def test_restated_epilogues_lie_in_the_interval(case, direction):
    r = _case(case, direction)
    for form in ("v8", "v4"):
        G = C.g16_restated(r["k"], r["x32"], r["lse32"], form)
        assert ((G >= r["lo"]) & (G <= r["hi"])).all(), form
        got = C.grads_from_g16(r["k"], G)
        for g_, w, b in zip(got, r["want"], r["bound"]):
            assert (np.abs(g_ - w) <= b).all(), form
    if r["k"]["kind"] != "bce":
        z = C.lse_restated(r["x32"]).astype(np.float64)
        assert (np.abs(z - C.lse64(r["x32"])) <= C.lse_bound(r["x32"])).all()


# ---- conditions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,direction", ALL, ids=IDS)
def test_conditions(case, direction):
    r = _case(case, direction)
    k, x = r["k"], r["x64"]
    und = float((r["lo"] != r["hi"]).mean())
    free = float((r["lo"] == r["hi"]).all(axis=0).mean())
    print(f"ce16 conditions {C.case_id(case)} {direction}: undecided {und:.5f}  g_tgt rows without slack {free:.3f}")
    assert und <= 0.01
    assert free >= 0.25
    m = k["E"]
    prof = case["profile"]
    hot_rows = np.concatenate([k["hot_rows"], k["n"] + np.flatnonzero(k["o"] == k["hot"][0])]) if k["kind"] == "ce2" \
        else k["hot_rows"]
    hot_rows = hot_rows[:1] if k["kind"] == "ce2" and prof in ("ascending", "descending") else hot_rows
    xs = x[hot_rows]
    if prof in ("spike_first", "spike_last", "plateau"):
        assert (np.abs(xs).max(axis=1) >= 100).all()
        assert (xs.argmax(axis=1) // 32 == k["hot"][0] // 32).all()
        assert (xs.max(axis=1)[:, None] - np.delete(xs, k["hot"], axis=1) > 99.9).all()  # softmax below 2^-134 g
    if prof == "spike_last":
        assert k["hot"][0] == m - 1 and m % 32 != 0  # inside the ragged sub-unit
    if prof == "plateau":
        assert (k["ent"][k["hot"]] == k["ent"][k["hot"][0]]).all() and k["hot"].size >= 1
        assert np.ptp(xs[:, k["hot"]], axis=1).max() <= 1e-9
        assert (r["x32"][hot_rows][:, k["hot"]] == r["x32"][hot_rows][:, k["hot"][:1]]).all()  # exact ties
    if prof == "ascending":  # the running max rises in every 32-column sub-unit
        run = np.array([xs[:, :min(m, 32 * (s + 1))].max(axis=1) for s in range(-(-m // 32))])
        assert (np.diff(run, axis=0) > 0).all()
    if prof == "descending":
        assert (xs.argmax(axis=1) < 32).all()
    if k["kind"] in ("ce", "ce2") and k["n"] >= 16:
        listed = {j for j in C.LABEL_COLS + (m - 1, (m - 1) // 32 * 32) if j < m}
        assert listed <= set(k["label"].tolist())
        assert np.unique(k["label"]).size < k["n"]  # several rows share a label
        assert k["hot"][0] in k["label"][k["hot_rows"]] and (k["label"][k["hot_rows"]] != k["hot"][0]).any()
    if k["kind"] in ("kl", "bce"):
        cnt = np.diff(k["rowptr"])
        assert (cnt == 0).any() and (cnt == 1).any() and (cnt >= min(m, 30)).any()
        assert 0 in k["col"] and m - 1 in k["col"]
    g = C.row_gradients(k)[0]
    if k.get("g_rows") is not None and k["rows"] >= 8:
        assert (g == 0).any() and (g < 0).any() and np.abs(g[g != 0]).max() / np.abs(g[g != 0]).min() >= 2.0 ** 20
    assert sum(1 for c in C.CASES_CE if c.get("g_scalar") is not None) == 1


ROUTES = {  # case id -> (forward pass, gradient pass)
    "ce-complex-n1-E33-d128-spike_last": ("v3", "v3"), "ce-distmult-n129-E65-d128-ascending": ("v3", "v3"),
    "ce-complex-n128-E64-d256-descending": ("v4", "v4"), "ce-distmult-n300-E1037-d512-ascending": ("v4", "v4"),
    "ce-complex-n129-E1037-d512-ascending": ("v8", "v8"), "ce-distmult-n256-E2053-d256-spike_first": ("v8", "v8"),
    "ce-complex-n257-E65-d256-plateau": ("v4", "v4"), "ce-complex-n257-E65-d256-plateau-CE_V81": ("v8", "v8"),
    "ce-distmult-n256-E2053-d256-spike_first-CE_V80": ("v4", "v4"),
    "ce-complex-n129-E1037-d512-ascending-CE_V31": ("v3", "v3"),
    "ce2-distmult-n513-E33-d512-spike_last": ("v4", "v4"), "ce2-complex-n256-E1037-d256-descending": ("v8", "v8"),
    "kl-complex-n129-E1037-d256-ascending": ("v8", "v8"), "klw-distmult-n128-E65-d512-plateau": ("v4", "v4"),
    "bce-complex-n129-E1037-d256-ascending": ("v3", "v4"), "bce-distmult-n37-E65-d128-spike_first": ("v3", "v3"),
}


def test_host_rule_and_routes():
    assert [C.v8_takes(512, n, 100) for n in (1, 128, 129, 256, 257, 300, 384, 385, 513, 1024, 1025)] == \
        [False, False, True, True, False, False, False, True, False, True, True]
    assert not C.v8_takes(128, 256, 100)
    assert len(C.CASES_CE) == len(ROUTES) == 16
    for c in C.CASES_CE:
        bce = c["kind"] == "bce"
        assert (C.route(c, "splus" if bce else "lse"), C.route(c, "dsig" if bce else "ds")) == ROUTES[C.case_id(c)], C.case_id(c)
    assert {v for r in ROUTES.values() for v in r} == {"v3", "v4", "v8"}
    assert {c["d"] for c in C.CASES_CE} == {128, 256, 512} and {c["name"] for c in C.CASES_CE} == {"complex", "distmult"}
    assert {c["n"] for c in C.CASES_CE} >= {1, 128, 129, 256, 257, 300, 513}
    assert {c["E"] for c in C.CASES_CE} == {33, 64, 65, 1037, 2053}


# ---- planted defects -----------------------------------------------------------------------------------------------------
def _grad_ratio(r, G, pad_one=False):
    got = C.grads_from_g16(r["k"], G, pad_one=pad_one)
    with np.errstate(divide="ignore", invalid="ignore"):
        return max(float(np.nanmax(np.where(np.abs(g_ - w) == 0, 0.0, np.abs(g_ - w) / b)))
                   for g_, w, b in zip(got, r["want"], r["bound"]))


G_DEFECTS = {
    "label_plus4": lambda k: k["kind"] in ("ce", "ce2"),
    "label_last": lambda k: k["kind"] in ("ce", "ce2") and bool((C.labels_of(k) >= (k["E"] - 1) // 32 * 32).any()),
    "g_next": lambda k: k["rows"] >= 2 and k.get("g_rows") is not None,
    "drop_row": lambda k: k["rows"] >= 2,
    "trunc": lambda k: k["rows"] >= 2,  # (the lone hot row holds 1, -1 and zeros: nothing to truncate)
    "pad_one": lambda k: True,
    "sub_before": lambda k: k["kind"] in ("kl", "bce"),
    "no_offset": lambda k: k["kind"] == "bce",
}


@pytest.mark.parametrize("defect", sorted(G_DEFECTS))
def test_planted_gradient_defects_exceed_the_bound(defect):
    """each defect in the float32 restatement of the gradient pass, pushed through the products: outside the GPU file's
    bound in at least one element of g_a / g_p / g_tgt, on every case it applies to"""
    hit = 0
    for case, direction in ALL:
        r = _case(case, direction)
        k = r["k"]
        if not G_DEFECTS[defect](k):
            continue
        form = "v8" if C.route(case, "ds") == "v8" else "v4"
        if defect == "pad_one":
            ratio = _grad_ratio(r, C.g16_restated(k, r["x32"], r["lse32"], form), pad_one=True)
        else:
            ratio = _grad_ratio(r, C.g16_restated(k, r["x32"], r["lse32"], form, {defect: True}))
        print(f"ce16 defect {defect} {C.case_id(case)} {direction}: max err / bound {ratio:.3g}")
        assert ratio > 1.0, (defect, C.case_id(case), direction, ratio)
        hit += 1
    assert hit >= 2


@pytest.mark.parametrize("defect", ["no_rescale", "no_mask"])
def test_planted_forward_defects_exceed_the_bound(defect):
    """the rescale factor dropped when the max rises (cases whose max rises behind the first sub-unit), the ragged-tail mask
    missing (m % 32 != 0): lse outside the TIER A bound -- B_x included -- in at least one row"""
    hit = 0
    for case, direction in ALL:
        r = _case(case, direction)
        k = r["k"]
        m = k["E"]
        if k["kind"] == "bce":
            continue
        if defect == "no_rescale" and not (case["profile"] in ("ascending", "spike_last", "plateau") and m > 32):
            continue
        if defect == "no_mask" and (m % 32 == 0 or k["n"] < 2):  # (a lone hot row: pad columns at 0 lie 128 below its max)
            continue
        z = C.lse_restated(r["x32"], {defect: True}).astype(np.float64)
        bound = C.score_bound(k).max(axis=1) + C.lse_bound(r["x32"])
        ratio = float((np.abs(z - C.lse64(r["x64"])) / bound).max())
        print(f"ce16 defect {defect} {C.case_id(case)} {direction}: max err / bound {ratio:.3g}")
        assert ratio > 1.0, (defect, C.case_id(case), direction, ratio)
        hit += 1
    assert hit >= 2
