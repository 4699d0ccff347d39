"""kge_score_neg_shared / kge_score_neg_shared_bwd_accum on the GPU: scores of shared negative samples (unique ids,
drop indexes, repeat columns; kge/util/sampler.py:383-585) bit-identical to the C oracle's score_neg on the
materialised samples, nothing written outside the [n, K] block, and the table gradients of kge_amd.model's
score_neg_shared against torch autograd through the reference's op sequence on the expanded triples (float32, one
max-abs number per table, d in {33, 40, 200, 1024}: 1, 1, 2 and 8 coordinate pairs per lane of the backward kernel --
NC = 4, d = 257 .. 512, is not among them).  The backward entry itself is held elementwise to a derived bound against
float64 at every NC and at its tile and owner edges in tests/test_gpu_neg_shared_bwd.py."""
import itertools

import numpy as np
import pytest
import torch

import oracle as ko
import torch_port as tp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SCORERS = [("complex", 1.0), ("distmult", 1.0), ("transe", 1.0), ("transe", 2.0), ("rotate", 1.0), ("rotate", 2.0)]
E, R = 333, 7
_TABLES = {}


def _tables(name, d):
    """(ent, rel) float32 numpy tables, made once per (scorer, d) and never modified."""
    key = (name, d)
    if key not in _TABLES:
        rng = np.random.default_rng(1000 + d + 7 * len(name))
        ent = rng.standard_normal((E, d)).astype(np.float32)
        rel = rng.standard_normal((R, d // 2 if name == "rotate" else d)).astype(np.float32)
        _TABLES[key] = (ent, rel)
    return _TABLES[key]


def _shared_case(rng, n, uc, kind, slot, spo, nrep, pattern):
    """(unique, drop or None, repeat) as the sampler would hand them over; `pattern` = the drop rule's case."""
    p_unique = uc + (1 if kind == "default" else 0)
    unique = rng.permutation(E)[:p_unique].astype(np.int64)
    drop = None
    if kind == "default":
        if pattern == 0:      # no row uses the spare
            drop = np.full(n, uc, dtype=np.int64)
        elif pattern == 1:    # every row drops the same column
            drop = np.full(n, uc - 1, dtype=np.int64)
        elif pattern == 2:    # mixed, the "no spare" value included
            drop = rng.integers(0, uc + 1, n).astype(np.int64)
        else:                 # rows whose own positive is in the unique list drop it (sampler.py:677-686)
            own = spo[slot]
            mine = rng.permutation(np.unique(own))[:uc]
            others = rng.permutation(np.setdiff1d(np.arange(E), mine))[:p_unique - len(mine)]
            unique = np.concatenate([mine, others]).astype(np.int64)
            drop = rng.integers(0, uc + 1, n).astype(np.int64)
            where = {int(e): j for j, e in enumerate(unique[:uc])}
            for i in range(n):
                if int(own[i]) in where:
                    drop[i] = where[int(own[i])]
    repeat = rng.integers(0, uc, nrep).astype(np.int64) if nrep else None
    if nrep >= 2:
        repeat[1] = repeat[0]  # a duplicate among the repeats
    return unique, drop, repeat


def _check_forward(T, O, rng, n, uc, kind, slot, nrep, pattern, idt, strided):
    from kge_amd import engine
    tri = np.stack([rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)], 1).astype(np.int64)
    unique, drop, repeat = _shared_case(rng, n, uc, kind, slot, (tri[:, 0], tri[:, 1], tri[:, 2]), nrep, pattern)
    K = uc + nrep
    tu = torch.from_numpy(unique)
    td = None if drop is None else torch.from_numpy(drop)
    tr = torch.empty(0) if repeat is None else torch.from_numpy(repeat)  # (none: the sampler's empty FLOAT tensor)
    neg = engine.shared_samples(tu, td, tr, n).contiguous().numpy()
    assert neg.shape == (n, K)
    want = ko.score_neg(O, tri[:, 0], tri[:, 1], tri[:, 2], slot, neg)
    if strided:  # s / p / o as the stride-3 columns of one [n, 3] tensor
        tt = torch.from_numpy(tri).to(DEV).to(idt)
        s, p, o = tt[:, 0], tt[:, 1], tt[:, 2]
    else:
        s, p, o = (torch.from_numpy(tri[:, k].copy()).to(DEV).to(idt) for k in range(3))
    buf = torch.full((n + 2, K + 5), float("nan"), device=DEV)
    out = buf[1:n + 1, 2:2 + K]
    engine.score_neg_shared(T, s, p, o, slot, tu.to(DEV).to(idt), None if td is None else td.to(DEV),
                            tr.to(DEV), flags=engine.FLAG_EXACT, out=out)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    what = (n, uc, kind, slot, nrep, pattern, str(idt), strided)
    assert np.array_equal(got[1:n + 1, 2:2 + K], want), what
    got[1:n + 1, 2:2 + K] = np.nan
    assert np.isnan(got).all(), ("written outside the [n, K] block", what)


@pytest.mark.parametrize("name,l_norm", SCORERS)
def test_forward_is_bit_identical_to_score_neg_on_the_materialised_samples(name, l_norm):
    from kge_amd import engine
    from kge_amd.engine import NEG_SHARED_TILE_COLUMNS as TU, NEG_SHARED_TILE_POSITIVES as TN
    rng = np.random.default_rng(5)
    count = itertools.count()
    dims = [64, 100, 1024] + ([66] if name == "rotate" else [])
    for d in dims:
        ent, rel = _tables(name, d)
        T = engine.Tables(name, torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV), l_norm)
        O = ko.Tables(name, ent, rel, l_norm)
        shapes = list(itertools.product((1, 70), (1, 37)))
        if d == 64:  # the tile edges: positives per workgroup, staged columns (+ the spare) per workgroup
            shapes += list(itertools.product((TN - 1, TN, TN + 1), (TU - 2, TU - 1, TU)))
        for (n, uc), slot, kind, nrep in itertools.product(shapes, (0, 2), ("naive", "default"), (0, 11)):
            c = next(count)
            _check_forward(T, O, rng, n, uc, kind, slot, nrep, pattern=c % 4, idt=(torch.int64, torch.int32)[(c // 4) % 2],
                           strided=bool((c // 8) % 2))
    # every drop pattern at one multi-tile shape, whatever the enumeration above gave it
    ent, rel = _tables(name, 64)
    T = engine.Tables(name, torch.from_numpy(ent).to(DEV), torch.from_numpy(rel).to(DEV), l_norm)
    O = ko.Tables(name, ent, rel, l_norm)
    for pattern, slot in itertools.product(range(4), (0, 2)):
        _check_forward(T, O, rng, 70, 37, "default", slot, 11, pattern, torch.int64, False)
    # bf16 tables
    bent, brel = ko.f32_to_bf16(ent), ko.f32_to_bf16(rel)
    Tb = engine.Tables(name, torch.from_numpy(ent).to(DEV).bfloat16(), torch.from_numpy(rel).to(DEV).bfloat16(), l_norm)
    Ob = ko.Tables(name, bent, brel, l_norm)
    _check_forward(Tb, Ob, rng, 70, 37, "default", 0, 11, 2, torch.int64, False)
    _check_forward(Tb, Ob, rng, 33, 37, "naive", 2, 0, 0, torch.int32, True)


def test_rows_too_wide_for_the_tile_are_declined():
    """float32 d = 2048: the kernel answers UNSUPPORTED, engine.neg_shared_supported says so beforehand, and the model's
    score_neg_shared goes the per-triple way on the materialised samples instead (same scores, gradients flow)."""
    from kge_amd import engine
    ent = torch.zeros(8, 2048, device=DEV)
    T = engine.Tables("distmult", ent, torch.zeros(2, 2048, device=DEV))
    ix = torch.zeros(3, dtype=torch.long, device=DEV)
    assert not engine.neg_shared_supported(torch.float32, 2048, 3) and engine.neg_shared_supported(torch.float32, 1024, 3)
    with pytest.raises(RuntimeError, match="kge_status -2"):
        engine.score_neg_shared(T, ix, ix, ix, 2, torch.arange(4, device=DEV))
    m = _model("distmult", 8, 2, 2048, 1.0).train()
    s, p, o = (torch.tensor(x, device=DEV) for x in ([1, 2, 3], [0, 1, 0], [4, 5, 6]))
    unique, drop, repeat = torch.tensor([7, 0, 2, 5], device=DEV), torch.tensor([3, 0, 1], device=DEV), torch.tensor([1, 1], device=DEV)
    got = m.score_neg_shared(s, p, o, 2, unique, drop, repeat)
    want = m.score_neg(s, p, o, 2, engine.shared_samples(unique, drop, repeat, 3).contiguous())
    assert got.shape == (3, 5) and torch.equal(got, want)
    got.sum().backward()
    assert m.get_s_embedder().weight.grad is not None


def _model(name, n_ent, n_rel, d, l_norm):
    from kge_amd import model
    torch.manual_seed(0)
    return model.create(name, n_ent, n_rel, d, l_norm=l_norm, device=DEV)


def _check_gradients(name, l_norm, d, n, uc, nrep, n_ent=60, n_rel=4):
    """Random linear functional of model.score_neg_shared: both table gradients against torch autograd through
    torch_port.score_spo on the expanded materialised triples; error <= 2e-4 max(1, |want|max)."""
    from kge_amd import engine
    m = _model(name, n_ent, n_rel, d, l_norm).train()
    # (model.create's random tables: no two rows coincide, RotatE / TransE distances stay away from exact zero)
    ent0 = m.get_s_embedder().weight.detach().cpu().clone()
    rel0 = m.get_p_embedder().weight.detach().cpu().clone()
    g = torch.Generator().manual_seed(4)
    s, p, o = (torch.randint(hi, (n,), generator=g) for hi in (n_ent, n_rel, n_ent))
    for slot, kind in itertools.product((0, 2), ("naive", "default")):
        phys = uc + (1 if kind == "default" else 0)
        # (more ids than entities at uc = 70, E = 60: the list repeats some -- the kernels take any list)
        unique = torch.cat([torch.randperm(n_ent, generator=g) for _ in range(phys // n_ent + 1)])[:phys]
        drop = torch.randint(uc + 1, (n,), generator=g) if kind == "default" else None
        repeat = torch.randint(uc, (nrep,), generator=g) if nrep else torch.empty(0)
        K = uc + nrep
        neg = engine.shared_samples(unique, drop, repeat, n)
        w = torch.randn(n, K, generator=g)
        ent, rel = ent0.clone().requires_grad_(), rel0.clone().requires_grad_()
        tr = [x.repeat_interleave(K) for x in (s, p, o)]
        tr[slot] = neg.reshape(-1)
        ref = tp.score_spo(name, ent, rel, tr[0], tr[1], tr[2], l_norm).view(n, K)
        (ref * w).sum().backward()
        m.zero_grad()
        got = m.score_neg_shared(s.to(DEV), p.to(DEV), o.to(DEV), slot, unique.to(DEV),
                                 None if drop is None else drop.to(DEV), repeat.to(DEV))
        assert got.shape == (n, K)
        (got * w.to(DEV)).sum().backward()
        for gv, want, nm in ((m.get_s_embedder().weight.grad.cpu(), ent.grad, "entity"),
                             (m.get_p_embedder().weight.grad.cpu(), rel.grad, "relation")):
            scale = max(1.0, float(want.abs().max()))
            err = float((gv - want).abs().max())
            print(f"score_neg_shared gradient {name} l{l_norm} d={d} n={n} uc={uc} slot={slot} {kind} {nm}: "
                  f"err {err:.3e} scale {scale:.3e}")
            assert err <= 2e-4 * scale, (name, l_norm, d, slot, kind, nm, err, scale)


@pytest.mark.parametrize("name,l_norm", SCORERS)
@pytest.mark.parametrize("d", [40, 33])
def test_gradients_match_torch_autograd(name, l_norm, d):
    if name in ("complex", "rotate") and d % 2:
        pytest.skip("even dimensionality only")
    _check_gradients(name, l_norm, d, n=19, uc=70, nrep=9)


@pytest.mark.parametrize("name,l_norm", SCORERS)
@pytest.mark.parametrize("d", [200, 1024])
def test_gradients_with_several_coordinate_pairs_per_lane(name, l_norm, d):
    """d = 200 and d = 1024: two and eight coordinate pairs per lane in the backward kernel (NC; its tiles are 64 / NC
    physical rows and 32 / NC positives: 32 and 16 at d = 200, 8 and 4 at d = 1024), past one tile of either with n = 19
    positives and 70 (+ 1) rows."""
    _check_gradients(name, l_norm, d, n=19, uc=70, nrep=9)


@pytest.mark.parametrize("name,l_norm", SCORERS)
def test_gradients_with_long_sums_per_target(name, l_norm):
    _check_gradients(name, l_norm, 40, n=300, uc=5, nrep=0)


@pytest.mark.parametrize("name,l_norm", [("complex", 1.0), ("transe", 2.0), ("rotate", 1.0)])
def test_gradients_through_the_fallback(name, l_norm, monkeypatch):
    """The accumulate kernel declining (forced): the backward goes through score_neg_bwd_accum on the materialised
    samples and meets the same bar."""
    from kge_amd import engine
    calls = []

    def declined(*a, **k):
        calls.append(1)
        return False

    monkeypatch.setattr(engine, "score_neg_shared_bwd_accum", declined)
    _check_gradients(name, l_norm, 40, n=19, uc=70, nrep=9)
    assert len(calls) == 4
