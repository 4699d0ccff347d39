"""kge_score_so / kge_score_so_bwd_accum (score_so.hip) on the GPU.

Forward: every score has the bits kge_score_spo stores for (s[i], rels[j], o[i]) on the same tables -- the four
scorers x {float32, bf16}, l_norm 1 / 2 / 3 for TransE and RotatE, dims on the vector and the scalar chunk path, either
side of a group_size step (8 / 9 chunks), more than one chunk per lane (D > 512) and the 16-row tile of wide bf16 RotatE
rows; n and m across the 32 x 32 tile; a listed subset with a repeat, int32 and strided indexes, an output pitch with
a canary around the block; the gates.  The spo scores are taken in ONE kge_score_spo call on the n m expanded triples
(a triple's bits do not depend on its place in the batch).

Backward (float32): grad_ent / grad_rel pre-filled with random values, |got - (prefill + ref64)| <= bound elementwise
with the float64 reference and the derived bound of tests/_score_so_ref.py (its case list, checked against float64
autograd in tests/test_score_so_ref_cpu.py); rows no index names keep their bits.  No tolerance here is measured: every
case prints its largest err / bound (profiles/score_so_bound.txt is one such run)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import _score_so_ref as SO

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INVALID_ARG, UNSUPPORTED = -1, -2
NS, MS = (1, 31, 33, 70), (1, 5, 33, 70)
E = 47


def _tables(name, d, R, dtype, l_norm=1.0, seed=0):
    from kge_amd import engine
    g = torch.Generator().manual_seed(seed + d + 7 * R)
    ent = torch.randn(E, d, generator=g)
    dr = d // 2 if name == "rotate" else d
    rel = (torch.rand(R, dr, generator=g) * 2 - 1) * 3.14159 if name == "rotate" else torch.randn(R, dr, generator=g)
    return engine.Tables(name, ent.to(DEV).to(dtype), rel.to(DEV).to(dtype), l_norm=l_norm)


def _pairs(n, seed=0):
    g = torch.Generator().manual_seed(100 + n + seed)
    return torch.randint(E, (n,), generator=g).to(DEV), torch.randint(E, (n,), generator=g).to(DEV)


def _spo_block(T, s, o, rels):
    """[n, m] from one kge_score_spo call on the expanded triples"""
    from kge_amd import engine
    R = T.rel.shape[0]
    rels = torch.arange(R, device=DEV) if rels is None else rels.long()
    n, m = s.numel(), rels.numel()
    return engine.score_spo(T, s.long().repeat_interleave(m), rels.repeat(n), o.long().repeat_interleave(m)).view(n, m)


def _dims(name, dtype):
    cplx = name in ("complex", "rotate")
    step = (128, 144) if cplx else (64, 72)  # 64 / 72 reduction coordinates: 8 and 9 chunks
    return (16, 64, SO.scalar_dim(name)) + step


COMBOS = [(name, dtype, lp) for name in SO.NAMES for dtype in (torch.float32, torch.bfloat16)
          for lp in ((1.0, 2.0, 3.0) if name in ("transe", "rotate") else (1.0,))]
_cid = lambda c: f"{c[0]}-{'f32' if c[1] == torch.float32 else 'bf16'}-L{c[2]:g}"


@pytest.mark.parametrize("combo", COMBOS, ids=_cid)
def test_forward_has_the_bits_of_score_spo(combo):
    from kge_amd import engine
    name, dtype, lp = combo
    for d in _dims(name, dtype):
        for n, m in itertools.product(NS, MS):
            T = _tables(name, d, m, dtype, lp)
            s, o = _pairs(n)
            out = engine.score_so(T, s, o)
            assert out.shape == (n, m) and out.dtype == torch.float32
            want = _spo_block(T, s, o, None)
            assert torch.equal(out, want), (d, n, m, (out != want).sum().item())


@pytest.mark.parametrize("name,dtype,d,n,m", [
    ("distmult", torch.float32, 1024, 33, 5), ("transe", torch.float32, 1024, 3, 33), ("complex", torch.float32, 1024, 33, 5),
    ("rotate", torch.float32, 1024, 3, 33), ("distmult", torch.bfloat16, 2048, 3, 33), ("rotate", torch.bfloat16, 2048, 3, 33),
    ("rotate", torch.bfloat16, 1024, 3, 33), ("transe", torch.float32, 1023, 3, 5)],
    ids=lambda v: str(v).replace("torch.", ""))
def test_forward_on_wide_rows(name, dtype, d, n, m):
    """more than one chunk per lane (D > 512), the full 32-row LDS tile, and the 16-row tile of bf16 RotatE at 2048"""
    from kge_amd import engine
    for lp in ((1.0, 2.0) if name in ("transe", "rotate") else (1.0,)):
        T = _tables(name, d, m, dtype, lp)
        s, o = _pairs(n)
        assert torch.equal(engine.score_so(T, s, o), _spo_block(T, s, o, None))


@pytest.mark.parametrize("name", SO.NAMES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_subset_index_types_strides_and_output_pitch(name, dtype):
    from kge_amd import engine
    for d in (16, SO.scalar_dim(name)):
        T = _tables(name, d, 5, dtype, 2.0)
        n = 33
        s, o = _pairs(n)
        rels = torch.tensor([3, 1, 3], device=DEV)
        want = _spo_block(T, s, o, rels)
        assert torch.equal(engine.score_so(T, s, o, rels), want)
        assert torch.equal(engine.score_so(T, s.int(), o.int(), rels.int()), want)
        tri = torch.stack([s, torch.zeros_like(s), o], dim=1).contiguous()  # columns of one [n, 3] tensor: stride 3
        wide = torch.stack([rels, rels + 100], dim=1).contiguous()          # stride 2
        assert torch.equal(engine.score_so(T, tri[:, 0], tri[:, 2], wide[:, 0]), want)
        # an output pitch: ldo = m + 3, every float around the block keeps its bits
        for rl, m in ((rels, 3), (None, 5)):
            canary = torch.arange((n + 2) * (m + 3), device=DEV, dtype=torch.float32).view(n + 2, m + 3) + 0.5
            buf = canary.clone()
            engine.score_so(T, s, o, rl, out=buf[1:n + 1, 2:2 + m])
            assert torch.equal(buf[1:n + 1, 2:2 + m], _spo_block(T, s, o, rl))
            mask = torch.ones_like(buf, dtype=torch.bool)
            mask[1:n + 1, 2:2 + m] = False
            assert torch.equal(buf[mask], canary[mask])


def _raw_fwd(T, s, o, n, m, out, ldo):
    from kge_amd import _lib, engine
    keep = []
    si, oi, ri = engine._index(s, DEV, keep), engine._index(o, DEV, keep), engine._index(None, DEV, keep)
    tc = T.c()
    return _lib.lib().kge_score_so(ctypes.byref(tc), si, oi, n, ri, m, out.data_ptr(), ldo, None, 0,
                                   engine._stream_handle(DEV))


def test_gates_write_nothing():
    T = _tables("complex", 1032, 5, torch.float32)
    s, o = _pairs(4)
    out = torch.full((4, 5), 7.25, device=DEV)
    assert _raw_fwd(T, s, o, 4, 5, out, 5) == UNSUPPORTED
    T16 = _tables("complex", 16, 5, torch.float32)
    assert _raw_fwd(T16, s, o, 0, 5, out, 5) == 0          # n == 0: nothing is launched
    assert _raw_fwd(T16, s, o, 4, 4, out, 5) == INVALID_ARG  # NULL rels with m != num_rel
    torch.cuda.synchronize()
    assert bool((out == 7.25).all())
    from kge_amd import engine
    assert engine.score_so(T16, s[:0], o[:0]).shape == (0, 5)


# ---- backward -----------------------------------------------------------------------------------------------------------
RATIOS = {}


def _t(x, dtype=None):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run_bwd(k, with_scores=True):
    from kge_amd import engine
    T = engine.Tables(k["name"], _t(k["ent"]), _t(k["rel"]), l_norm=k["l_norm"])
    s, o, rels = _t(k["s"]), _t(k["o"]), _t(k["rels"])
    scores = engine.score_so(T, s, o, rels) if with_scores else None
    ge, gr = _t(k["ge0"]).clone(), _t(k["gr0"]).clone()
    ok = engine.score_so_bwd(T, s, o, rels, _t(k["gout"]), scores, ge, gr)
    torch.cuda.synchronize()
    return ok, ge.cpu().numpy(), gr.cpu().numpy()


def _case_ratio(c):
    """runs one case, asserts the bound and the untouched rows -> its largest err / bound (cached)"""
    cid = SO.case_id(c)
    if cid in RATIOS:
        return RATIOS[cid]
    k = SO.make_case(c)
    ok, ge, gr = _run_bwd(k)
    assert ok
    want = SO.bwd_accum(*SO.ref_args(k))
    bound = SO.bwd_accum_bound(*SO.ref_args(k))
    worst = 0.0
    for label, g, w, b in zip(("grad_ent", "grad_rel"), (ge, gr), want, bound):
        err = np.abs(g.astype(np.float64) - w)
        ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0)))
        print(f"score_so_bwd {cid} {label}: max err / bound = {ratio:.4f}")
        worst = max(worst, ratio)
        assert (err <= b).all(), (label, ratio, int((err > b).sum()))
    # rows no index names: the bits of their prefill
    me, mr = SO.owned_rows(k["s"], k["o"], k["rels"], k["E"], k["R"])
    assert (~me).any() and np.array_equal(ge[~me].view(np.uint32), k["ge0"][~me].view(np.uint32))
    assert np.array_equal(gr[~mr].view(np.uint32), k["gr0"][~mr].view(np.uint32))
    RATIOS[cid] = worst
    return worst


@pytest.mark.parametrize("c", SO.BWD_CASES, ids=SO.case_id)
def test_backward_inside_the_derived_bound(c):
    assert _case_ratio(c) <= 1.0


def test_backward_largest_ratio_is_at_most_one():
    """err / bound <= 1 by construction; the figure is printed for profiles/score_so_bound.txt"""
    ratios = {SO.case_id(c): _case_ratio(c) for c in SO.BWD_CASES}
    worst = max(ratios, key=ratios.get)
    print(f"score_so_bwd largest err / bound over {len(ratios)} cases: {ratios[worst]:.4f} ({worst})")
    assert ratios[worst] <= 1.0


def test_backward_gates():
    from kge_amd import _lib, engine
    # l_norm 2 without the forward scores: KGE_ERR_INVALID_ARG, gradients untouched
    k = SO.make_case(SO._c("transe", 2, 33, 5, 16, False), seed=3)
    T = engine.Tables(k["name"], _t(k["ent"]), _t(k["rel"]), l_norm=2.0)
    keep = []
    si, oi, ri = (engine._index(_t(k[x]), DEV, keep) for x in ("s", "o", "rels"))
    ge, gr, gout = _t(k["ge0"]).clone(), _t(k["gr0"]).clone(), _t(k["gout"])
    tc = T.c()
    rc = _lib.lib().kge_score_so_bwd_accum(ctypes.byref(tc), si, oi, 33, ri, 5, gout.data_ptr(), 5, None, 0, ge.data_ptr(),
                                           ge.stride(0), gr.data_ptr(), gr.stride(0), None, 0, engine._stream_handle(DEV))
    assert rc == INVALID_ARG
    # bf16 tables and dim > 1024: declined, gradients untouched
    Tb = engine.Tables("distmult", _t(k["ent"]).bfloat16(), _t(k["rel"]).bfloat16())
    assert engine.score_so_bwd(Tb, _t(k["s"]), _t(k["o"]), None, gout, None, ge, gr) is False
    Tw = _tables("distmult", 1032, 5, torch.float32)
    gew, grw = torch.full((E, 1032), 1.5, device=DEV), torch.full((5, 1032), 2.5, device=DEV)
    s, o = _pairs(33)
    assert engine.score_so_bwd(Tw, s, o, None, gout, None, gew, grw) is False
    torch.cuda.synchronize()
    assert torch.equal(ge, _t(k["ge0"])) and torch.equal(gr, _t(k["gr0"]))
    assert bool((gew == 1.5).all()) and bool((grw == 2.5).all())
    # n == 0
    assert engine.score_so_bwd(T, _t(k["s"])[:0], _t(k["o"])[:0], None, gout[:0], None, ge, gr) is True
