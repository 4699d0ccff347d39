"""kge_conve_queries (csrc/conve.hip) through the C ABI on the GPU: the augmented query rows and the scores contracted from
them within the derived bound of tests/_conve_ref.py, NaN-filled guards around q, an exactly sized NaN-filled workspace,
and the equalities the canonical arithmetic promises, bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import _conve_ref as cr

pytestmark = pytest.mark.gpu

TM = 32  # CV_TM: the row tile of conve_partial_kernel


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


_REFS = {}
WORST = {"q": 0.0, "score": 0.0}


def _ref(name):
    """the case, its float64 query rows and scores: computed once"""
    if name not in _REFS:
        net, ent, rel, s, p, o = cr.gpu_case(name)
        _REFS[name] = (net, ent, rel, s, p, o, cr.queries(net, ent, rel, s, p), cr.score_sp(net, ent, rel, s, p),
                       cr.score_spo(net, ent, rel, s, p, o))
    return _REFS[name]


def _pitched(x, ld, dev, misalign=False):
    r, c = x.shape
    buf = torch.full((r * ld + 4,), float("nan"), device=dev)
    v = buf[1:1 + r * ld] if misalign else buf[:r * ld]
    v = v.view(r, ld)[:, :c]
    v.copy_(x if torch.is_tensor(x) else torch.from_numpy(x))
    return v


class Dev:
    """a network and its tables on the device, and the ctypes call"""

    def __init__(self, net, ent, rel, dev, proj_ld=None, ent_ld=None, rel_ld=None, misalign=False):
        from kge_amd import _lib
        self.dev, self.net = dev, net
        self.d = net["h"] * net["w"]
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        self.t = {k: t(net[k]) for k in ("conv_w", "conv_b", "mean1", "var1", "proj_b", "mean2", "var2")}
        F = net["proj_w"].shape[1]
        self.proj = t(net["proj_w"]) if proj_ld is None else _pitched(net["proj_w"], proj_ld, dev, misalign)
        self.ent = t(ent) if ent_ld is None else _pitched(ent, ent_ld, dev, misalign)
        self.rel = t(rel) if rel_ld is None else _pitched(rel, rel_ld, dev, misalign)
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self.c = _lib.KgeConveNet(net["h"], net["w"], net["fs"], net["pad"], 0 if net["conv_b"] is None else 1, 0,
                                  ptr(self.t["conv_w"]), ptr(self.t["conv_b"]), ptr(self.t["mean1"]),
                                  ptr(self.t["var1"]), self.proj.data_ptr(), self.proj.stride(0) if self.d > 1 else F,
                                  ptr(self.t["proj_b"]), ptr(self.t["mean2"]), ptr(self.t["var2"]), net["eps1"],
                                  net["eps2"])

    def index(self, x, dtype=torch.int64, stride=1):
        from kge_amd import _lib
        x = torch.as_tensor(np.asarray(x), device=self.dev).to(dtype)
        if stride > 1:
            buf = torch.full((stride * x.numel(),), -1, dtype=dtype, device=self.dev)
            buf[::stride] = x
            x = buf
        return x, _lib.KgeIndex(x.data_ptr(), _lib.I32 if dtype == torch.int32 else _lib.I64, 0, stride)

    def run(self, s, p, dtype=torch.int64, stride=1, q_ld=None, misalign=False):
        """q [n, d + 1] from a NaN-filled pitched buffer with NaN guards and an exactly sized NaN-filled workspace"""
        from kge_amd import _lib
        L = _lib.lib()
        n, w = len(s), self.d + 1
        ld = w if q_ld is None else q_ld
        guard = 8
        off = guard + (1 if misalign else 0)
        buf = torch.full((off + n * ld + guard,), float("nan"), device=self.dev)
        need = L.kge_conve_workspace_bytes(ctypes.byref(self.c), n)
        assert need == 32 * n * self.d * 4
        ws = torch.full((need // 4,), float("nan"), device=self.dev)
        ks, si = self.index(s, dtype, stride)
        kp, pi = self.index(p, dtype, stride)
        rc = L.kge_conve_queries(ctypes.byref(self.c), self.ent.data_ptr(), self.ent.stride(0), self.rel.data_ptr(),
                                 self.rel.stride(0), si, pi, n, buf[off:].data_ptr(), ld, ws.data_ptr(), need,
                                 ctypes.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize(self.dev)
        body = buf[off:off + n * ld].view(n, ld)
        assert bool(torch.isnan(buf[:off]).all()) and bool(torch.isnan(buf[off + n * ld:]).all()), "the guards around q"
        if ld > w:
            assert bool(torch.isnan(body[:, w:]).all()), "nothing written between the rows of q"
        assert not bool(torch.isnan(ws).any()), "every float of the workspace is written"
        return body[:, :w].clone()


def _within(got, ref, what, key):
    want, e = ref
    got = got.double().cpu().numpy().reshape(want.shape)
    err = np.abs(got - want)
    tol = cr.bound(e)
    ratio = float((err / tol).max())
    WORST[key] = max(WORST[key], ratio)
    print("{}: max err / bound = {:.4f}".format(what, ratio))
    bad = err > tol
    assert not bad.any(), "{}: {} of {} outside the bound (worst {:.3e} at a bound of {:.3e})".format(
        what, int(bad.sum()), bad.size, float(err[bad].max()), float(tol[bad][err[bad].argmax()]))


@pytest.mark.parametrize("name", list(cr.GPU_CASES))
def test_queries_and_scores_within_bound(dev, name):
    from kge_amd import engine
    net, ent, rel, s, p, o, qref, spref, sporef = _ref(name)
    D = Dev(net, ent, rel, dev)
    q = D.run(s, p)
    assert bool((q[:, 0] == 1.0).all()), "q[:, 0] == 1"
    assert bool((q[:, 1:] >= 0).all())
    dead = float((q[:, 1:] == 0).float().mean())
    assert 0.05 < dead < 0.95, "outputs die and survive at the second ReLU"
    _within(q, qref, name + " q'", "q")
    assert torch.equal(q[0], q[-1]), "the same (s, p) pair at two positions"
    # the contraction: kge_score_emb(DistMult, SP_ / SPO, q', ones, entity rows)
    ones = torch.ones_like(q)
    _within(engine.score_emb("distmult", q, ones, D.ent, "sp_"), spref, name + " sp_", "score")
    _within(engine.score_emb("distmult", q, ones, D.ent[torch.from_numpy(o).to(dev)].contiguous(), "spo"), sporef,
            name + " spo", "score")


@pytest.mark.parametrize("name", ["seam", "odd_d"])
def test_row_counts_at_the_tile_edges_and_past_one_wave(dev, name):
    """n = 1, the row tile - 1 / 0 / + 1, two tiles + 1, and just past one full wave of workgroups (256 CUs x 8
    workgroups = 64 row tiles of 32 channels each): a row's bits never depend on n or on its position"""
    net, ent, rel, s, p, o, qref, _, _ = _ref(name)
    D = Dev(net, ent, rel, dev)
    big = 64 * TM + 1
    rng = np.random.default_rng(5)
    S, P = rng.integers(0, cr.GPU_E, big), rng.integers(0, cr.GPU_R, big)
    S[:len(s)], P[:len(p)] = s, p
    full = D.run(S, P)
    _within(full[:len(s)], qref, name + " rows of the large call", "q")
    # every (s, p) pair has one row image, wherever it stands
    first = {}
    for i, key in enumerate(zip(S.tolist(), P.tolist())):
        first.setdefault(key, i)
    rep = torch.tensor([first[k] for k in zip(S.tolist(), P.tolist())], device=dev)
    assert torch.equal(full, full[rep]), "equal pairs, equal bits, at every position"
    for n in (1, TM - 1, TM, TM + 1, 2 * TM + 1):
        assert torch.equal(D.run(S[:n], P[:n]), full[:n]), n
        assert torch.equal(D.run(S[-n:], P[-n:]), full[-n:]), (n, "from the end")


@pytest.mark.parametrize("name", ["odd_d", "default", "fs5_pad2"])
def test_bit_equalities_across_forms(dev, name):
    net, ent, rel, s, p, o, _, _, _ = _ref(name)
    d, F = net["h"] * net["w"], net["proj_w"].shape[1]
    want = Dev(net, ent, rel, dev).run(s, p)
    D = Dev(net, ent, rel, dev)
    assert torch.equal(D.run(s, p), want), "two runs"
    assert torch.equal(D.run(s, p, torch.int32), want), "int32 indices"
    assert torch.equal(D.run(s, p, torch.int64, 3), want) and torch.equal(D.run(s, p, torch.int32, 2), want), "strided"
    assert torch.equal(D.run(s, p, q_ld=d + 8), want), "pitched q"
    assert torch.equal(D.run(s, p, q_ld=d + 4, misalign=True), want), "pitched q off the 16-byte grid"
    for kw in (dict(ent_ld=d + 6), dict(rel_ld=d + 2), dict(proj_ld=F + 4), dict(proj_ld=F + 3, misalign=True),
               dict(ent_ld=d + 4, rel_ld=d + 9, proj_ld=F + 1, misalign=True)):
        assert torch.equal(Dev(net, ent, rel, dev, **kw).run(s, p), want), kw
    # the range form: rows start .. start + n - 1 of both tables
    from kge_amd import _lib
    L = _lib.lib()
    n = 5
    q = torch.full((n, d + 1), float("nan"), device=dev)
    need = L.kge_conve_workspace_bytes(ctypes.byref(D.c), n)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = L.kge_conve_queries(ctypes.byref(D.c), D.ent.data_ptr(), d + 1, D.rel.data_ptr(), d + 1,
                             _lib.KgeIndex(None, _lib.I64, 2, 1), _lib.KgeIndex(None, _lib.I64, 1, 1), n, q.data_ptr(),
                             d + 1, ws.data_ptr(), need, None)
    assert rc == 0
    torch.cuda.synchronize(dev)
    assert torch.equal(q, D.run(np.arange(2, 2 + n), np.arange(1, 1 + n))), "range form"


def test_engine_front_end_and_worst_ratio(dev):
    """engine.conve_queries gives the bits of the C call; the largest err / bound of this file goes to stdout (the figure
    of profiles/conve_bound.txt)"""
    from kge_amd import engine
    net, ent, rel, s, p, o, qref, _, _ = _ref("pad1")
    D = Dev(net, ent, rel, dev)
    en = engine.ConveNet(net["h"], net["w"], net["fs"], net["pad"], D.t["conv_w"].view(32, 1, net["fs"], net["fs"]),
                         D.t["conv_b"], D.t["mean1"], D.t["var1"], net["eps1"], D.proj, D.t["proj_b"], D.t["mean2"],
                         D.t["var2"], net["eps2"])
    st, pt = torch.from_numpy(s).to(dev), torch.from_numpy(p).to(dev)
    q = engine.conve_queries(en, D.ent, D.rel, st, pt)
    assert torch.equal(q, D.run(s, p))
    out = torch.zeros(len(s), 24, device=dev)
    engine.conve_queries(en, D.ent, D.rel, st, pt, out=out)
    assert torch.equal(out[:, :16], q) and not bool(out[:, 16:].any())
    assert engine.conve_queries(en, D.ent, D.rel, st[:0], pt[:0]).shape == (0, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.conve_queries(en, D.ent.cpu(), D.rel, st, pt)
    print("conve_bound: largest err / bound so far: q' {:.4f}, scores {:.4f}".format(WORST["q"], WORST["score"]))


def test_a_slice_near_the_largest_the_gate_takes(dev):
    """h = 14, w = 36, fs = 1: Ho * Wo = 1008 positions, 1009 floats a row of the slice (the gate's limit is 1024):
    129 KB of dynamic LDS, d = 504 crosses two column passes of 256 outputs"""
    net = cr.make_net(14, 36, 1, 0, True, seed=3)
    ent, rel = cr.make_tables(9, 4, 504, 21)
    s, p = np.array([0, 8, 3, 3, 0]), np.array([1, 0, 3, 3, 1])
    D = Dev(net, ent, rel, dev)
    q = D.run(s, p)
    _within(q, cr.queries(net, ent, rel, s, p), "slice of 1009 floats q'", "q")
    assert torch.equal(q[0], q[4]) and torch.equal(q[2], q[3]) and bool((q[:, 0] == 1).all())
