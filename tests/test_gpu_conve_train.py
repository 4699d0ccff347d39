"""kge_conve_train_fwd / kge_conve_train_bwd (csrc/conve_train.hip) against float64 torch autograd of the same graph with
the masks supplied from the numpy Philox of tests/_dropout_ref.py (roles 3 / 4 of include/kge_amd.h).

The bound is the arithmetic of tests/_conve_train_ref.py (its _bn / _bn_abs, U, FLOOR, the absolute graph, the charge for
ReLU units inside their forward bound: gamma_K A(M + U) + (A(M + U) - A(M - U))) restated for the network alone with the
two masks as positive scales, with two changes that only make it ask more:
  * K counts the roundings of conve_train.hip's own summation trees (`roundings`), not those of an arbitrary order: that
    module's count charges 2 n Ho Wo for bn1 alone, gamma = 3e-3 at the largest case, under which most units count as
    unstable and the bound exceeds every gradient;
  * the upstream gradient g_x is set to 0 at the second-layer units inside their forward bound (`reference`; the device
    gets the same g_x), so no path is charged through them; first-layer units inside theirs are charged as in the module.
Forward values and means: gamma_{K_fwd} x the absolute graph's value (ReLU is 1-Lipschitz); variances: first order,
d var = mean(2 (x - mu)(dx - dmu)) with |dx| <= gamma_{K_fwd} xA, plus gamma_{K_fwd} var for the reduction.
The ReLU-stability condition (`informative`, asserted for every case on the CPU and the GPU): below 0.1 % of the first
layer's and 10 % of the second layer's units inside their forward bound (these carry g_x = 0), and the bound below more than 30 % of the elements
of every gradient that is not identically 0 (`shows` says which are, and why).  The planted defects are checked on the
CPU at every shape."""
import ctypes

import numpy as np
import pytest
import torch

import _conve_train_ref as tr
import _dropout_ref as dr

SEED, CALL, EPS = 0x1234_5678_9ABC_DEF0, 5, 1e-5
GRADS = ("s_emb", "p_emb", "conv_w", "conv_b", "proj_w", "proj_b")
WORST = {}
SHAPES = [(2, 4, 1, 0), (4, 8, 3, 0), (4, 8, 3, 1), (4, 8, 5, 2), (10, 20, 3, 0)]


def make(h, w, fs, pad, n, bias, ps, seed=0):
    rng = np.random.default_rng(1000 * h + 10 * fs + pad + n + seed)
    d, F = h * w, 32 * (2 * h - fs + 2 * pad + 1) * (w - fs + 2 * pad + 1)
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    P = dict(s_emb=f32(n, d + 1), p_emb=f32(n, d + 1), conv_w=f32(32, 1, fs, fs) * 0.5,
             conv_b=f32(32) * 0.5 if bias else None, proj_w=f32(d, F) / np.float32(np.sqrt(F)), proj_b=f32(d) * 0.5)
    return dict(P=P, h=h, w=w, fs=fs, pad=pad, n=n, d=d, F=F, gx=f32(n, d), ps=ps,
                f=dr.factor(n, 32, 0, CALL, 3, SEED, ps[0]), m=dr.factor(n, d, 0, CALL, 4, SEED, ps[1]))


def roundings(n, d, HW, fs):
    """(K_fwd, K): the roundings on the longest path of conve_train.hip's OWN summation trees (a bound for this order, far
    below the any-order count of tests/_conve_train_ref.py, which charges 2 n Ho Wo for bn1 alone)"""
    up = lambda a, b: -(-a // b)  # noqa: E731
    t32, t8 = up(n, 32), up(n, 8)
    s1 = 2 * (8 * up(HW, 64) + 9 + 6 * t32 + 4)  # bn1: a thread's 8 rows x its positions, butterfly + 3 waves, Chan's merge
    s2 = 2 * (up(n, 4) + 3 + 2)                  # bn2 / its backward: a row phase, the 4 phases, the division
    kf = fs * fs + 1 + s1 + 5 + 1 + (HW + 8 + 32 + 1) + 1 + s2 + 5
    sf = 2 * (8 * t32 + 9 + up(HW, 64) + 2)      # the channel's two sums of the feature backward
    kb = s2 + 7 + (d + 10) + 2 + sf + 5 + 32 * (fs * fs + 1) + (up(HW, 32) + 9 + t8) + 32 * t32 + up(n, 4) + 3
    return kf, kf + kb


def reference(c, f=None, m=None, gx=None):
    """{output: (float64 value, bound)} of the case; f / m / gx replace the case's masks and upstream gradient"""
    P, h, w, pad, n, d, fs = c["P"], c["h"], c["w"], c["pad"], c["n"], c["d"], c["fs"]
    t64 = lambda a: torch.as_tensor(np.asarray(a, np.float64))  # noqa: E731
    f, m, G = t64(c["f"] if f is None else f), t64(c["m"] if m is None else m), t64(c["gx"] if gx is None else gx)

    def leaves(ab):
        return {k: (t64(v).abs() if ab else t64(v)).requires_grad_() for k, v in P.items() if v is not None}

    def images(L):
        return torch.cat([L["s_emb"][:, 1:].reshape(n, 1, h, w), L["p_emb"][:, 1:].reshape(n, 1, h, w)], 2)

    def forward(L, ab=None):
        v = torch.nn.functional.conv2d(images(L), L["conv_w"], L.get("conv_b"), padding=pad)
        if ab is None:
            z, r = tr._bn(v, (0, 2, 3), EPS)
            y = ((torch.relu(z) * f[:, :, None, None]).reshape(n, -1) @ L["proj_w"].t() + L["proj_b"]) * m
            return (v, z, r, y) + tr._bn(y, (0,), EPS)
        z1A = tr._bn_abs(v, (0, 2, 3), r1, h1)
        yA = ((z1A * ab * f[:, :, None, None]).reshape(n, -1) @ L["proj_w"].t() + L["proj_b"]) * m
        return v, z1A, yA, tr._bn_abs(yA, (0,), r2, h2)

    L = leaves(False)
    v, z1, r1, y, z2, r2 = forward(L)
    r1, r2, h1, h2 = r1.detach(), r2.detach(), z1.detach().abs(), z2.detach().abs()
    HW, F = v.shape[2] * v.shape[3], c["F"]
    gam_f, gam = (k * tr.U / (1 - k * tr.U) for k in roundings(n, d, HW, fs))
    on1, on2 = (z1.detach() > 0).double(), (z2.detach() > 0).double()
    with torch.no_grad():
        _, z1A, _, z2A = forward(leaves(True), on1)
    u1, u2 = (h1 <= gam_f * z1A).double(), (h2 <= gam_f * z2A).double()
    G = G * (1 - u2)  # no gradient enters at a second-layer unit inside its forward bound (the docstring)
    if gx is None:
        c["gx"] = G.numpy().astype(np.float32)
    (torch.relu(z2) * G).sum().backward()

    def absolute(m1):
        A = leaves(True)
        vA, _, yA, z2A = forward(A, m1)
        (z2A * on2 * G.abs()).sum().backward()
        return {k: A[k].grad.numpy() for k in A}, vA.detach(), yA.detach(), z2A.detach()

    hi, vA, yA, z2A = absolute(torch.clamp(on1 + u1, max=1))
    lo = absolute(on1 * (1 - u1))[0]
    vd, yd = v.detach(), y.detach()

    def var_bound(x, xA, dims):  # d var = mean(2 (x - mu)(dx - dmu)), |dx| <= gam_f xA; + the reduction's own roundings
        e, mu = gam_f * xA, x.mean(dims, keepdim=True)
        return (2 * ((x - mu).abs() * (e + e.mean(dims, keepdim=True))).mean(dims) + gam_f * x.var(dims, unbiased=False)).numpy()

    out = {k: (L[k].grad.numpy(), gam * hi[k] + (hi[k] - lo[k]) + tr.FLOOR) for k in L}
    out.update(x=(torch.relu(z2).detach().numpy(), gam_f * z2A.numpy() + tr.FLOOR),
               bn1_mean=(vd.mean((0, 2, 3)).numpy(), gam_f * vA.mean((0, 2, 3)).numpy() + tr.FLOOR),
               bn1_var=(vd.var((0, 2, 3), unbiased=False).numpy(), var_bound(vd, vA, (0, 2, 3)) + tr.FLOOR),
               bn2_mean=(yd.mean(0).numpy(), gam_f * yA.mean(0).numpy() + tr.FLOOR),
               bn2_var=(yd.var(0, unbiased=False).numpy(), var_bound(yd, yA, (0,)) + tr.FLOOR))
    out["unstable"] = (float(u1.mean()), float(u2.mean()))
    return out


def outside(got, ref):
    return bool((np.abs(np.asarray(got, np.float64).reshape(ref[0].shape) - ref[0]) > ref[1]).any())


def shows(c):
    """the gradients that are not identically 0 in exact arithmetic: bn1 removes the scale of a 1 x 1 filter (conv_w at
    fs = 1) and every conv_b; bn2 removes proj_b unless the projection mask stands between them"""
    return ("s_emb", "p_emb", "proj_w") + (("conv_w",) if c["fs"] > 1 else ()) + (("proj_b",) if c["ps"][1] > 0 else ())


def informative(c, ref):
    """the stability condition of a case: few charged units, and a bound below most of every non-zero gradient"""
    u1, u2 = ref["unstable"]
    assert u1 < 1e-3 and u2 < (0.1 if c["n"] > 2 else 0.15), (u1, u2)  # (n = 2: a column masked in both rows has z = 0)
    if c["n"] > 2:  # (n = 2: bn2 maps every column to +-1 whatever y is, so every gradient is 0 up to eps)
        for k in shows(c):
            assert float((np.abs(ref[k][0]) > ref[k][1]).mean()) > 0.3, k


@pytest.mark.parametrize("n", [33, 70])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_bound_rejects_planted_defects_on_the_cpu(shape, n):
    c = make(*shape, n, True, (0.2, 0.3))  # (cases of the GPU test below)
    ref = reference(c)
    informative(c, ref)
    for k in GRADS:
        assert not outside(ref[k][0], ref[k]), k
    assert all(outside(2 * ref[k][0], ref[k]) for k in shows(c)), "a gradient scaled by two"
    gx = c["gx"].copy()
    gx[32:] = 0  # the rows behind the first row tile dropped from the backward
    cut = reference(c, gx=gx)
    assert all(outside(cut[k][0], ref[k]) for k in shows(c)), "a dropped tile"
    m = c["m"].copy()
    i, j = max(np.argwhere(m == 0), key=lambda e: abs(c["gx"][e[0], e[1]]))
    m[i, j] = m.max()  # one dropped element passes
    bad = reference(c, m=m)
    # g_u[i, j] alone changes: it feeds proj_w[j, :] and proj_b[j] directly and every other gradient as one term of d
    assert outside(bad["proj_w"][0], ref["proj_w"]) and outside(bad["proj_b"][0], ref["proj_b"]), "an unmasked element"


class Run:
    """the two C calls on NaN-guarded buffers; ld: extra floats per row of every pitched operand (+ a 4-byte offset)"""

    def __init__(self, c, dev, ld=0):
        from kge_amd import _lib
        self.c, self.dev, self.L, self.bufs = c, dev, _lib.lib(), []
        P, d, F, n = c["P"], c["d"], c["F"], c["n"]
        self.t = {k: None if v is None else self.put(v.reshape(v.shape[0], -1), ld if k in ("s_emb", "p_emb", "proj_w") else 0)
                  for k, v in P.items()}
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        self.net = _lib.KgeConveNet(c["h"], c["w"], c["fs"], c["pad"], 0 if P["conv_b"] is None else 1, 0,
                                    ptr(self.t["conv_w"]), ptr(self.t["conv_b"]), None, None, ptr(self.t["proj_w"]),
                                    F + ld, ptr(self.t["proj_b"]), None, None, EPS, EPS)
        self.tr = _lib.KgeConveTrain(c["ps"][0], c["ps"][1], SEED, CALL)
        self.need = self.L.kge_conve_train_workspace_bytes(ctypes.byref(self.net), n)
        assert self.need > 0
        o = self.out = {k: self.put(np.full(s, np.nan, np.float32), l) for k, s, l in (
            ("x", (n, d), ld), ("y", (n, d), 0), ("bn1_mean", (1, 32), 0), ("bn1_var", (1, 32), 0), ("bn2_mean", (1, d), 0),
            ("bn2_var", (1, d), 0), ("s_emb", (n, d + 1), ld), ("p_emb", (n, d + 1), ld), ("conv_w", (32, c["fs"] ** 2), 0),
            ("conv_b", (1, 32), 0), ("proj_w", (d, F), ld), ("proj_b", (1, d), 0), ("ws", (1, self.need // 4), 0))}
        gx = self.put(c["gx"], ld)
        st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        a = (ctypes.byref(self.net), ctypes.byref(self.tr), ptr(self.t["s_emb"]), d + 1 + ld, ptr(self.t["p_emb"]), d + 1 + ld, n)
        stats = tuple(ptr(o[k]) for k in ("bn1_mean", "bn1_var", "bn2_mean", "bn2_var"))
        assert self.L.kge_conve_train_fwd(*a, ptr(o["x"]), d + ld, ptr(o["y"]), *stats, ptr(o["ws"]), self.need, st) == 0
        assert self.L.kge_conve_train_bwd(*a, ptr(gx), d + ld, ptr(o["y"]), *stats, ptr(o["s_emb"]), d + 1 + ld, ptr(o["p_emb"]),
                                          d + 1 + ld, ptr(o["conv_w"]), ptr(o["conv_b"]) if P["conv_b"] is not None else None,
                                          ptr(o["proj_w"]), F + ld, ptr(o["proj_b"]), ptr(o["ws"]), self.need, st) == 0
        torch.cuda.synchronize(dev)
        for buf, lo, hi, view in self.bufs:
            assert bool(torch.isnan(buf[:lo]).all()) and bool(torch.isnan(buf[hi:]).all()), "guard words"
            if view.stride(0) > view.shape[1] and view.shape[0] > 1:
                gaps = torch.as_strided(view, (view.shape[0] - 1, view.stride(0) - view.shape[1]), view.stride(),
                                        view.storage_offset() + view.shape[1])
                assert bool(torch.isnan(gaps).all()), "between the rows"

    def put(self, a, ld):
        r, k = a.shape
        lo = 8 + (1 if ld else 0)
        buf = torch.full((lo + r * (k + ld) + 8,), float("nan"), device=self.dev)
        view = buf[lo:lo + r * (k + ld)].view(r, k + ld)[:, :k]
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        self.bufs.append((buf, lo, lo + r * (k + ld), view))
        return view

    def results(self):
        skip = ("ws", "y") + (("conv_b",) if self.c["P"]["conv_b"] is None else ())
        return {k: v.clone() for k, v in self.out.items() if k not in skip}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible")
    return torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("ps", [(0.0, 0.0), (0.2, 0.3)])
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("n", [2, 33, 70])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_and_backward_within_the_bound_and_bit_equal(dev, shape, n, bias, ps):
    from kge_amd import _lib
    c = make(*shape, n, bias, ps)
    ref = reference(c)
    informative(c, ref)
    run = Run(c, dev)
    got = run.results()
    for k, v in got.items():
        err = np.abs(v.double().cpu().numpy().reshape(ref[k][0].shape) - ref[k][0])
        WORST[k] = max(WORST.get(k, 0.0), float((err / ref[k][1]).max()))
        assert (err <= ref[k][1]).all(), (k, float((err / ref[k][1]).max()))
    assert bool((got["s_emb"][:, 0] == 0).all()) and bool((got["p_emb"][:, 0] == 0).all()), "column 0 of the row gradients"
    again = Run(c, dev).results()
    assert all(torch.equal(got[k], again[k]) for k in got), "two runs, the same bits"
    print("conve_train_bound:", " ".join("{} {:.4f}".format(k, r) for k, r in sorted(WORST.items())))
    if ps == (0.0, 0.0):  # the batch statistics as running statistics of kge_conve_queries: the same bits
        d, o = c["d"], run.out
        net = _lib.KgeConveNet.from_buffer_copy(run.net)
        net.bn1_mean, net.bn1_var = o["bn1_mean"].data_ptr(), o["bn1_var"].data_ptr()
        net.bn2_mean, net.bn2_var = o["bn2_mean"].data_ptr(), o["bn2_var"].data_ptr()
        q = torch.empty(n, d + 1, device=dev)
        ws = torch.empty(run.L.kge_conve_workspace_bytes(ctypes.byref(net), n), dtype=torch.uint8, device=dev)
        rng = _lib.KgeIndex(None, _lib.I64, 0, 1)
        assert run.L.kge_conve_queries(ctypes.byref(net), run.t["s_emb"].data_ptr(), d + 1, run.t["p_emb"].data_ptr(), d + 1,
                                       rng, rng, n, q.data_ptr(), d + 1, ws.data_ptr(), ws.numel(), None) == 0
        torch.cuda.synchronize(dev)
        assert torch.equal(q[:, 1:], got["x"]), "bit equality with the eval kernel"


@pytest.mark.gpu
def test_a_width_whose_projection_block_does_not_fit_the_lds(dev):
    """d = 496 > 486: ct_feature_bwd_kernel reads proj_w[:, block] through L2 and splits the outputs over two workgroups"""
    test_forward_and_backward_within_the_bound_and_bit_equal(dev, (16, 31, 1, 0), 33, True, (0.2, 0.3))


@pytest.mark.gpu
def test_pitched_unaligned_rows_give_the_same_bits(dev):
    c = make(4, 8, 3, 1, 33, True, (0.2, 0.3))
    want, got = Run(c, dev).results(), Run(c, dev, ld=3).results()
    assert all(torch.equal(want[k], got[k]) for k in want)


@pytest.mark.gpu
def test_model_takes_the_train_route_and_updates_the_running_statistics(dev):
    from kge_amd import model
    ms = [model.create("conve", 40, 5, 32, device=dev, feature_map_dropout=0.0, projection_dropout=0.0, fused_train=ft)
          for ft in (True, False)]
    ms[1].load_state_dict(ms[0].state_dict())
    s, p = torch.arange(33, device=dev) % 40, torch.arange(33, device=dev) % 5
    for m in ms:
        m.train()
        m.score_sp(s, p).square().sum().backward()
    assert ms[0].routes == {"kernel": 0, "torch": 0, "train": 1} and ms[1].routes == {"kernel": 0, "torch": 1}
    for (k, a), b in zip(ms[0].state_dict().items(), ms[1].state_dict().values()):
        # gamma_{K_fwd} of this shape (K_fwd = 3619) is 2.2e-4, of statistics of magnitude O(1) under momentum 0.1
        assert torch.allclose(a.double(), b.double(), rtol=2.2e-4, atol=2.2e-5), k
    for (k, a), (_, b) in zip(ms[0].named_parameters(), ms[1].named_parameters()):
        # both routes are float32 evaluations inside gamma_K A of the float64 gradient: K = 1.1e3 here (roundings), A
        # below 20 max |g| on these inputs -> 2 x 6.6e-5 x 20 of the largest element
        # (both biases: identically 0 behind their batch-norm with the dropouts at 0, noise on both routes -- held to the
        # scale of their layer's weight gradient)
        scale = getattr(ms[1].get_scorer(), k.split(".")[-2]).weight.grad if k.endswith(".bias") else b.grad
        assert a.grad is not None and float((a.grad - b.grad).abs().max()) <= 2.7e-3 * float(scale.abs().max()), k
    assert int(ms[0].get_scorer().bn1.num_batches_tracked) == 1
    ms[0].eval()
    with torch.no_grad():
        ms[0].score_sp(s, p)
    assert ms[0].routes == {"kernel": 1, "torch": 0, "train": 1}
