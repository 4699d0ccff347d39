"""Fused KvsAll kl / bce losses of float32 ComplEx / DistMult (kge_kl_f32_* / kge_bce_f32_*) without a GPU: the
declarations, the argument checks of the C entries and of the engine, the float64 references of tests/_multilabel_f32_ref.py
against torch autograd of KgeModel._kl_composed / _bce_composed, and the control flow of hip_KvsAll with
`fused_f32_loss` (stand-ins for the engine calls; the models' and the job's own code runs)."""
import ctypes
import os
import re
import shutil
import types

import numpy as np
import pytest
import torch

import _multilabel_f32_ref as ref
import ref_harness as rh
import torch_port as tp
from conftest import ROOT

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")
ENTRIES = ("kge_multilabel_f32_workspace_bytes", "kge_kl_f32_fwd", "kge_kl_f32_bwd", "kge_bce_f32_fwd", "kge_bce_f32_bwd")


def test_entries_are_declared_documented_exported_and_bound():
    from kge_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    _lib.build()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.M), name
    doc = header[header.index("kge_kl_f32_fwd / _bwd and kge_bce_f32_fwd / _bwd"):
                 header.index("int64_t kge_multilabel_f32_workspace_bytes")]
    for name in ENTRIES:  # each entry cites the reference's lines
        assert re.search(name + r"[^\n]*\(train_KvsAll\.py:\d+-\d+", doc), name
    for cite in ("train_KvsAll.py:216-294", "loss.py:137-159", "loss.py:192-213", "complex.py:30-39", "distmult.py:15-21",
                 "KGE_ERR_WORKSPACE", "KGE_ERR_UNSUPPORTED", "label_bias", "BIT-EQUAL", "ANY\n * order"):
        assert cite in doc, cite
    # the label scores are not the bits of kge_score_sp / kge_score_po: said in kge_kl_fwd's words
    flat = " ".join(doc.replace("*", " ").split())
    assert "the same operands as the matrix-core kernel in a different f32 summation order" in flat
    ext = _lib.ext()
    for name in ("multilabel_f32_workspace_bytes", "kl_f32_fwd", "kl_f32_bwd", "bce_f32_fwd", "bce_f32_bwd"):
        assert hasattr(ext, name), name
    assert lib.kge_abi_version() == 1


def test_c_entries_validate_arguments_without_a_device():
    from kge_amd import _lib
    from kge_amd._lib import KgeIndex, KgeTables
    _lib.build()
    lib = _lib.lib()
    P = ctypes.c_void_p(256)  # never dereferenced on these paths
    good, null = KgeIndex(P, 1, 0, 1), KgeIndex(None, 1, 0, 1)

    def mk(dtype, scorer, d=32, dr=None, ld=None, ent=P):
        dr = d if dr is None else dr
        return KgeTables(ent, P, dtype, scorer, 1000, 3, d, dr, ld or d, dr, 1.0, 0)

    cx, dm = mk(0, 0), mk(0, 1)
    ws = lambda t, n, c: lib.kge_multilabel_f32_workspace_bytes(ctypes.byref(t), n, c)
    ws_ce = lambda t, n, c: lib.kge_ce_f32_workspace_bytes(ctypes.byref(t), n, c)
    al = lambda b: -(-b // 256) * 256
    # kge_ce_f32's layout (records | dQ | Q | split-K partials | G [n, chunk]) + n x chunk bits, each part on 256 bytes
    nd = 100 * 32 * 4
    rec = al(100 * 3 * 4 * 8)
    assert ws(cx, 100, 128) == rec + 2 * al(nd) + al(32 * nd) + al(100 * 128 * 4) + al(100 * 128 // 8)
    for c in (128, 256, 0):
        cols = min(c or (32 << 20) // 400 // 128 * 128, 1024)
        assert ws(cx, 100, c) == ws_ce(cx, 100, c) + al(100 * cols // 8), c
    assert ws(cx, 100, 0) == ws(cx, 100, 1024) == ws(cx, 100, 1 << 20)   # clamped to E rounded up to 128
    assert ws(cx, 100, 128) < ws(cx, 100, 256) < ws(cx, 100, 0)
    assert ws(dm, 100, 0) == ws(cx, 100, 0) and ws(mk(0, 0, 32, ld=36), 100, 0) > 0
    assert ws(cx, 100, 64) == 0 and ws(cx, 100, -128) == 0 and ws(cx, 0, 0) == 0
    kl_f = lambda t=cx, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_kl_f32_fwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, None, out, out, w, wb, None)
    kl_b = lambda t=cx, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_kl_f32_bwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, None, None, P, None, 1.0, P, P, out, w, wb, None)
    bce_f = lambda t=cx, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_bce_f32_fwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, 0.5, out, w, wb, None)
    bce_b = lambda t=cx, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_bce_f32_bwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, 0.5, None, 1.0, P, P, out, w, wb, None)
    calls = (kl_f, kl_b, bce_f, bce_b)
    # bf16, TransE, RotatE, dim % 8, a row pitch or a base off 16 bytes
    for t in (mk(1, 0), mk(1, 1), mk(0, 2), mk(0, 3, 32, 16), mk(0, 0, 36), mk(0, 1, 12), mk(0, 0, 32, ld=33),
              mk(0, 0, ent=ctypes.c_void_p(260))):
        assert ws(t, 100, 0) == 0
        for call in calls:
            assert call(t=t) == -2
    for call in calls:
        assert call(dirc=0) == -1 and call(dirc=3) == -1
        assert call(n=-1) == -1
        assert call(a=null) == -1
        assert call(rp=None) == -1            # no label CSR
        assert call(out=None) == -1           # loss_rows / lse, g_tgt
        assert call(w=None) == -5 and call(wb=64) == -5
        assert call(w=ctypes.c_void_p(264)) == -5   # not on 256 bytes
    assert lib.kge_kl_f32_fwd(None, 1, good, good, 4, P, P, None, P, P, P, 1 << 20, None) == -1
    assert lib.kge_kl_f32_bwd(ctypes.byref(cx), 1, good, good, 4, P, P, None, None, None, None, 1.0, P, P, P, P, 1 << 20,
                              None) == -1   # no lse
    # empty batch: nothing to do for the forward, no CSR, no outputs, no workspace needed
    assert kl_f(n=0, a=null, rp=None, out=None, w=None, wb=0) == 0
    assert bce_f(n=0, a=null, rp=None, out=None, w=None, wb=0) == 0
    assert kl_b(n=0, a=null, rp=None, out=None, w=None, wb=0) == -1   # (the backward zero-fills g_tgt: it must exist)
    # the documented minima.  forward: the records and the two [n, dim] buffers; backward: 128 columns
    fwd_min = al(4 * 3 * 4 * 8) + 2 * al(4 * 32 * 4)
    for call in (kl_f, bce_f):
        assert call(wb=fwd_min - 1) == -5
    for call in (kl_b, bce_b):
        assert call(wb=ws(cx, 4, 128) - 1) == -5
    assert ws(cx, 4, 128) - 1 >= fwd_min
    # the existing entries keep declining float32 tables
    assert lib.kge_kl_fwd(ctypes.byref(cx), 1, good, good, 4, P, P, P, P, P, 1 << 20, None) == -2
    assert lib.kge_kl_dist_fwd(ctypes.byref(cx), 1, good, good, 4, P, P, None, P, P, P, 1 << 20, None) == -2


def _cpu_tables(scorer, dtype=torch.float32, d=8):
    """engine.Tables refuses CPU tensors in its constructor; the checks under test come before any device is asked."""
    from kge_amd import engine
    t = engine.Tables.__new__(engine.Tables)
    t.scorer = engine.SCORERS[scorer]
    t.ent, t.rel = torch.zeros(10, d, dtype=dtype), torch.zeros(3, d, dtype=dtype)
    t.l_norm, t.flags, t.device, t._c_cache = 1.0, 0, t.ent.device, {}
    return t


def test_engine_refuses_bad_arguments_with_the_usual_exceptions():
    from kge_amd import engine
    ix4, ix5 = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    rp, cl, rows = torch.arange(5), torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    calls = (lambda t, a, rp_=rp, cl_=cl, **k: engine.kl_f32_fwd(t, "sp", a, ix4, rp_, cl_, **k),
             lambda t, a, rp_=rp, cl_=cl, **k: engine.kl_f32_bwd(t, "sp", a, ix4, rp_, cl_, rows, **k),
             lambda t, a, rp_=rp, cl_=cl, **k: engine.bce_f32_fwd(t, "po", a, ix4, rp_, cl_, 0.5, **k),
             lambda t, a, rp_=rp, cl_=cl, **k: engine.bce_f32_bwd(t, "po", a, ix4, rp_, cl_, 0.5, **k))
    for call in calls:
        with pytest.raises(ValueError, match="different lengths"):
            call(_cpu_tables("complex"), ix5)
        for cc in (64, 129, -128):
            with pytest.raises(ValueError, match="multiple of 128"):
                call(_cpu_tables("complex"), ix4, chunk_cols=cc)
        for bad in (_cpu_tables("complex", torch.bfloat16), _cpu_tables("distmult", torch.bfloat16),
                    _cpu_tables("transe"), _cpu_tables("rotate")):
            with pytest.raises(RuntimeError, match="ComplEx / DistMult on float32"):
                call(bad, ix4)
        with pytest.raises(RuntimeError, match="multiple of 8"):
            call(_cpu_tables("complex", d=12), ix4)
        with pytest.raises(ValueError, match="rowptr has 4 entries for 4 rows"):
            call(_cpu_tables("complex"), ix4, torch.arange(4))
        with pytest.raises(TypeError, match="holds integers"):
            call(_cpu_tables("complex"), ix4, torch.arange(5).float())
        with pytest.raises(ValueError, match="two 1-d tensors"):
            call(_cpu_tables("complex"), ix4, rp, cl.view(2, 2))
        # a non-contiguous CSR and valid arguments get as far as the device question: the path has no CPU fallback
        with pytest.raises(RuntimeError, match="no CPU path"):
            call(_cpu_tables("distmult"), ix4, torch.arange(10)[::2], chunk_cols=256)
    with pytest.raises(ValueError, match="lse has 3 entries for 4 rows"):
        engine.kl_f32_bwd(_cpu_tables("complex"), "sp", ix4, ix4, rp, cl, torch.zeros(3))
    with pytest.raises(ValueError, match="label_bias has 5 entries for 4 rows"):
        engine.kl_f32_bwd(_cpu_tables("complex"), "sp", ix4, ix4, rp, cl, rows, label_bias=torch.zeros(5))
    assert not engine.multilabel_f32_supported(_cpu_tables("complex"))


def _problem(name, seed=3):
    rng = np.random.default_rng(seed)
    E, R, d, n = 300, 4, 16, 21
    ent, rel = rng.standard_normal((E, d)), rng.standard_normal((R, d))
    a, p = rng.integers(0, E, n), rng.integers(0, R, n)
    a[5] = a[6]
    rowptr, col = ref.labels(rng, n, E)
    return E, R, d, n, ent, rel, a, p, rowptr, col, rng.uniform(0.1, 1.0, n)


@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("name", ["complex", "distmult"])
@pytest.mark.parametrize("direction", ["sp", "po"])
def test_references_equal_torch_autograd_of_the_composed_losses(name, direction, eps):
    """The float64 references the GPU tests compare against -- loss rows, lse and the three gradients of the chunked
    backward with its explicit bit mask (chunk widths 128, 256, one chunk) -- equal float64 autograd of
    KgeModel._kl_composed / _bce_composed on the ported scorer to 1e-12, without and with label smoothing (the weighted
    kernel + label_bias + the value terms for kl; the kernel + the two linear terms for bce: kl_fused / bce_fused)."""
    from kge_amd import model as km
    E, R, d, n, ent, rel, a, p, rowptr, col, g = _problem(name)
    rp_t, cl_t = torch.from_numpy(rowptr), torch.from_numpy(col)
    assert np.diff(rowptr)[:7].tolist() == [0, 1, 2, 63, 64, 65, 130]
    x = ref.scores(name, direction, ent, rel, a, p)
    hit = ref.dense(rowptr, col, n, E)
    for kind in ("kl", "bce"):
        e64, r64 = torch.from_numpy(ent).requires_grad_(), torch.from_numpy(rel).requires_grad_()
        ai, pi = torch.from_numpy(a), torch.from_numpy(p)
        ea, rp = e64[ai], r64[pi]
        ea.retain_grad(), rp.retain_grad()
        sc = tp.score_emb(name, ea, rp, e64, "sp_") if direction == "sp" else tp.score_emb(name, e64, rp, ea, "_po")
        assert np.abs(x - sc.detach().numpy()).max() <= 1e-12
        rows = (km.KgeModel._kl_composed(sc, rp_t, cl_t, eps) if kind == "kl"
                else km.KgeModel._bce_composed(sc, rp_t, cl_t, 0.75, eps))
        (rows * torch.from_numpy(g)).sum().backward()
        kw, extra = {}, None
        if kind == "kl" and eps == 0.0:
            loss, lse = ref.kl_forward(name, direction, ent, rel, a, p, rowptr, col)
        elif kind == "kl":
            w, b, const = ref.smoothing_terms(rowptr, E, eps)
            loss, lse = ref.kl_forward(name, direction, ent, rel, a, p, rowptr, col, w)
            loss = loss - b * x.sum(axis=1) + const
            kw = {"label_weight": w, "label_bias": b}
        else:
            loss, lse = ref.bce_forward(name, direction, ent, rel, a, p, rowptr, col, 0.75), None
            kw = {"offset": 0.75}
            if eps > 0.0:
                loss = loss + eps * ((x + 0.75) * hit).sum(axis=1) - (x + 0.75).sum(axis=1) / E
                extra = ref.dense_backward(name, direction, ent, rel, a, p, g[:, None] * (eps * hit - 1.0 / E))
        assert np.abs(loss - rows.detach().numpy()).max() <= 1e-12, kind
        if lse is not None:
            assert np.abs(lse - torch.logsumexp(sc, 1).detach().numpy()).max() <= 1e-12
        for cc in (128, 256, 0):
            g_a, g_p, g_t = ref.chunked_backward(kind, name, direction, ent, rel, a, p, rowptr, col, g, cc, **kw)
            assert not np.isnan(g_t).any()
            if extra is not None:
                g_a, g_p, g_t = g_a + extra[0], g_p + extra[1], g_t + extra[2]
            ge = g_t.copy()
            np.add.at(ge, a, g_a)
            gr = np.zeros_like(rel)
            np.add.at(gr, p, g_p)
            for nm, got, want in (("g_a", g_a, ea.grad), ("g_p", g_p, rp.grad), ("entity", ge, e64.grad),
                                  ("relation", gr, r64.grad)):
                err = np.abs(got - want.numpy()).max()
                assert err <= 1e-12, (kind, cc, nm, err)


def test_the_label_generator_and_the_bit_mask():
    rng = np.random.default_rng(0)
    rowptr, col = ref.labels(rng, 40, 129)
    k = np.diff(rowptr)
    assert k[:7].tolist() == [0, 1, 2, 63, 64, 65, 129] and set(ref.edge_columns(129)) <= set(col[rowptr[5]:rowptr[6]].tolist())
    for c0, C in ((0, 128), (128, 128), (0, 256)):
        mc = min(C, 129 - c0)
        mask = ref.chunk_mask(rowptr, col, 40, c0, mc, C)
        y = np.arange(C)
        bits = (mask[:, y >> 5] >> (y & 31).astype(np.uint32)) & 1
        want = np.zeros((40, C))
        want[:, :mc] = ref.dense(rowptr, col, 40, 129)[:, c0:c0 + mc]
        assert np.array_equal(bits, want)
    bad = ref.chunk_mask(np.array([0, 2]), np.array([-1, 129]), 1, 0, 129, 256)
    assert not bad.any()


@pytest.mark.parametrize("name", ["complex", "distmult"])
def test_model_declines_to_the_composed_loss_on_cpu(name, monkeypatch):
    from kge_amd import model as km
    m = km.create(name, 30, 4, 8, fused_f32_loss=True)
    assert m.fused_f32_loss and m._ce_f32_tables() is None
    g = torch.Generator().manual_seed(0)
    s, p = (torch.randint(hi, (6,), generator=g) for hi in (30, 4))
    rowptr, col = torch.tensor([0, 2, 2, 3, 6, 7, 9]), torch.tensor([5, 1, 0, 29, 3, 17, 8, 2, 11])
    sc_sp, sc_po = torch.randn(6, 30, generator=g), torch.randn(6, 30, generator=g)
    monkeypatch.setattr(m, "score_sp", lambda s_, p_, o_=None: sc_sp)
    monkeypatch.setattr(m, "score_po", lambda p_, o_, s_=None: sc_po)
    for fn in (km._FusedKLF32, km._FusedBCEF32):
        monkeypatch.setattr(fn, "forward", staticmethod(lambda *a, **k: pytest.fail("fused function entered on CPU")))
    for eps in (0.0, 0.1):
        assert torch.equal(m.kl_loss_sp(s, p, rowptr, col, eps), km.KgeModel._kl_composed(sc_sp, rowptr, col, eps))
        assert torch.equal(m.kl_loss_po(p, s, rowptr, col, eps), km.KgeModel._kl_composed(sc_po, rowptr, col, eps))
        assert torch.equal(m.bce_loss_sp(s, p, rowptr, col, 1.5, eps), km.KgeModel._bce_composed(sc_sp, rowptr, col, 1.5, eps))
        assert torch.equal(m.bce_loss_po(p, s, rowptr, col, 1.5, eps), km.KgeModel._bce_composed(sc_po, rowptr, col, 1.5, eps))


# ---- the plugin's control flow ------------------------------------------------------------------------------------------
def _job(tmp, model, option, loss="kl", smoothing=0.0, base=None, extra=(), repeat_a_triple=False, train_type="hip_KvsAll"):
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    data = os.path.join(tmp, "dataset_test" + ("_repeat" if repeat_a_triple else ""))
    if not os.path.isdir(data):
        shutil.copytree(os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"), data)
        if repeat_a_triple:  # the first training triple a second time
            path = os.path.join(data, "train.del")
            lines = open(path).read().splitlines()
            open(path, "w").write("\n".join(lines + lines[:1]) + "\n")
            meta = os.path.join(data, "dataset.yaml")
            open(meta, "w").write(open(meta).read().replace("files.train.size: %d" % len(lines),
                                                            "files.train.size: %d" % (len(lines) + 1)))
    config = Config()
    config.folder = os.path.join(tmp, f"run_{model}_{option}_{len(os.listdir(tmp))}")
    os.makedirs(config.folder, exist_ok=True)
    config.set("console.quiet", True)
    config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
    config.set("model", model)
    config._import(model)
    if base is not None:
        config._import(base)
        config.set(f"{model}.base_model.type", base)
    config.set("dataset.name", "dataset_test")
    config.set("job.device", "cpu")
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 32)
    config.set("train.num_workers", 0)
    config.set("train.loss", loss)
    if loss == "bce":
        config.set("train.loss_arg", -0.5)  # score offset
    config.set("KvsAll.label_smoothing", smoothing)
    config.set("lookup_embedder.dim", 16)
    config.set("random_seed.default", 7)
    config._import(train_type)
    config.set("train.type", train_type)
    if option is not None:
        config.set(train_type + ".fused_f32_loss", option)
    for k, v in extra:
        config.set(k, v)
    torch.manual_seed(21)
    return TrainingJob.create(config, Dataset.create(config, folder=data))


class _Tables:
    """stand-in for engine.Tables (which refuses CPU tensors)"""

    def __init__(self, name, ent, rel, l_norm=1.0, flags=0):
        self.name, self.ent, self.rel = name, ent, rel


class _TorchSPO:
    """stand-in for kge_amd.model._ScoreSPO (kge_score_spo): the ported scorer, differentiable"""

    @staticmethod
    def apply(name, l_norm, ent, rel, s, p, o):
        return tp.score_spo(name, ent, rel, s.long(), p.long(), o.long())


class _TorchEmb:
    """stand-in for kge_amd.model._ScoreEmb (kge_score_emb)"""

    @staticmethod
    def apply(name, combine, l_norm, s_emb, p_emb, o_emb):
        return tp.score_emb(name, s_emb, p_emb, o_emb, combine)


def _instrument(monkeypatch, target):
    """There is no HIP device here.  Stand-ins: engine.Tables / ce_f32_supported / kl_f32_* / bce_f32_* (float64 numpy of
    tests/_multilabel_f32_ref.py; the backward walks chunks of 128 columns through its bit mask), the two scoring
    functions bce_fused composes the smoothing terms from, and the ONE device question of the model's decision --
    `_fused()` asks whether the parameters are on a GPU -- answered as if they were, inside `_ce_f32_tables()` only.
    Everything else is the project's code: the job's routing, the hooks, kl_fused / bce_fused, _FusedKLF32 / _FusedBCEF32.
    score_sp / score_po count and go on to the composed path."""
    from kge.model import LookupEmbedder
    from kge_amd import engine
    from kge_amd import model as km
    calls = {"kl_fwd": 0, "kl_bwd": 0, "bce_fwd": 0, "bce_bwd": 0, "score_sp": 0, "score_po": 0, "directions": set(),
             "bias": 0, "weight": 0}
    npy = lambda x: None if x is None else x.detach().cpu().numpy()
    f32 = lambda x: torch.from_numpy(np.asarray(x)).float()

    def kl_fwd(t, direction, a, p, rp, cl, label_weight=None, chunk_cols=0):
        calls["kl_fwd"] += 1
        calls["weight"] += label_weight is not None
        calls["directions"].add(direction)
        loss, lse = ref.kl_forward(t.name, direction, npy(t.ent), npy(t.rel), npy(a), npy(p), npy(rp), npy(cl), npy(label_weight))
        return f32(loss), f32(lse)

    def kl_bwd(t, direction, a, p, rp, cl, lse, g_rows=None, g_scalar=1.0, label_weight=None, label_bias=None, chunk_cols=0):
        calls["kl_bwd"] += 1
        calls["bias"] += label_bias is not None
        out = ref.chunked_backward("kl", t.name, direction, npy(t.ent), npy(t.rel), npy(a), npy(p), npy(rp), npy(cl),
                                   npy(g_rows), 128, npy(label_weight), npy(label_bias))
        return tuple(f32(x) for x in out)

    def bce_fwd(t, direction, a, p, rp, cl, offset=0.0, chunk_cols=0):
        calls["bce_fwd"] += 1
        calls["directions"].add(direction)
        return f32(ref.bce_forward(t.name, direction, npy(t.ent), npy(t.rel), npy(a), npy(p), npy(rp), npy(cl), offset))

    def bce_bwd(t, direction, a, p, rp, cl, offset=0.0, g_rows=None, g_scalar=1.0, chunk_cols=0):
        calls["bce_bwd"] += 1
        out = ref.chunked_backward("bce", t.name, direction, npy(t.ent), npy(t.rel), npy(a), npy(p), npy(rp), npy(cl),
                                   npy(g_rows), 128, offset=offset)
        return tuple(f32(x) for x in out)

    monkeypatch.setattr(engine, "Tables", _Tables)
    monkeypatch.setattr(engine, "ce_f32_supported", lambda t: t.ent.dtype == torch.float32 and t.ent.shape[1] % 8 == 0)
    for nm, f in (("kl_f32_fwd", kl_fwd), ("kl_f32_bwd", kl_bwd), ("bce_f32_fwd", bce_fwd), ("bce_f32_bwd", bce_bwd)):
        monkeypatch.setattr(engine, nm, f)
    monkeypatch.setattr(km, "_ScoreSPO", _TorchSPO)
    monkeypatch.setattr(km, "_ScoreEmb", _TorchEmb)

    def fused_but_for_the_device(self):
        se, oe, pe = self.get_s_embedder(), self.get_o_embedder(), self.get_p_embedder()
        if se is not oe or type(se) is not LookupEmbedder or type(pe) is not LookupEmbedder:
            return False
        return not (self.training and (se.dropout.p > 0 or pe.dropout.p > 0))

    real = type(target)._ce_f32_tables

    def ce_f32_tables(self):
        self._fused = types.MethodType(fused_but_for_the_device, self)
        try:
            return real(self)
        finally:
            del self._fused

    target._ce_f32_tables = types.MethodType(ce_f32_tables, target)
    for nm in ("score_sp", "score_po"):
        def counted(self, *a, _nm=nm, _f=getattr(type(target), nm), **k):
            calls[_nm] += 1
            return _f(self, *a, **k)
        setattr(target, nm, types.MethodType(counted, target))
    return calls


def _epoch(job):
    job._prepare()
    trace = job.run_epoch()
    return trace["avg_loss"], {k: v.detach().clone() for k, v in job.model.state_dict().items()}


def _query_types_per_epoch(job):
    """(batch, query type) pairs of an epoch: what the per-type loop of _process_subbatch iterates over"""
    pairs = [0]
    inner = job._process_subbatch

    def counted(batch_index, batch, subbatch_slice, result):
        pairs[0] += int(torch.unique(batch["query_type_indexes"][subbatch_slice]).numel())
        return inner(batch_index, batch, subbatch_slice, result)

    job._process_subbatch = counted
    return pairs


@needs_reference
@pytest.mark.parametrize("loss,smoothing", [("kl", 0.0), ("kl", 0.4), ("bce", 0.0), ("bce", 0.4)])
@pytest.mark.parametrize("model", ["hip_complex", "hip_distmult"])
def test_fused_f32_loss_routes_a_float32_job_through_the_fused_functions(tmp_path, monkeypatch, model, loss, smoothing):
    """hip_KvsAll.fused_f32_loss: true -- every query type of every batch of a float32 hip_complex / hip_distmult job goes
    through kl_loss_* / bce_loss_* into _FusedKLF32 / _FusedBCEF32 (one engine forward and one engine backward each),
    WITH label smoothing too (the weighted kernel and label_bias), and never score_sp / score_po; the epoch's avg_loss and
    the parameters after it are those of the option-off job."""
    job = _job(str(tmp_path), model, True, loss=loss, smoothing=smoothing)
    assert type(job).__name__ == "HipTrainingJobKvsAll" and job.model._fused_f32_loss is True
    calls = _instrument(monkeypatch, job.model)
    pairs = _query_types_per_epoch(job)
    l_on, st_on = _epoch(job)
    other = "bce" if loss == "kl" else "kl"
    assert pairs[0] >= len(job.loader)
    assert calls[loss + "_fwd"] == calls[loss + "_bwd"] == pairs[0], (calls, pairs)
    assert calls[other + "_fwd"] == calls[other + "_bwd"] == calls["score_sp"] == calls["score_po"] == 0, calls
    assert calls["directions"] == {"sp", "po"}
    if loss == "kl":
        assert calls["weight"] == calls["bias"] == (pairs[0] if smoothing else 0), calls
    monkeypatch.undo()
    plain = _job(str(tmp_path), model, None, loss=loss, smoothing=smoothing)
    assert plain.model._fused_f32_loss is False
    l_off, st_off = _epoch(plain)
    assert abs(l_on - l_off) <= 1e-5 * max(1.0, abs(l_off)), (l_on, l_off)
    for k in st_off:
        assert torch.allclose(st_on[k], st_off[k], rtol=1e-4, atol=1e-6), k


@needs_reference
@pytest.mark.parametrize("model,option,extra", [
    ("hip_complex", None, ()), ("hip_complex", False, ()),
    ("hip_complex", True, (("hip_complex.score_dtype", "bfloat16"),)),
    ("hip_complex", True, (("hip_complex.entity_embedder.dropout", 0.2),)),
    ("hip_complex", True, (("lookup_embedder.dim", 12),)),
    ("hip_distmult", False, (("KvsAll.label_smoothing", 0.4), ("train.loss", "bce"))),
])
def test_every_other_configuration_keeps_the_composed_route(tmp_path, monkeypatch, model, option, extra):
    """Option off or absent, `score_dtype: bfloat16`, embedder dropout in training, a dimension the kernel does not take:
    one score_sp / score_po call per query type and the reference's loss, no engine call."""
    job = _job(str(tmp_path), model, option, extra=extra)
    assert job.model._fused_f32_loss is bool(option)
    calls = _instrument(monkeypatch, job.model)
    assert job.model.train()._ce_f32_tables() is None
    pairs = _query_types_per_epoch(job)
    l, _ = _epoch(job)
    assert np.isfinite(l)
    assert calls["kl_fwd"] == calls["bce_fwd"] == calls["kl_bwd"] == calls["bce_bwd"] == 0, calls
    assert calls["score_sp"] + calls["score_po"] == pairs[0] >= len(job.loader), (calls, pairs)


@needs_reference
@pytest.mark.parametrize("loss", ["kl", "bce"])
def test_a_split_that_repeats_a_triple_declines_before_any_backward(tmp_path, monkeypatch, loss):
    """A repeated training triple is a repeated id in a label row (a 2 in the reference's dense labels); the fused
    entries take unique ids, so the batch takes the reference's path: no fused function entered, the option-off loss."""
    res = {}
    for option in (True, False):
        job = _job(str(tmp_path), "hip_complex", option, loss=loss, repeat_a_triple=True)
        calls = _instrument(monkeypatch, job.model)
        assert (job.model.train()._ce_f32_tables() is not None) == option   # (the tables qualify: the batch declines)
        res[option] = _epoch(job)[0]
        assert len(job.loader) == 1   # (five training triples: every batch holds the repeat)
        assert calls["kl_fwd"] == calls["bce_fwd"] == calls["kl_bwd"] == calls["bce_bwd"] == 0, calls
        assert calls["score_sp"] + calls["score_po"] >= 1
        monkeypatch.undo()
    assert res[True] == res[False]


@needs_reference
def test_without_a_device_the_option_declines_and_values_are_those_of_the_option_off(tmp_path):
    """job.device: cpu with the option on and NO stand-in: `_fused()` declines, the reference's path runs."""
    res = {}
    for option in (True, False):
        job = _job(str(tmp_path), "hip_complex", option, smoothing=0.4)
        assert job.model._fused_f32_loss is option and job.model._ce_f32_tables() is None
        z = torch.zeros(2, dtype=torch.long)
        assert job.model.kl_loss_sp(z, z, torch.arange(3), z, 0.4) is None
        assert job.model.bce_loss_po(z, z, torch.arange(3), z) is None
        res[option] = _epoch(job)
    assert res[True][0] == res[False][0]
    assert all(torch.equal(res[True][1][k], res[False][1][k]) for k in res[False][1])


@needs_reference
def test_reciprocal_wrapper_forwards_the_option_to_its_base_model(tmp_path, monkeypatch):
    """hip_reciprocal_relations_model over hip_complex: the job sets the option on the base model; both query types are
    sp_ queries of the base model's kl_loss_sp (label smoothing on), no score_* call; the option-off loss."""
    off = _job(str(tmp_path), "hip_reciprocal_relations_model", False, base="hip_complex", smoothing=0.4)
    l_off, _ = _epoch(off)
    job = _job(str(tmp_path), "hip_reciprocal_relations_model", True, base="hip_complex", smoothing=0.4)
    base = job.model._base_model
    assert base._fused_f32_loss is True and job.model._ce_f32_tables() is None   # (cpu: the real decision)
    calls = _instrument(monkeypatch, base)
    assert job.model._ce_f32_tables() is not None
    pairs = _query_types_per_epoch(job)
    l_on, _ = _epoch(job)
    assert calls["kl_fwd"] == calls["kl_bwd"] == pairs[0] >= len(job.loader) and calls["directions"] == {"sp"}, calls
    assert calls["bias"] == pairs[0] and calls["score_sp"] == calls["score_po"] == 0, calls
    assert abs(l_on - l_off) <= 1e-5 * max(1.0, abs(l_off)), (l_on, l_off)
