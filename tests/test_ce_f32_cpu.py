"""Fused 1vsAll loss of float32 ComplEx / DistMult (kge_ce_f32_*) without a GPU: the declarations, the argument checks
of the C entries and of the engine, the float64 reference of the chunked backward against torch autograd, and the control
flow of hip_1vsAll with `fused_f32_loss` (stand-ins for the engine calls; the models' and the job's own code runs)."""
import ctypes
import os
import re
import shutil
import types

import numpy as np
import pytest
import torch

import _ce_f32_ref as ref
import ref_harness as rh
import torch_port as tp
from conftest import ROOT

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")
ENTRIES = ("kge_ce_f32_workspace_bytes", "kge_ce_f32_fwd", "kge_ce_f32_bwd")


def test_entries_are_declared_documented_and_exported():
    from kge_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    _lib.build()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.M), name
    doc = header[header.index("kge_ce_f32_fwd / kge_ce_f32_bwd"):header.index("int64_t kge_ce_f32_workspace_bytes")]
    for name in ENTRIES:  # each entry cites the reference's lines
        assert re.search(name + r"[^\n]*\(train_1vsAll\.py:64-81, loss\.py:192-207", doc), name
    for cite in ("complex.py:30-39", "distmult.py:15-21", "KGE_ERR_WORKSPACE", "KGE_ERR_UNSUPPORTED"):
        assert cite in doc, cite
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
    ws = lambda t, n, c: lib.kge_ce_f32_workspace_bytes(ctypes.byref(t), n, c)
    al = lambda b: -(-b // 256) * 256
    # records (8 column groups of 128) | dQ | Q | split-K partials (at most 32, at most 8 MB) | G [n, chunk]
    nd = 100 * 32 * 4
    assert ws(cx, 100, 128) == al(100 * 3 * 4 * 8) + 2 * al(nd) + al(32 * nd) + 100 * 128 * 4
    assert ws(cx, 100, 0) == ws(cx, 100, 1024) == ws(cx, 100, 1 << 20)   # clamped to E rounded up to 128
    assert ws(cx, 100, 128) < ws(cx, 100, 256) < ws(cx, 100, 0)
    assert ws(dm, 100, 0) == ws(cx, 100, 0) and ws(mk(0, 0, 32, ld=36), 100, 0) > 0
    assert ws(cx, 100, 64) == 0 and ws(cx, 100, -128) == 0 and ws(cx, 0, 0) == 0
    # bf16, TransE, RotatE, dim % 8, a row pitch or a base off 16 bytes
    for t in (mk(1, 0), mk(1, 1), mk(0, 2), mk(0, 3, 32, 16), mk(0, 0, 36), mk(0, 1, 12), mk(0, 0, 32, ld=33),
              mk(0, 0, ent=ctypes.c_void_p(260))):
        assert ws(t, 100, 0) == 0
        assert lib.kge_ce_f32_fwd(ctypes.byref(t), 1, good, good, good, 4, P, P, P, 1 << 20, None) == -2
        assert lib.kge_ce_f32_bwd(ctypes.byref(t), 1, good, good, good, 4, P, None, 1.0, P, P, P, P, 1 << 20, None) == -2
    fwd = lambda t=cx, dirc=1, a=good, n=4, out=P, w=P, wb=1 << 20: lib.kge_ce_f32_fwd(
        ctypes.byref(t), dirc, a, good, good, n, out, out, w, wb, None)
    bwd = lambda t=cx, dirc=1, a=good, n=4, lse=P, gt=P, w=P, wb=1 << 20: lib.kge_ce_f32_bwd(
        ctypes.byref(t), dirc, a, good, good, n, lse, None, 1.0, P, P, gt, w, wb, None)
    for call in (fwd, bwd):
        assert call(dirc=0) == -1 and call(dirc=3) == -1
        assert call(n=-1) == -1
        assert call(a=null) == -1
        assert call(w=None) == -5 and call(wb=64) == -5
        assert call(w=ctypes.c_void_p(264)) == -5   # not on 256 bytes
    assert lib.kge_ce_f32_fwd(None, 1, good, good, good, 4, P, P, P, 1 << 20, None) == -1
    assert fwd(out=None) == -1 and bwd(lse=None) == -1 and bwd(gt=None) == -1
    assert fwd(n=0, a=null, out=None, w=None, wb=0) == 0   # empty batch: nothing to do, no workspace needed
    assert bwd(wb=ws(cx, 4, 128) - 1) == -5                # the backward's minimum: the fixed part and 128 columns
    # the bf16 entries keep declining float32 tables
    assert lib.kge_ce_workspace_bytes(ctypes.byref(cx), 4) == 0


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
    lse = torch.zeros(4)
    for call in (lambda t, a, **k: engine.ce_f32_fwd(t, "sp", a, ix4, ix4, **k),
                 lambda t, a, **k: engine.ce_f32_bwd(t, "sp", a, ix4, ix4, lse, **k)):
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
        with pytest.raises(RuntimeError, match="no CPU path"):   # valid arguments: the product path has no CPU fallback
            call(_cpu_tables("distmult"), ix4, chunk_cols=256)
    with pytest.raises(ValueError, match="one entry per row"):
        engine.ce_f32_bwd(_cpu_tables("complex"), "sp", ix4, ix4, ix4, torch.zeros(3))
    assert not engine.ce_f32_supported(_cpu_tables("complex"))


@pytest.mark.parametrize("name", ["complex", "distmult"])
@pytest.mark.parametrize("direction", ["sp", "po"])
def test_chunked_reference_equals_torch_autograd(name, direction):
    """The float64 reference the GPU tests compare against: loss rows, lse and the three gradients of the chunked
    backward (chunk widths 128, 256, the whole table) equal cross_entropy autograd on the ported scorer to 1e-12."""
    rng = np.random.default_rng(3)
    E, R, d, n = 300, 4, 16, 21
    ent, rel = rng.standard_normal((E, d)), rng.standard_normal((R, d))
    a, p, label = rng.integers(0, E, n), rng.integers(0, R, n), rng.integers(0, E, n)
    label[:4] = (0, E - 1, 127, 128)
    a[5] = a[6]
    g = rng.uniform(0.1, 1.0, n)
    e64, r64 = torch.from_numpy(ent).requires_grad_(), torch.from_numpy(rel).requires_grad_()
    ai, pi = torch.from_numpy(a), torch.from_numpy(p)
    ea, rp = e64[ai], r64[pi]
    ea.retain_grad(), rp.retain_grad()
    sc = tp.score_emb(name, ea, rp, e64, "sp_") if direction == "sp" else tp.score_emb(name, e64, rp, ea, "_po")
    rows = torch.nn.functional.cross_entropy(sc, torch.from_numpy(label), reduction="none")
    (rows * torch.from_numpy(g)).sum().backward()
    loss, lse = ref.forward(name, direction, ent, rel, a, p, label)
    assert np.abs(loss - rows.detach().numpy()).max() <= 1e-12
    assert np.abs(lse - torch.logsumexp(sc, 1).detach().numpy()).max() <= 1e-12
    # autograd's table gradient = the dense target gradient + the scattered query rows
    for cc in (128, 256, 0):
        g_a, g_p, g_t = ref.chunked_backward(name, direction, ent, rel, a, p, label, g, cc)
        assert not np.isnan(g_t).any()
        ge = g_t.copy()
        np.add.at(ge, a, g_a)
        gr = np.zeros_like(rel)
        np.add.at(gr, p, g_p)
        for nm, got, want in (("g_a", g_a, ea.grad), ("g_p", g_p, rp.grad), ("entity", ge, e64.grad), ("relation", gr, r64.grad)):
            err = np.abs(got - want.numpy()).max()
            assert err <= 1e-12, (cc, nm, err)


@pytest.mark.parametrize("name", ["complex", "distmult"])
def test_model_declines_to_the_composed_loss_on_cpu(name, monkeypatch):
    from kge_amd import model as km
    m = km.create(name, 30, 4, 8, fused_f32_loss=True)
    assert m.fused_f32_loss and m._ce_f32_tables() is None
    assert not km.create(name, 30, 4, 8).fused_f32_loss
    g = torch.Generator().manual_seed(0)
    s, p, o = (torch.randint(hi, (6,), generator=g) for hi in (30, 4, 30))
    sc_sp, sc_po = torch.randn(6, 30, generator=g), torch.randn(6, 30, generator=g)
    monkeypatch.setattr(m, "score_sp", lambda s_, p_, o_=None: sc_sp)
    monkeypatch.setattr(m, "score_po", lambda p_, o_, s_=None: sc_po)
    ce = torch.nn.functional.cross_entropy
    assert torch.equal(m.loss_sp(s, p, o), ce(sc_sp, o, reduction="none"))
    assert torch.equal(m.loss_po(p, o, s), ce(sc_po, s, reduction="none"))


# ---- the plugin's control flow ------------------------------------------------------------------------------------------
def _job(tmp, model, option, base=None, extra=()):
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    data = os.path.join(tmp, "dataset_test")
    if not os.path.isdir(data):
        shutil.copytree(os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"), data)
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
    config.set("lookup_embedder.dim", 16)
    config.set("random_seed.default", 7)
    config._import("hip_1vsAll")
    config.set("train.type", "hip_1vsAll")
    if option is not None:
        config.set("hip_1vsAll.fused_f32_loss", option)
    for k, v in extra:
        config.set(k, v)
    torch.manual_seed(21)
    return TrainingJob.create(config, Dataset.create(config, folder=data))


class _Tables:
    """stand-in for engine.Tables (which refuses CPU tensors)"""

    def __init__(self, name, ent, rel, l_norm=1.0, flags=0):
        self.name, self.ent, self.rel = name, ent, rel


def _instrument(monkeypatch, target):
    """There is no HIP device here.  Stand-ins: engine.Tables / ce_f32_supported / ce_f32_fwd / ce_f32_bwd (float64
    numpy of tests/_ce_f32_ref.py), and the ONE device question of the model's decision -- `_fused()` asks whether the
    parameters are on a GPU -- answered as if they were, inside `_ce_f32_tables()` only.  Everything else is the
    project's code: the job's routing, _ce_tables / _dropout_only / _ce_f32_tables, loss_sp / loss_po, _FusedCEF32.
    score_sp / score_po count and go on to the composed path."""
    from kge.model import LookupEmbedder
    from kge_amd import engine
    calls = {"fwd": 0, "bwd": 0, "score_sp": 0, "score_po": 0}
    npy = lambda x: x.detach().cpu().numpy()

    def fwd(t, direction, a, p, label, chunk_cols=0):
        calls["fwd"] += 1
        loss, lse = ref.forward(t.name, direction, npy(t.ent), npy(t.rel), npy(a), npy(p), npy(label))
        return torch.from_numpy(loss).float(), torch.from_numpy(lse).float()

    def bwd(t, direction, a, p, label, lse, g_rows=None, g_scalar=1.0, chunk_cols=0):
        calls["bwd"] += 1
        out = ref.chunked_backward(t.name, direction, npy(t.ent), npy(t.rel), npy(a), npy(p), npy(label), npy(g_rows), 128)
        return tuple(torch.from_numpy(x).float() for x in out)

    monkeypatch.setattr(engine, "Tables", _Tables)
    monkeypatch.setattr(engine, "ce_f32_supported", lambda t: t.ent.dtype == torch.float32 and t.ent.shape[1] % 8 == 0)
    monkeypatch.setattr(engine, "ce_f32_fwd", fwd)
    monkeypatch.setattr(engine, "ce_f32_bwd", bwd)

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


@needs_reference
@pytest.mark.parametrize("model", ["hip_complex", "hip_distmult"])
def test_fused_f32_loss_routes_a_float32_job_through_the_fused_function(tmp_path, monkeypatch, model):
    """hip_1vsAll.fused_f32_loss: true -- every subbatch of a float32 hip_complex / hip_distmult job goes loss_sp, then
    loss_po -> _FusedCEF32 (one engine forward and one engine backward each) and never score_sp / score_po; the epoch's
    avg_loss and the parameters after it are those of the composed path."""
    from kge_amd.model import _FusedCEF32
    seen = []
    real_apply = _FusedCEF32.apply
    monkeypatch.setattr(_FusedCEF32, "apply", lambda direction, *a: (seen.append(direction), real_apply(direction, *a))[1])
    job = _job(str(tmp_path), model, True)
    assert type(job).__name__ == "HipTrainingJob1vsAll" and job.model._fused_f32_loss is True
    calls = _instrument(monkeypatch, job.model)
    job._prepare()
    trace = job.run_epoch()
    batches = len(job.loader)
    assert calls == {"fwd": 2 * batches, "bwd": 2 * batches, "score_sp": 0, "score_po": 0}, calls
    assert seen == ["sp", "po"] * batches
    monkeypatch.undo()
    plain = _job(str(tmp_path), model, None)
    assert plain.model._fused_f32_loss is False
    plain._prepare()
    want = plain.run_epoch()
    assert abs(trace["avg_loss"] - want["avg_loss"]) <= 1e-5 * max(1.0, abs(want["avg_loss"]))
    for (k, x), (_, y) in zip(job.model.state_dict().items(), plain.model.state_dict().items()):
        assert torch.allclose(x, y, rtol=1e-4, atol=1e-6), k


@needs_reference
@pytest.mark.parametrize("model,option,extra", [
    ("hip_complex", None, ()), ("hip_complex", False, ()),
    ("hip_complex", True, (("hip_complex.score_dtype", "bfloat16"),)),
    ("hip_complex", True, (("hip_complex.entity_embedder.dropout", 0.2),)),
    ("hip_complex", True, (("lookup_embedder.dim", 12),)),
    ("hip_complex", True, (("train.loss", "bce"),)),
    ("hip_transe", True, ()),
])
def test_every_other_configuration_keeps_its_route(tmp_path, monkeypatch, model, option, extra):
    """Option off or absent, `score_dtype: bfloat16`, embedder dropout in training, a dimension the kernel does not take,
    another loss, another scorer: score_sp / score_po and the reference's loss once per batch each, no engine call."""
    job = _job(str(tmp_path), model, option, extra=extra)
    assert job.model._fused_f32_loss is bool(option) if model == "hip_complex" else True
    calls = _instrument(monkeypatch, job.model) if hasattr(type(job.model), "_ce_f32_tables") else None
    if model == "hip_complex" and ("train.loss", "bce") not in extra:  # (bce: the tables qualify, the job does not ask)
        assert job.model.train()._ce_f32_tables() is None
    job._prepare()
    assert np.isfinite(job.run_epoch()["avg_loss"])
    batches = len(job.loader)
    assert calls == {"fwd": 0, "bwd": 0, "score_sp": batches, "score_po": batches}, calls


@needs_reference
def test_without_a_device_the_option_declines_to_the_composed_path(tmp_path):
    """job.device: cpu with the option on and NO stand-in: `_fused()` declines, the reference's path runs."""
    job = _job(str(tmp_path), "hip_complex", True)
    assert job.model._fused_f32_loss is True and job.model._ce_f32_tables() is None
    z = torch.zeros(2, dtype=torch.long)
    assert job.model.loss_sp(z, z, z) is None and job.model.loss_sp_po(z, z, z) is None
    job._prepare()
    assert np.isfinite(job.run_epoch()["avg_loss"])


@needs_reference
def test_reciprocal_wrapper_forwards_the_option_to_its_base_model(tmp_path, monkeypatch):
    """hip_reciprocal_relations_model over hip_complex: the job sets the option on the base model, the wrapper's
    loss_sp / loss_po are two sp_ queries of the base model's loss_sp, no score_* call."""
    from kge_amd.model import _FusedCEF32
    seen = []
    real_apply = _FusedCEF32.apply
    monkeypatch.setattr(_FusedCEF32, "apply", lambda direction, *a: (seen.append(direction), real_apply(direction, *a))[1])
    job = _job(str(tmp_path), "hip_reciprocal_relations_model", True, base="hip_complex")
    base = job.model._base_model
    assert base._fused_f32_loss is True
    calls = _instrument(monkeypatch, base)
    job._prepare()
    assert np.isfinite(job.run_epoch()["avg_loss"])
    batches = len(job.loader)
    assert calls == {"fwd": 2 * batches, "bwd": 2 * batches, "score_sp": 0, "score_po": 0}, calls
    assert seen == ["sp", "sp"] * batches
