"""Fused 1vsAll loss of TransE / RotatE (kge_ce_dist_*) without a GPU: the declarations, the argument checks of the C
entries and of the engine, the control flow of hip_1vsAll with `fused_dist_loss` (stand-ins for the fused autograd
function), and the model's decline to the composed loss on CPU tensors."""
import ctypes
import os
import re
import shutil
import types

import pytest
import torch

import ref_harness as rh
from conftest import ROOT

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")
ENTRIES = ("kge_ce_dist_workspace_bytes", "kge_ce_dist_fwd", "kge_ce_dist_bwd")


def test_entries_are_declared_documented_and_exported():
    from kge_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    _lib.build()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.M), name
    doc = header[header.index("kge_ce_dist_fwd / kge_ce_dist_bwd"):header.index("int64_t kge_ce_dist_workspace_bytes")]
    for cite in ("train_1vsAll.py:64-81", "loss.py:192-207", "transe.py:18-34", "rotate.py:30-64", "KGE_ERR_WORKSPACE",
                 "KGE_ERR_UNSUPPORTED"):
        assert cite in doc, cite
    assert lib.kge_abi_version() == 1


def test_c_entries_validate_arguments_without_a_device():
    from kge_amd import _lib
    from kge_amd._lib import KgeIndex, KgeTables
    _lib.build()
    lib = _lib.lib()
    P = ctypes.c_void_p(256)  # never dereferenced on these paths
    good, null = KgeIndex(P, 1, 0, 1), KgeIndex(None, 1, 0, 1)
    mk = lambda dtype, scorer, d=32, dr=32, l_norm=1.0: KgeTables(P, P, dtype, scorer, 1000, 3, d, dr, d, dr, l_norm, 0)
    transe, rotate = mk(0, 2), mk(0, 3, 32, 16, 2.0)
    ws = lambda t, n, c: lib.kge_ce_dist_workspace_bytes(ctypes.byref(t), n, c)
    # sizes: records + [n, dim] + [n, chunk] floats, each part on 256 bytes; default = at most 32 MB of scores,
    # clamped to E rounded up to 64
    assert ws(transe, 100, 64) == 256 * -(-100 * 3 * 4 * 16 // 256) + 256 * -(-100 * 32 * 4 // 256) + 100 * 64 * 4
    assert ws(transe, 100, 0) == ws(transe, 100, 1024) == ws(transe, 100, 1 << 20)
    assert ws(transe, 100, 64) < ws(transe, 100, 128) < ws(transe, 100, 0)
    assert ws(rotate, 100, 0) > 0
    assert ws(transe, 100, 65) == 0 and ws(transe, 100, -64) == 0 and ws(transe, 0, 0) == 0
    for t in (mk(1, 2), mk(0, 0), mk(0, 1), mk(0, 2, l_norm=3.0)):   # bf16, ComplEx, DistMult, general p
        assert ws(t, 100, 0) == 0
        assert lib.kge_ce_dist_fwd(ctypes.byref(t), 1, good, good, good, 4, P, P, P, 1 << 20, None) == -2
        assert lib.kge_ce_dist_bwd(ctypes.byref(t), 1, good, good, good, 4, P, None, 1.0, P, P, P, P, 1 << 20, None) == -2
    fwd = lambda t=transe, dirc=1, a=good, n=4, out=P, w=P, wb=1 << 20: lib.kge_ce_dist_fwd(
        ctypes.byref(t), dirc, a, good, good, n, out, out, w, wb, None)
    bwd = lambda t=transe, dirc=1, a=good, n=4, lse=P, gt=P, w=P, wb=1 << 20: lib.kge_ce_dist_bwd(
        ctypes.byref(t), dirc, a, good, good, n, lse, None, 1.0, P, P, gt, w, wb, None)
    for call in (fwd, bwd):
        assert call(dirc=0) == -1 and call(dirc=3) == -1
        assert call(n=-1) == -1
        assert call(a=null) == -1
        assert call(w=None) == -5 and call(wb=64) == -5
        assert call(w=ctypes.c_void_p(264)) == -5   # not on 256 bytes
    assert lib.kge_ce_dist_fwd(None, 1, good, good, good, 4, P, P, P, 1 << 20, None) == -1
    assert fwd(out=None) == -1 and bwd(lse=None) == -1 and bwd(gt=None) == -1
    assert fwd(n=0, a=null, out=None, w=None, wb=0) == 0   # empty batch: nothing to do, no workspace needed
    # the backward's minimum: the records, the [n, dim] buffer and 64 columns
    assert bwd(wb=ws(transe, 4, 64) - 1) == -5
    # the existing entries keep declining these tables
    assert lib.kge_ce_workspace_bytes(ctypes.byref(transe), 4) == 0
    assert lib.kge_ce_fwd(ctypes.byref(transe), 1, good, good, good, 4, P, P, P, 1 << 20, None) == -2


def _cpu_tables(scorer, dtype=torch.float32, l_norm=1.0):
    """engine.Tables refuses CPU tensors in its constructor; the checks under test come before any device is asked."""
    from kge_amd import engine
    t = engine.Tables.__new__(engine.Tables)
    t.scorer = engine.SCORERS[scorer]
    t.ent, t.rel = torch.zeros(10, 8, dtype=dtype), torch.zeros(3, 8, dtype=dtype)
    t.l_norm, t.flags, t.device, t._c_cache = l_norm, 0, t.ent.device, {}
    return t


def test_engine_refuses_bad_arguments_with_the_usual_exceptions():
    from kge_amd import engine
    ix4, ix5 = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    lse = torch.zeros(4)
    for call in (lambda t, a, **k: engine.ce_dist_fwd(t, "sp", a, ix4, ix4, **k),
                 lambda t, a, **k: engine.ce_dist_bwd(t, "sp", a, ix4, ix4, lse, **k)):
        with pytest.raises(ValueError, match="different lengths"):
            call(_cpu_tables("transe"), ix5)
        for cc in (65, 32, -64):
            with pytest.raises(ValueError, match="multiple of 64"):
                call(_cpu_tables("transe"), ix4, chunk_cols=cc)
        for bad in (_cpu_tables("transe", torch.bfloat16), _cpu_tables("complex"), _cpu_tables("distmult"),
                    _cpu_tables("rotate", l_norm=3.0)):
            with pytest.raises(RuntimeError, match="TransE / RotatE on float32"):
                call(bad, ix4)
        with pytest.raises(RuntimeError, match="no CPU path"):   # valid arguments: the product path has no CPU fallback
            call(_cpu_tables("rotate", l_norm=2.0), ix4, chunk_cols=128)
    assert not engine.ce_dist_supported(_cpu_tables("transe"))


@pytest.mark.parametrize("name", ["transe", "rotate"])
def test_model_declines_to_the_composed_loss_on_cpu(name, monkeypatch):
    """kge_amd.model.create(..., fused_dist_loss=True) on CPU parameters: the composed loss, value for value.  (The
    composed score itself has no CPU path: score_sp is replaced by a recorded stand-in, and the loss must be exactly
    cross_entropy of what it returned.)"""
    from kge_amd import model as km
    m = km.create(name, 30, 4, 8, fused_dist_loss=True)
    assert m.fused_dist_loss and m._ce_dist_tables() is None
    assert not km.create(name, 30, 4, 8).fused_dist_loss
    g = torch.Generator().manual_seed(0)
    s, p, o = (torch.randint(hi, (6,), generator=g) for hi in (30, 4, 30))
    sc_sp, sc_po = torch.randn(6, 30, generator=g), torch.randn(6, 30, generator=g)
    monkeypatch.setattr(m, "score_sp", lambda s_, p_, o_=None: sc_sp)
    monkeypatch.setattr(m, "score_po", lambda p_, o_, s_=None: sc_po)
    ce = torch.nn.functional.cross_entropy
    assert torch.equal(m.loss_sp(s, p, o), ce(sc_sp, o, reduction="none"))
    assert torch.equal(m.loss_po(p, o, s), ce(sc_po, s, reduction="none"))
    assert torch.equal(m.loss_sp_po(s, p, o), torch.cat([ce(sc_sp, o, reduction="none"), ce(sc_po, s, reduction="none")]))
    assert torch.equal(m.loss_sp_po_sum(s, p, o, 0.5), m.loss_sp_po(s, p, o).sum() * 0.5)


def _job(tmp, model, option, base=None):
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    data = os.path.join(tmp, "dataset_test")
    if not os.path.isdir(data):
        shutil.copytree(os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"), data)
    config = Config()
    config.folder = os.path.join(tmp, f"run_{model}_{option}")
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
        config.set("hip_1vsAll.fused_dist_loss", option)
    torch.manual_seed(21)
    return TrainingJob.create(config, Dataset.create(config, folder=data))


def _instrument(job, target):
    """Stand-ins on `target` (the model that scores): loss_sp / loss_po compute the reference's arithmetic from the
    embedders (no score_sp / score_po call) and count; score_sp / score_po count and go on; `_ce_dist_tables` says the
    tables qualify iff the job switched the model's option on (there is no HIP device here)."""
    from kge.model.kge_model import KgeModel
    calls = {"loss_sp": 0, "loss_po": 0, "score_sp": 0, "score_po": 0}
    ce = torch.nn.functional.cross_entropy

    def loss_sp(self, s, p, o):
        calls["loss_sp"] += 1
        sc = self._scorer.score_emb(self.get_s_embedder().embed(s), self.get_p_embedder().embed(p),
                                    self.get_o_embedder().embed_all(), combine="sp_")
        return ce(sc, o.long(), reduction="none")

    def loss_po(self, p, o, s):
        calls["loss_po"] += 1
        sc = self._scorer.score_emb(self.get_s_embedder().embed_all(), self.get_p_embedder().embed(p),
                                    self.get_o_embedder().embed(o), combine="_po")
        return ce(sc, s.long(), reduction="none")

    def score_sp(self, s, p, o=None):
        calls["score_sp"] += 1
        return KgeModel.score_sp(self, s, p, o)

    def score_po(self, p, o, s=None):
        calls["score_po"] += 1
        return KgeModel.score_po(self, p, o, s)

    for nm, f in (("loss_sp", loss_sp), ("loss_po", loss_po), ("score_sp", score_sp), ("score_po", score_po)):
        setattr(target, nm, types.MethodType(f, target))
    target._ce_dist_tables = types.MethodType(lambda self: object() if self._fused_dist_loss else None, target)
    return calls


@needs_reference
@pytest.mark.parametrize("option", [None, False, True])
def test_fused_dist_loss_is_the_switch_of_the_hip_transe_job(tmp_path, option):
    """hip_1vsAll.fused_dist_loss: true -- every subbatch of a hip_transe job asks loss_sp and loss_po and never
    score_sp / score_po; false or absent -- today's path: score_sp / score_po and the reference's loss, no loss_* call.
    The epoch's avg_loss is the same either way (the stand-ins compute the reference's arithmetic)."""
    job = _job(str(tmp_path), "hip_transe", option)
    assert type(job).__name__ == "HipTrainingJob1vsAll"
    assert job.model._fused_dist_loss is bool(option)
    calls = _instrument(job, job.model)
    job._prepare()
    trace = job.run_epoch()
    batches = len(job.loader)
    if option:
        assert calls == {"loss_sp": batches, "loss_po": batches, "score_sp": 0, "score_po": 0}, calls
    else:
        assert calls == {"loss_sp": 0, "loss_po": 0, "score_sp": batches, "score_po": batches}, calls
    plain = _job(str(tmp_path), "hip_transe", None)
    plain._prepare()
    want = plain.run_epoch()["avg_loss"]
    assert abs(trace["avg_loss"] - want) <= 1e-6 * max(1.0, abs(want)), (trace["avg_loss"], want)


@needs_reference
def test_without_a_device_the_option_declines_to_the_composed_path(tmp_path):
    """job.device: cpu with the option on and NO stand-in: `_fused()` declines, the reference's path runs."""
    job = _job(str(tmp_path), "hip_rotate", True)
    assert job.model._fused_dist_loss is True and job.model._ce_dist_tables() is None
    assert job.model.loss_sp(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long),
                             torch.zeros(2, dtype=torch.long)) is None
    job._prepare()
    assert torch.isfinite(torch.tensor(job.run_epoch()["avg_loss"]))


@needs_reference
@pytest.mark.parametrize("option", [False, True])
def test_hip_complex_is_unaffected(tmp_path, option):
    job = _job(str(tmp_path), "hip_complex", option)
    calls = _instrument(job, job.model)
    job.model._ce_dist_tables = types.MethodType(type(job.model)._ce_dist_tables, job.model)  # the real decision
    assert job.model._ce_dist_tables() is None
    job._prepare()
    job.run_epoch()
    assert calls["loss_sp"] == calls["loss_po"] == 0 and calls["score_sp"] == calls["score_po"] == len(job.loader), calls


@needs_reference
def test_reciprocal_wrapper_forwards_the_option_to_its_base_model(tmp_path):
    """hip_reciprocal_relations_model over hip_transe: the job sets the option on the base model, the wrapper's
    loss_sp / loss_po are two sp_ queries of the base model's loss_sp, no score_* call."""
    job = _job(str(tmp_path), "hip_reciprocal_relations_model", True, base="hip_transe")
    base = job.model._base_model
    assert base._fused_dist_loss is True
    calls = _instrument(job, base)
    job._prepare()
    job.run_epoch()
    assert calls == {"loss_sp": 2 * len(job.loader), "loss_po": 0, "score_sp": 0, "score_po": 0}, calls
