"""KvsAll kl / bce losses of TransE / RotatE without a score matrix (kge_kl_dist_* / kge_bce_dist_*) without a GPU: the
declarations, the argument checks of the C entries and of the engine, the decline to the composed loss on CPU tensors,
and the control flow of hip_KvsAll (and hip_1vsAll with train.loss: bce) with `fused_dist_loss`: the real hooks and
autograd functions over CPU stand-ins of the engine functions built on torch_port."""
import ctypes
import os
import re
import shutil
import types

import pytest
import torch

import ref_harness as rh
import torch_port as tp
from conftest import ROOT

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")
ENTRIES = ("kge_multilabel_dist_workspace_bytes", "kge_kl_dist_fwd", "kge_kl_dist_bwd", "kge_bce_dist_fwd",
           "kge_bce_dist_bwd")


def test_entries_are_declared_documented_exported_and_bound():
    from kge_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    _lib.build()
    lib = _lib.lib()
    for name in ENTRIES:
        assert name in _lib.PROTOTYPES and hasattr(lib, name)
        assert re.search(r"^(?:int|int64_t)\s+" + name + r"\s*\(", header, flags=re.M), name
    doc = header[header.index("kge_kl_dist_fwd / _bwd and kge_bce_dist_fwd / _bwd"):
                 header.index("int64_t kge_multilabel_dist_workspace_bytes")]
    for cite in ("train_KvsAll.py:216-294", "loss.py:137-159", "loss.py:192-213", "KGE_ERR_WORKSPACE",
                 "KGE_ERR_UNSUPPORTED", "ANY\n * order"):
        assert cite in doc, cite
    ext = _lib.ext()
    for name in ("multilabel_dist_workspace_bytes", "kl_dist_fwd", "kl_dist_bwd", "bce_dist_fwd", "bce_dist_bwd"):
        assert hasattr(ext, name), name
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
    ws = lambda t, n, c: lib.kge_multilabel_dist_workspace_bytes(ctypes.byref(t), n, c)
    al = lambda b: 256 * -(-b // 256)
    # records + [n, dim] + [n, chunk] floats + n x chunk bits, each part on 256 bytes
    assert ws(transe, 100, 64) == al(100 * 3 * 4 * 16) + al(100 * 32 * 4) + al(100 * 64 * 4) + al(100 * 64 // 8)
    assert ws(transe, 100, 64) == lib.kge_ce_dist_workspace_bytes(ctypes.byref(transe), 100, 64) + al(100 * 64 // 8)
    assert ws(transe, 100, 0) == ws(transe, 100, 1024) == ws(transe, 100, 1 << 20)
    assert ws(transe, 100, 64) < ws(transe, 100, 128) < ws(transe, 100, 0)
    assert ws(rotate, 100, 0) > 0
    assert ws(transe, 100, 65) == 0 and ws(transe, 100, -64) == 0 and ws(transe, 0, 0) == 0
    kl_f = lambda t=transe, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_kl_dist_fwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, None, out, out, w, wb, None)
    kl_b = lambda t=transe, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_kl_dist_bwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, None, P, None, 1.0, P, P, out, w, wb, None)
    bce_f = lambda t=transe, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_bce_dist_fwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, 0.5, out, w, wb, None)
    bce_b = lambda t=transe, dirc=1, a=good, n=4, rp=P, out=P, w=P, wb=1 << 20: lib.kge_bce_dist_bwd(
        ctypes.byref(t), dirc, a, good, n, rp, P, 0.5, None, 1.0, P, P, out, w, wb, None)
    for t in (mk(1, 2), mk(0, 0), mk(0, 1), mk(0, 2, l_norm=3.0)):   # bf16, ComplEx, DistMult, general p
        assert ws(t, 100, 0) == 0
        for call in (kl_f, kl_b, bce_f, bce_b):
            assert call(t=t) == -2
    for call in (kl_f, kl_b, bce_f, bce_b):
        assert call(dirc=0) == -1 and call(dirc=3) == -1
        assert call(n=-1) == -1
        assert call(a=null) == -1
        assert call(rp=None) == -1            # no label CSR
        assert call(out=None) == -1           # loss_rows / lse, g_tgt
        assert call(w=None) == -5 and call(wb=64) == -5
        assert call(w=ctypes.c_void_p(264)) == -5   # not on 256 bytes
    assert lib.kge_kl_dist_fwd(None, 1, good, good, 4, P, P, None, P, P, P, 1 << 20, None) == -1
    assert lib.kge_kl_dist_bwd(ctypes.byref(transe), 1, good, good, 4, P, P, None, None, None, 1.0, P, P, P, P, 1 << 20,
                               None) == -1   # no lse
    # empty batch: nothing to do for the forward, no CSR, no outputs, no workspace needed
    assert kl_f(n=0, a=null, rp=None, out=None, w=None, wb=0) == 0
    assert bce_f(n=0, a=null, rp=None, out=None, w=None, wb=0) == 0
    # the backward's minimum: the records, the [n, dim] buffer, 64 columns of scores and their label bits
    for call in (kl_b, bce_b):
        assert call(wb=ws(transe, 4, 64) - 1) == -5
    # the existing entries keep declining these tables
    assert lib.kge_kl_fwd(ctypes.byref(transe), 1, good, good, 4, P, P, P, P, P, 1 << 20, None) == -2
    assert lib.kge_bce_fwd(ctypes.byref(transe), 1, good, good, 4, P, P, 0.0, P, P, 1 << 20, None) == -2


def _cpu_tables(scorer, dtype=torch.float32, l_norm=1.0, ent=None, rel=None):
    """engine.Tables refuses CPU tensors in its constructor; the checks under test come before any device is asked."""
    from kge_amd import engine
    t = engine.Tables.__new__(engine.Tables)
    t.scorer = engine.SCORERS[scorer]
    t.ent = torch.zeros(10, 8, dtype=dtype) if ent is None else ent
    t.rel = torch.zeros(3, 8, dtype=dtype) if rel is None else rel
    t.l_norm, t.flags, t.device, t._c_cache = l_norm, 0, t.ent.device, {}
    return t


def test_engine_refuses_bad_arguments_with_the_usual_exceptions():
    from kge_amd import engine
    ix4, ix5 = torch.zeros(4, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)
    rp, cl, rows = torch.arange(5), torch.zeros(4, dtype=torch.int64), torch.zeros(4)
    calls = (lambda t, a, rp_=rp, **k: engine.kl_dist_fwd(t, "sp", a, ix4, rp_, cl, **k),
             lambda t, a, rp_=rp, **k: engine.kl_dist_bwd(t, "sp", a, ix4, rp_, cl, rows, **k),
             lambda t, a, rp_=rp, **k: engine.bce_dist_fwd(t, "po", a, ix4, rp_, cl, 0.5, **k),
             lambda t, a, rp_=rp, **k: engine.bce_dist_bwd(t, "po", a, ix4, rp_, cl, 0.5, **k))
    for call in calls:
        with pytest.raises(ValueError, match="different lengths"):
            call(_cpu_tables("transe"), ix5)
        for cc in (65, 32, -64):
            with pytest.raises(ValueError, match="multiple of 64"):
                call(_cpu_tables("transe"), ix4, chunk_cols=cc)
        for bad in (_cpu_tables("transe", torch.bfloat16), _cpu_tables("complex"), _cpu_tables("distmult"),
                    _cpu_tables("rotate", l_norm=3.0)):
            with pytest.raises(RuntimeError, match="TransE / RotatE on float32"):
                call(bad, ix4)
        with pytest.raises(ValueError, match="rowptr has 4 entries for 4 rows"):
            call(_cpu_tables("transe"), ix4, torch.arange(4))
        with pytest.raises(TypeError, match="holds integers"):
            call(_cpu_tables("transe"), ix4, torch.arange(5).float())
        with pytest.raises(RuntimeError, match="no CPU path"):   # valid arguments: the product path has no CPU fallback
            call(_cpu_tables("rotate", l_norm=2.0), ix4, chunk_cols=128)


@pytest.mark.parametrize("name", ["transe", "rotate"])
def test_model_declines_to_the_composed_loss_on_cpu(name, monkeypatch):
    """kge_amd.model.create(..., fused_dist_loss=True) on CPU parameters: the composed losses, value for value (the
    composed score itself has no CPU path: score_sp / score_po are recorded stand-ins)."""
    from kge_amd import model as km
    m = km.create(name, 30, 4, 8, fused_dist_loss=True)
    assert m.fused_dist_loss and m._ce_dist_tables() is None
    g = torch.Generator().manual_seed(0)
    s, p = (torch.randint(hi, (6,), generator=g) for hi in (30, 4))
    rowptr, col = torch.tensor([0, 2, 2, 3, 6, 7, 9]), torch.tensor([5, 1, 0, 29, 3, 17, 8, 2, 11])
    sc_sp, sc_po = torch.randn(6, 30, generator=g), torch.randn(6, 30, generator=g)
    monkeypatch.setattr(m, "score_sp", lambda s_, p_, o_=None: sc_sp)
    monkeypatch.setattr(m, "score_po", lambda p_, o_, s_=None: sc_po)
    for fn in (km._FusedKLDist, km._FusedBCEDist):
        monkeypatch.setattr(fn, "forward", staticmethod(lambda *a, **k: pytest.fail("fused function entered on CPU")))
    assert torch.equal(m.kl_loss_sp(s, p, rowptr, col), km.KgeModel._kl_composed(sc_sp, rowptr, col))
    assert torch.equal(m.kl_loss_po(p, s, rowptr, col), km.KgeModel._kl_composed(sc_po, rowptr, col))
    assert torch.equal(m.bce_loss_sp(s, p, rowptr, col, 1.5), km.KgeModel._bce_composed(sc_sp, rowptr, col, 1.5))
    assert torch.equal(m.bce_loss_po(p, s, rowptr, col, 1.5), km.KgeModel._bce_composed(sc_po, rowptr, col, 1.5))
    both = m.multilabel_loss_sp_po("kl", s, p, rowptr, col, s, p, rowptr, col)
    assert torch.equal(both[0], km.KgeModel._kl_composed(sc_sp, rowptr, col))
    assert torch.equal(both[1], km.KgeModel._kl_composed(sc_po, rowptr, col))


# ---- the jobs through LibKGE's own factory ----------------------------------------------------------------------------
def _job(tmp, model, option, train_type="hip_KvsAll", loss="kl", base=None, smoothing=0.0, repeat_a_triple=False):
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
    config.folder = os.path.join(tmp, f"run_{model}_{train_type}_{loss}_{option}_{smoothing}_{repeat_a_triple}")
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
        config.set(train_type + ".fused_dist_loss", option)
    torch.manual_seed(21)
    return TrainingJob.create(config, Dataset.create(config, folder=data))


def _dense(rowptr, col, n, E, dtype):
    y = torch.zeros(n, E, dtype=dtype)
    y[torch.repeat_interleave(torch.arange(n), rowptr[1:] - rowptr[:-1]), col.long()] = 1.0
    return y


def _instrument(monkeypatch, target):
    """The model that scores (`target`) keeps its REAL hooks (kl_loss_* / bce_loss_* -> _FusedKLDist / _FusedBCEDist); its
    `_ce_dist_tables` says the tables qualify iff the job switched the option on (there is no HIP device here) and hands
    out CPU tables; the four engine functions are CPU stand-ins built on torch_port's op sequence.  score_sp / score_po
    count and go on."""
    from kge.model.kge_model import KgeModel
    from kge_amd import engine
    calls = {"kl_fwd": 0, "kl_bwd": 0, "bce_fwd": 0, "bce_bwd": 0, "score_sp": 0, "score_po": 0, "directions": set()}
    name = {engine.SCORERS["transe"]: "transe", engine.SCORERS["rotate"]: "rotate"}

    def tables(self):
        if not self._fused_dist_loss:
            return None
        ent, rel = self._w()
        return _cpu_tables(self._scorer.name, l_norm=self._scorer._norm, ent=ent.detach(), rel=rel.detach())

    def rows_of(kind, t, direction, A, P, TG, rowptr, col, offset):
        sc = tp.score_emb(name[t.scorer], A, P, TG, "sp_", t.l_norm) if direction == "sp" else \
            tp.score_emb(name[t.scorer], TG, P, A, "_po", t.l_norm)
        y = _dense(rowptr, col, sc.shape[0], sc.shape[1], sc.dtype)
        return (tp.kl_loss(sc, y, "rows") if kind == "kl" else tp.bce_loss(sc, y, offset, "rows")), sc

    def fwd(kind, t, direction, a, p, rowptr, col, offset):
        calls[kind + "_fwd"] += 1
        calls["directions"].add(direction)
        with torch.no_grad():
            rows, sc = rows_of(kind, t, direction, t.ent[a.long()], t.rel[p.long()], t.ent, rowptr, col, offset)
        return rows, torch.logsumexp(sc, dim=1)

    def bwd(kind, t, direction, a, p, rowptr, col, offset, g_rows):
        calls[kind + "_bwd"] += 1
        with torch.enable_grad():
            A, P, TG = (x.detach().clone().requires_grad_() for x in (t.ent[a.long()], t.rel[p.long()], t.ent))
            rows, _ = rows_of(kind, t, direction, A, P, TG, rowptr, col, offset)
            (rows * g_rows).sum().backward()
        return A.grad, P.grad, TG.grad

    monkeypatch.setattr(engine, "kl_dist_fwd", lambda t, direction, a, p, rp, cl, label_weight=None, chunk_cols=0:
                        fwd("kl", t, direction, a, p, rp, cl, 0.0))
    monkeypatch.setattr(engine, "kl_dist_bwd", lambda t, direction, a, p, rp, cl, lse, g_rows=None, g_scalar=1.0,
                        label_weight=None, chunk_cols=0: bwd("kl", t, direction, a, p, rp, cl, 0.0, g_rows))
    monkeypatch.setattr(engine, "bce_dist_fwd", lambda t, direction, a, p, rp, cl, offset=0.0, chunk_cols=0:
                        fwd("bce", t, direction, a, p, rp, cl, offset)[0])
    monkeypatch.setattr(engine, "bce_dist_bwd", lambda t, direction, a, p, rp, cl, offset=0.0, g_rows=None, g_scalar=1.0,
                        chunk_cols=0: bwd("bce", t, direction, a, p, rp, cl, offset, g_rows))

    def score_sp(self, s, p, o=None):
        calls["score_sp"] += 1
        return KgeModel.score_sp(self, s, p, o)

    def score_po(self, p, o, s=None):
        calls["score_po"] += 1
        return KgeModel.score_po(self, p, o, s)

    target.score_sp = types.MethodType(score_sp, target)
    target.score_po = types.MethodType(score_po, target)
    if hasattr(type(target), "_ce_dist_tables"):
        target._ce_dist_tables = types.MethodType(tables, target)
    return calls


def _epoch(job):
    job._prepare()
    trace = job.run_epoch()
    return trace["avg_loss"], {k: v.detach().clone() for k, v in job.model.state_dict().items()}


@needs_reference
@pytest.mark.parametrize("loss", ["kl", "bce"])
@pytest.mark.parametrize("model", ["hip_transe", "hip_rotate"])
def test_fused_dist_loss_is_the_switch_of_the_kvsall_job(tmp_path, monkeypatch, model, loss):
    """hip_KvsAll.fused_dist_loss: true -- every query type of every batch goes through the model's kl_loss_* / bce_loss_*
    hooks into _FusedKLDist / _FusedBCEDist (forward and backward), and score_sp / score_po are never asked; the epoch's
    avg_loss and the parameters after it are those of the job with the option off."""
    off = _job(str(tmp_path), model, False, loss=loss)
    assert type(off).__name__ == "HipTrainingJobKvsAll" and off.model._fused_dist_loss is False
    calls_off = _instrument(monkeypatch, off.model)
    l_off, st_off = _epoch(off)
    per_type = calls_off["score_sp"] + calls_off["score_po"]   # the reference's path: one score_* call per query type
    assert per_type >= len(off.loader) and calls_off[loss + "_fwd"] == calls_off[loss + "_bwd"] == 0, calls_off

    on = _job(str(tmp_path), model, True, loss=loss)
    assert on.model._fused_dist_loss is True
    calls = _instrument(monkeypatch, on.model)
    l_on, st_on = _epoch(on)
    other = "bce" if loss == "kl" else "kl"
    assert calls[loss + "_fwd"] == calls[loss + "_bwd"] == per_type, (calls, per_type)
    assert calls[other + "_fwd"] == calls["score_sp"] == calls["score_po"] == 0, calls
    assert calls["directions"] == {"sp", "po"}
    assert abs(l_on - l_off) <= 1e-5 * max(1.0, abs(l_off)), (l_on, l_off)
    # (Adagrad divides by the accumulated gradient: where an element's gradient is rounding noise of two float32
    # summation orders, the first steps still move it by a fraction of the learning rate)
    for k in st_off:
        assert torch.allclose(st_on[k], st_off[k], rtol=0.0, atol=2e-3), k


@needs_reference
@pytest.mark.parametrize("option", [None, False])
def test_with_the_option_off_or_absent_the_hooks_are_never_asked(tmp_path, monkeypatch, option):
    job = _job(str(tmp_path), "hip_transe", option)
    assert job.model._fused_dist_loss is False
    calls = _instrument(monkeypatch, job.model)
    for hook in ("kl_loss_sp", "kl_loss_po", "bce_loss_sp", "bce_loss_po"):
        setattr(job.model, hook, lambda *a, _h=hook, **k: pytest.fail(_h + " asked with the option off"))
    _epoch(job)
    assert calls["kl_fwd"] == calls["bce_fwd"] == 0 and calls["score_sp"] + calls["score_po"] >= len(job.loader)


@needs_reference
def test_without_a_device_the_option_declines_and_values_are_those_of_the_option_off(tmp_path):
    """job.device: cpu with the option on and NO stand-in: `_fused()` declines, the reference's path runs."""
    res = {}
    for option in (True, False):
        job = _job(str(tmp_path), "hip_rotate", option)
        assert job.model._fused_dist_loss is option and job.model._ce_dist_tables() is None
        z = torch.zeros(2, dtype=torch.long)
        assert job.model.kl_loss_sp(z, z, torch.arange(3), z) is None and job.model.bce_loss_po(z, z, torch.arange(3), z) is None
        res[option] = _epoch(job)
    assert res[True][0] == res[False][0]
    assert all(torch.equal(res[True][1][k], res[False][1][k]) for k in res[False][1])


@needs_reference
@pytest.mark.parametrize("option", [False, True])
def test_hip_complex_is_unaffected(tmp_path, monkeypatch, option):
    job = _job(str(tmp_path), "hip_complex", option)
    calls = _instrument(monkeypatch, job.model)
    job.model._ce_dist_tables = types.MethodType(type(job.model)._ce_dist_tables, job.model)  # the real decision
    assert job.model._ce_dist_tables() is None
    _epoch(job)
    assert calls["kl_fwd"] == calls["bce_fwd"] == 0 and calls["score_sp"] + calls["score_po"] >= len(job.loader), calls


@needs_reference
@pytest.mark.parametrize("loss", ["kl", "bce"])
def test_label_smoothing_declines_before_any_backward(tmp_path, monkeypatch, loss):
    """KvsAll.label_smoothing > 0 with the option on: the whole subbatch takes the reference's path -- no fused function
    is entered, every query type is scored by score_sp / score_po, the loss is the option-off job's."""
    res = {}
    for option in (True, False):
        job = _job(str(tmp_path), "hip_transe", option, loss=loss, smoothing=0.4)
        calls = _instrument(monkeypatch, job.model)
        res[option] = _epoch(job)[0]
        assert calls["kl_fwd"] == calls["bce_fwd"] == calls["kl_bwd"] == calls["bce_bwd"] == 0, calls
        assert calls["score_sp"] + calls["score_po"] >= len(job.loader)
    assert res[True] == res[False]


def test_repeated_labels_are_found():
    rh.import_reference()
    from kge_amd.libkge_plugin.train_job import _has_repeated_labels
    t = lambda rows: torch.tensor(rows, dtype=torch.int32).view(-1, 2)
    assert not _has_repeated_labels(t([])) and not _has_repeated_labels(t([[0, 3]]))
    assert not _has_repeated_labels(t([[0, 3], [0, 1], [1, 3], [2, 0], [2, 3]]))   # ids in any order, shared between rows
    assert _has_repeated_labels(t([[0, 3], [0, 1], [1, 3], [2, 0], [0, 3]]))
    assert _has_repeated_labels(t([[5, 0], [5, 0]]))


@needs_reference
@pytest.mark.parametrize("loss", ["kl", "bce"])
def test_a_split_that_repeats_a_triple_declines_before_any_backward(tmp_path, monkeypatch, loss):
    """A repeated training triple is a repeated id in a label row (a 2 in the reference's dense labels); the fused
    entries take unique ids, so the batch takes the reference's path: no fused function entered, the option-off loss."""
    res = {}
    for option in (True, False):
        job = _job(str(tmp_path), "hip_transe", option, loss=loss, repeat_a_triple=True)
        calls = _instrument(monkeypatch, job.model)
        res[option] = _epoch(job)[0]
        assert len(job.loader) == 1   # (five training triples: every batch holds the repeat)
        assert calls["kl_fwd"] == calls["bce_fwd"] == calls["kl_bwd"] == calls["bce_bwd"] == 0, calls
        assert calls["score_sp"] + calls["score_po"] >= 1
    assert res[True] == res[False]


@needs_reference
def test_reciprocal_wrapper_forwards_the_option_to_its_base_model(tmp_path, monkeypatch):
    """hip_reciprocal_relations_model over hip_transe: the job sets the option on the base model; both query types are
    sp_ queries of the base model's kl_loss_sp, no score_* call."""
    off = _job(str(tmp_path), "hip_reciprocal_relations_model", False, base="hip_transe")
    l_off, _ = _epoch(off)
    job = _job(str(tmp_path), "hip_reciprocal_relations_model", True, base="hip_transe")
    base = job.model._base_model
    assert base._fused_dist_loss is True and job.model._ce_dist_tables() is None   # (cpu: the real decision)
    calls = _instrument(monkeypatch, base)
    assert job.model._ce_dist_tables() is not None
    l_on, _ = _epoch(job)
    assert calls["kl_fwd"] == calls["kl_bwd"] >= len(job.loader) and calls["directions"] == {"sp"}, calls
    assert calls["score_sp"] == calls["score_po"] == 0, calls
    assert abs(l_on - l_off) <= 1e-5 * max(1.0, abs(l_off)), (l_on, l_off)


@needs_reference
def test_1vsall_bce_takes_the_fused_functions(tmp_path, monkeypatch):
    """hip_1vsAll with train.loss: bce and fused_dist_loss: true: a distance model goes through _process_subbatch_bce
    (one label per row) -- bce_loss_sp, then bce_loss_po; with the option off the reference's path, the same loss."""
    off = _job(str(tmp_path), "hip_transe", False, train_type="hip_1vsAll", loss="bce")
    calls_off = _instrument(monkeypatch, off.model)
    l_off, _ = _epoch(off)
    assert calls_off["bce_fwd"] == 0 and calls_off["score_sp"] == calls_off["score_po"] == len(off.loader)
    on = _job(str(tmp_path), "hip_transe", True, train_type="hip_1vsAll", loss="bce")
    calls = _instrument(monkeypatch, on.model)
    l_on, _ = _epoch(on)
    assert calls["bce_fwd"] == calls["bce_bwd"] == 2 * len(on.loader) and calls["directions"] == {"sp", "po"}, calls
    assert calls["score_sp"] == calls["score_po"] == calls["kl_fwd"] == 0, calls
    assert abs(l_on - l_off) <= 1e-5 * max(1.0, abs(l_off)), (l_on, l_off)
