"""kge_sparse_adam_step_touched and kge_amd.optim.SparseAdam without a GPU: symbol and prototype, every status code of
the header reached without a launch, the state-dict round trip with torch.optim.SparseAdam, and the ValueError gates of
the optimizer and of the LibKGE plugin (`HipSparseAdam`)."""
import copy
import os
import re
import shutil

import pytest
import torch

import ref_harness as rh
from conftest import ROOT

OK, INVALID, UNSUPPORTED = 0, -1, -2
NAME = "kge_sparse_adam_step_touched"


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def _call(lib, **kw):
    a = dict(param=16, param_ld=8, grad=16, grad_ld=8, m1=16, m1_ld=8, m2=16, m2_ld=8, bitmap=16, num_rows=40, dim=8,
             clock=32, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, copy=None, copy_ld=0)
    a.update(kw)
    return lib.kge_sparse_adam_step_touched(a["param"], a["param_ld"], a["grad"], a["grad_ld"], a["m1"], a["m1_ld"],
                                            a["m2"], a["m2_ld"], a["bitmap"], a["num_rows"], a["dim"], a["clock"],
                                            a["lr"], a["beta1"], a["beta2"], a["eps"], a["copy"], a["copy_ld"], None)


def test_symbol_and_prototype(lib):
    from kge_amd import _lib
    header = open(ROOT + "/include/kge_amd.h").read()
    assert NAME in _lib.PROTOTYPES and hasattr(lib, NAME)
    proto = re.search(r"int " + NAME + r"\((.*?)\);", header, re.S).group(1)
    assert len(proto.split(",")) == len(_lib.PROTOTYPES[NAME][1]) == 19
    assert "kge_adam_clock* clock" in proto and "double lr, double beta1, double beta2" in proto
    for phrase in ("ONCE PER CALL", "grad is None", "STILL decays", "neither read nor written"):
        assert phrase in header, phrase


def test_every_refusal_of_the_header_without_a_launch(lib):
    # sizes
    assert _call(lib, num_rows=-1) == INVALID and _call(lib, dim=-1) == INVALID
    assert _call(lib, dim=1 << 31, param_ld=1 << 31, grad_ld=1 << 31, m1_ld=1 << 31, m2_ld=1 << 31) == INVALID
    # a pitch below dim
    for ld in ("param_ld", "grad_ld", "m1_ld", "m2_ld"):
        assert _call(lib, **{ld: 7}) == INVALID, ld
    assert _call(lib, copy=16, copy_ld=7) == INVALID
    # NULL arrays with rows to step
    for name in ("param", "grad", "m1", "m2", "bitmap"):
        assert _call(lib, **{name: None}) == INVALID, name
    # the clock: NULL or misaligned, whatever num_rows
    for n in (40, 0):
        assert _call(lib, clock=None, num_rows=n) == INVALID
        assert _call(lib, clock=36, num_rows=n) == INVALID
    # betas outside [0, 1)
    for bad in (dict(beta1=1.0), dict(beta1=-0.1), dict(beta2=1.5), dict(beta2=float("nan"))):
        assert _call(lib, **bad) == INVALID, bad
        assert _call(lib, num_rows=0, **bad) == INVALID, bad
    # more than 2^31 - 1 workgroups of 256 rows: declined before the clock is launched
    assert _call(lib, num_rows=256 << 31) == UNSUPPORTED
    assert _call(lib, num_rows=(256 << 31) - 256 + 1) == UNSUPPORTED


def test_state_dict_round_trip_with_torch_sparse_adam():
    from kge_amd import optim as kopt
    w = [torch.nn.Parameter(torch.randn(6, 4)), torch.nn.Parameter(torch.randn(3, 4))]
    ours = kopt.SparseAdam(w, lr=0.1, betas=(0.8, 0.95), eps=1e-6)
    assert isinstance(ours, torch.optim.SparseAdam) and ours.graph_capturable
    for k, p in enumerate(w):  # (what a step leaves, the clock record included)
        ours.state[p].update(step=3 + k, exp_avg=torch.randn_like(p), exp_avg_sq=torch.rand_like(p),
                             clock=torch.zeros(4, dtype=torch.int64))
    sd = ours.state_dict()
    assert all(sorted(st) == ["exp_avg", "exp_avg_sq", "step"] for st in sd["state"].values())
    assert "clock" in ours.state[w[0]]
    w2 = [torch.nn.Parameter(p.detach().clone()) for p in w]
    theirs = torch.optim.SparseAdam(w2, lr=0.1, betas=(0.8, 0.95), eps=1e-6)
    theirs.load_state_dict(sd)
    for a, b in zip(w, w2):
        assert theirs.state[b]["step"] == ours.state[a]["step"]
        assert torch.equal(theirs.state[b]["exp_avg"], ours.state[a]["exp_avg"])
        assert torch.equal(theirs.state[b]["exp_avg_sq"], ours.state[a]["exp_avg_sq"])
    # torch's own step on a sparse gradient, then back: our class takes torch's checkpoint and torch's route
    w2[0].grad = torch.sparse_coo_tensor(torch.tensor([[1, 4]]), torch.randn(2, 4), (6, 4))
    theirs.step()
    back = kopt.SparseAdam(w, lr=0.1, betas=(0.8, 0.95), eps=1e-6)
    back.load_state_dict(copy.deepcopy(theirs.state_dict()))  # (load_state_dict keeps the tensors it is handed)
    assert back.state[w[0]]["step"] == 4 and back.state[w[1]]["step"] == 4 and "clock" not in back.state[w[0]]
    assert torch.equal(back.state[w[0]]["exp_avg"], theirs.state[w2[0]]["exp_avg"])
    w[0].grad = torch.sparse_coo_tensor(torch.tensor([[0, 4]]), torch.ones(2, 4), (6, 4))
    w2[0].grad = w[0].grad.clone()
    w2[0].data.copy_(w[0].data)
    back.step()
    theirs.step()
    assert torch.equal(w[0].detach(), w2[0].detach()) and back.state[w[0]]["step"] == 5
    assert back.stepped_params() == [w[0]]
    # a dense gradient: torch's error
    w[1].grad = torch.ones_like(w[1])
    with pytest.raises(RuntimeError, match="does not support dense gradients"):
        back.step()


def test_optimizer_gates():
    from kge_amd import optim as kopt
    from kge_amd.train_graph import GraphedStep
    w = [torch.nn.Parameter(torch.zeros(4, 4))]
    with pytest.raises(ValueError, match="weight_decay"):
        kopt.SparseAdam(w, lr=0.1, weight_decay=1e-3)
    with pytest.raises(NotImplementedError):
        kopt.SparseAdam(w, lr=0.1, maximize=True)
    opt = kopt.SparseAdam(w, lr=0.1)
    st = GraphedStep(lambda *a: None, opt)
    assert st.enabled and st.disabled_reason is None
    with pytest.raises(ValueError, match="GPU parameter"):
        opt.enable_touched_rows(w[0])  # a CPU table
    with pytest.raises(ValueError, match="not a parameter"):
        opt.enable_touched_rows(torch.nn.Parameter(torch.zeros(2, 2)))
    assert opt.touched_rows(w[0]) is None and opt.stepped_params() == []


# ---- the plugin ------------------------------------------------------------------------------------------------------
def _job(tmp_path, tag, opts, device="cpu", model="hip_distmult", train_type="hip_negative_sampling"):
    """A LibKGE training job on a 60-entity toy dataset, prepared (tests/test_gpu_libkge_sparse_adam_plugin.py too)."""
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    folder = str(tmp_path / "toy")
    if not os.path.isdir(folder):
        write_libkge_dataset(folder, "toy", 60, 5, make_splits(60, 5, 256, 16, 16, seed=3))
    config = Config()
    config.folder = str(tmp_path / tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
    config.set("model", model)
    config._import(model)
    if train_type.startswith("hip_"):
        config._import(train_type)
    config.set("dataset.name", "toy")
    config.set("job.device", device)
    config.set("train.type", train_type)
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 64)
    config.set("train.num_workers", 0)
    config.set("lookup_embedder.dim", 16)
    config.set("valid.every", 0)
    config.set("negative_sampling.num_samples.s", 4)
    config.set("negative_sampling.num_samples.o", 4)
    config.set("train.optimizer.default.type", "HipSparseAdam")
    for k, v in opts.items():
        config.set(k, v, create=True)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder))
    job._prepare()
    job._is_prepared = True
    return job


@pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")
def test_plugin_gates(tmp_path, monkeypatch):
    import torch.optim
    from kge_amd import optim as kopt
    rh.import_reference()
    import kge_amd.libkge_plugin  # noqa: F401  (registers the optimizers)
    assert torch.optim.HipSparseAdam is kopt.SparseAdam
    # the option is off by default, and HipSparseAdam without it raises: it has no dense path
    job = _job(tmp_path, "off", {})
    assert job.config.get("hip_negative_sampling.touched_rows") is False
    assert isinstance(job.optimizer, kopt.SparseAdam)
    with pytest.raises(ValueError, match="touched_rows"):
        job.run_epoch()
    # on, but not on a GPU: declined by the Adagrad path's first condition -> a ValueError naming it
    job = _job(tmp_path, "cpu", {"hip_negative_sampling.touched_rows": True})
    with pytest.raises(ValueError, match="touched_rows with HipSparseAdam: not a CUDA device"):
        job.run_epoch()
    # weight_decay: the optimizer's own ValueError
    with pytest.raises(ValueError, match="weight_decay"):
        _job(tmp_path, "wd", {"hip_negative_sampling.touched_rows": True,
                              "train.optimizer.default.args.weight_decay": 1e-4})
    # what the Adagrad touched path declines further down -- penalty terms, dropout -- on either table: reached with
    # the device and fused-path conditions (which this box cannot meet) answered for the job
    batch = {"negative_samples": [None, None, None]}
    for tag, opts, word in (
            ("pen_e", {"hip_distmult.entity_embedder.regularize_weight": 1e-6}, "regularize_weight > 0 on the entity"),
            ("pen_r", {"hip_distmult.relation_embedder.regularize_weight": 1e-6}, "regularize_weight > 0 on the relation"),
            ("drop_e", {"hip_distmult.entity_embedder.dropout": 0.2}, "entity embedder is not a plain"),
            ("drop_r", {"hip_distmult.relation_embedder.dropout": 0.2}, "relation embedder is not a plain")):
        job = _job(tmp_path, tag, dict(opts, **{"hip_negative_sampling.touched_rows": True}))
        monkeypatch.setattr(job, "device", "cuda:0")
        monkeypatch.setattr(job.model, "_fused", lambda: True)
        assert word in job._touched_rows_why_not(batch), (tag, job._touched_rows_why_not(batch))
        with pytest.raises(ValueError, match="touched_rows with HipSparseAdam: .*" + word):
            job._decide_touched_rows(batch)
    # HipAdagrad with the option off (the default): nothing is decided, nothing raises
    job = _job(tmp_path, "adagrad", {"train.optimizer.default.type": "HipAdagrad"})
    job._decide_touched_rows(batch)
    assert job.touched_rows is False and job.touched_rows_declined is None
