"""KgeModel.score_so of the hip_* models inside an unmodified LibKGE on the GPU: the two option combinations that reach
kge_score_so -- hip_KvsAll with `KvsAll.query_types.s_o: true` and hip_negative_sampling with relation-slot negatives
under `negative_sampling.implementation: batch` -- against the reference job on the reference model, same initial
weights and seeds (the pattern of tests/test_gpu_libkge_rescal_plugin.py on a toy dataset, the loss and parameter
tolerances of the KvsAll cases of tests/test_gpu_libkge_plugin.py); the reciprocal wrapper keeps refusing."""
import os
import shutil

import pytest
import torch

import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R, D = 60, 5, 16
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_score_so")
    splits = make_splits(E, R, 400, 60, 60, seed=3)
    return str(root), write_libkge_dataset(str(root / "toy"), "toy", E, R, splits)


def _config(root, tag, model, train_type, opts=None, base=None):
    rh.import_reference()
    from kge import Config
    config = Config()
    config.folder = os.path.join(root, tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", MODULES)
    config.set("model", model)
    config._import(model)
    if base is not None:
        config._import(base)
        config.set(f"{model}.base_model.type", base)
    config.set("dataset.name", "toy")
    config.set("job.device", "cuda")
    config.set("train.type", train_type)
    if train_type.startswith("hip_"):
        config._import(train_type)
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 64)
    config.set("train.num_workers", 0)
    config.set("lookup_embedder.dim", D)
    config.set("valid.every", 0)
    for k in ("default", "torch", "numpy", "python"):
        config.set(f"random_seed.{k}", 17)
    for k, v in (opts or {}).items():
        config.set(k, v, create=True)
    return config


class _Counter:
    """counts the calls of kge_amd.engine.score_so (the one way to the kernel)"""

    def __init__(self, monkeypatch):
        from kge_amd import engine
        self.calls, self._orig = 0, engine.score_so
        monkeypatch.setattr(engine, "score_so", self)

    def __call__(self, *a, **kw):
        self.calls += 1
        return self._orig(*a, **kw)


def _epoch(root, folder, tag, model, train_type, opts, init_from=None):
    rh.import_reference()
    from kge import Dataset
    from kge.job import TrainingJob
    config = _config(root, tag, model, train_type, opts)
    dataset = Dataset.create(config, folder=folder)
    torch.manual_seed(17)
    job = TrainingJob.create(config, dataset)
    if init_from is not None:
        job.model.load_state_dict(init_from)
    state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
    torch.manual_seed(23)
    job._prepare()
    job._is_prepared = True
    trace = job.run_epoch()
    torch.cuda.synchronize()
    return job, float(trace["avg_loss"]), state0


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _param_diff(job_a, job_b):
    out = 0.0
    for (ka, a), (kb, b) in zip(job_a.model.state_dict().items(), job_b.model.state_dict().items()):
        assert ka == kb and a.shape == b.shape
        out = max(out, float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)))
    return out


def _compare(data, monkeypatch, tag, model, ref_type, hip_type, opts):
    root, folder = data
    ref, l_ref, st = _epoch(root, folder, f"{tag}_ref", model, ref_type, opts)
    cnt = _Counter(monkeypatch)
    hip, l_hip, _ = _epoch(root, folder, f"{tag}_hip", "hip_" + model, hip_type, opts, init_from=st)
    print(f"score_so plugin {tag}: loss ref {l_ref:.6f} hip {l_hip:.6f}, param rel diff {_param_diff(hip, ref):.3e}, "
          f"engine.score_so calls {cnt.calls}")
    assert cnt.calls > 0
    assert torch.isfinite(torch.tensor(l_hip)) and _rel(l_hip, l_ref) <= 1e-2
    assert _param_diff(hip, ref) <= 5e-2


@pytest.mark.parametrize("model", ["distmult", "transe"])
def test_hip_kvsall_with_s_o_queries(data, monkeypatch, model):
    _compare(data, monkeypatch, f"kvs_{model}", model, "KvsAll", "hip_KvsAll", {"KvsAll.query_types.s_o": True})


@pytest.mark.parametrize("model", ["distmult", "transe"])
def test_hip_negative_sampling_with_relation_slot_negatives(data, monkeypatch, model):
    opts = {"negative_sampling.num_samples.s": 3, "negative_sampling.num_samples.p": 2,
            "negative_sampling.num_samples.o": 3, "negative_sampling.implementation": "batch"}
    _compare(data, monkeypatch, f"ns_{model}", model, "negative_sampling", "hip_negative_sampling", opts)


def test_the_reciprocal_wrapper_cannot_score_relations(data):
    rh.import_reference()
    from kge import Dataset
    from kge.model import KgeModel
    root, folder = data
    config = _config(root, "recip", "hip_reciprocal_relations_model", "KvsAll", base="hip_distmult")
    dataset = Dataset.create(config, folder=folder)
    m = KgeModel.create(config, dataset)
    s = torch.zeros(2, dtype=torch.long, device="cuda")
    with pytest.raises(Exception, match="The reciprocal relations model cannot score relations."):
        m.score_so(s, s)
