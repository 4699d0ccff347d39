"""Shared negative samples (negative_sampling.shared: true) through an UNMODIFIED LibKGE on the MI355X:
`hip_transe` / `hip_complex` under `hip_negative_sampling` -- the shared sample objects scored by
kge_score_neg_shared, the backward by kge_score_neg_shared_bwd_accum -- against the reference model under the
reference job from the same initial parameters, and `fused_shared: false` against the plain job.  Needs the
reference package (oracle/ref_harness.py), like tests/test_gpu_libkge_plugin.py."""
import os
import shutil

import pytest
import torch

import ref_harness as rh

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

E, R = 2000, 20
MODULES = ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    from kge_amd.synthetic import make_splits, write_libkge_dataset
    root = tmp_path_factory.mktemp("libkge_gpu_shared")
    splits = make_splits(E, R, 4096, 256, 256, seed=3)
    folder = write_libkge_dataset(str(root / "small"), "small", E, R, splits)
    return str(root), folder


def _train_epoch(root, folder, tag, model, train_type, shared_type, opts=None, init_from=None):
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    from kge.util.seed import seed_from_config
    config = Config()
    config.folder = os.path.join(root, tag)
    shutil.rmtree(config.folder, ignore_errors=True)
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", MODULES)
    base = None
    if isinstance(model, tuple):  # (reciprocal wrapper, base model)
        model, base = model
    config.set("model", model)
    config._import(model)
    if base is not None:
        config._import(base)
        config.set(f"{model}.base_model.type", base)
    config.set("dataset.name", "small")
    config.set("job.device", "cuda")
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 256)
    config.set("train.num_workers", 0)
    config.set("lookup_embedder.dim", 128)
    for key in ("default", "torch", "numpy", "python"):
        config.set("random_seed." + key, 17)
    config.set("valid.every", 0)
    if train_type.startswith("hip_"):
        config._import(train_type)
    config.set("train.type", train_type)
    config.set("negative_sampling.num_samples.s", 64)
    config.set("negative_sampling.num_samples.o", 64)
    config.set("negative_sampling.shared", True)
    config.set("negative_sampling.shared_type", shared_type)
    config.set("negative_sampling.with_replacement", True)
    for k, v in (opts or {}).items():
        config.set(k, v, create=True)
    seed_from_config(config)  # (the shared samplers draw with numpy / random: sampler.py:620-698)
    torch.manual_seed(17)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder))
    if init_from is not None:
        job.model.load_state_dict(init_from)
    state0 = {k: v.detach().clone() for k, v in job.model.state_dict().items()}
    torch.manual_seed(23)
    job._prepare()
    trace = job.run_epoch()
    torch.cuda.synchronize()
    return job, trace["avg_loss"], state0


def _rel(a, b):
    return abs(a - b) / max(1.0, abs(b))


def _param_diff(job_a, job_b):
    out = 0.0
    for (ka, a), (kb, b) in zip(job_a.model.state_dict().items(), job_b.model.state_dict().items()):
        assert ka == kb and a.shape == b.shape
        out = max(out, float((a.float() - b.float()).norm() / b.float().norm().clamp_min(1e-30)))
    return out


@pytest.fixture
def naive_samples_take_a_slice(monkeypatch):
    """NaiveSharedNegativeSample.samples(indexes) takes len() of the job's slice (sampler.py:414) and raises; the
    "triple" implementation TransE is forced to (transe.py:58-68) calls it.  For the REFERENCE runs of that case the
    slice is turned into the range it stands for -- nothing else of the reference changes."""
    rh.import_reference()
    from kge.util.sampler import NaiveSharedNegativeSample
    orig = NaiveSharedNegativeSample.samples

    def samples(self, indexes=None):
        if isinstance(indexes, slice):
            indexes = range(*indexes.indices(len(self.positive_triples)))
        return orig(self, indexes)

    monkeypatch.setattr(NaiveSharedNegativeSample, "samples", samples)


@pytest.fixture
def counters(monkeypatch):
    """Calls of engine.score_neg_shared, and of the shared sample classes' own `score` (the stand-in shadows it on the
    instance: the class method only runs where the fused path was not taken)."""
    rh.import_reference()
    from kge.util import sampler
    from kge_amd import engine
    calls = {"shared": 0, "sampler": 0}
    orig = engine.score_neg_shared

    def spy(*a, **k):
        calls["shared"] += 1
        return orig(*a, **k)

    monkeypatch.setattr(engine, "score_neg_shared", spy)
    for cls in (sampler.NaiveSharedNegativeSample, sampler.DefaultSharedNegativeSample):
        def score(self, model, indexes=None, _orig=cls.score):
            calls["sampler"] += 1
            return _orig(self, model, indexes)
        monkeypatch.setattr(cls, "score", score)
    return calls


RECIPROCAL = "reciprocal_relations_model"


@pytest.mark.parametrize("shared_type", ["naive", "default"])
@pytest.mark.parametrize("model", ["transe", "complex", "reciprocal_distmult"])
def test_shared_samples_through_the_fused_kernels(data, naive_samples_take_a_slice, counters, model, shared_type):
    """One epoch (16 batches of 256, 2 x 64 shared samples with replacement) against the reference model and job from
    the same initial parameters: loss within 1e-4 relative, parameters within 1e-3 (TransE 5e-3: its L1 norm has a sign()
    gradient and Adagrad's first step is +-lr whatever the gradient's size -- a coordinate within rounding of 0 steps the
    other way; the bounds of test_b_negative_sampling_jobs); score_neg_shared ran for every slot and batch, the
    sampler's own score never.  Switched on through hip_negative_sampling.fused_shared.  "reciprocal_distmult":
    hip_reciprocal_relations_model over hip_distmult against the reference wrapper over distmult -- the wrapper's
    hook, a corrupted subject scored as the corrupted object of the reversed triple (o, p + R, s)."""
    root, folder = data
    tag = f"{model}_{shared_type}"
    ref_model, hip_model = model, "hip_" + model
    if model == "reciprocal_distmult":
        ref_model, hip_model = (RECIPROCAL, "distmult"), ("hip_" + RECIPROCAL, "hip_distmult")
    ref, l_ref, st = _train_epoch(root, folder, "ref_" + tag, ref_model, "negative_sampling", shared_type)
    assert counters["shared"] == 0 and counters["sampler"] == 2 * 16
    counters["sampler"] = 0
    fus, l_fus, _ = _train_epoch(root, folder, "fus_" + tag, hip_model, "hip_negative_sampling", shared_type,
                                 opts={"hip_negative_sampling.fused_shared": True}, init_from=st)
    assert type(fus).__name__ == "HipTrainingJobNegativeSampling"
    assert counters["shared"] == 2 * 16 and counters["sampler"] == 0, counters
    d = _param_diff(fus, ref)
    print(f"shared {tag}: loss ref {l_ref:.8g} fused {l_fus:.8g} rel {_rel(l_fus, l_ref):.3e} param rel diff {d:.3e}")
    assert _rel(l_fus, l_ref) <= 1e-4
    assert d <= (5e-3 if model == "transe" else 1e-3)


@pytest.mark.parametrize("model", ["transe", "complex"])
def test_fused_shared_false_is_the_plain_job(data, naive_samples_take_a_slice, counters, model):
    """hip_negative_sampling.fused_shared: false (where `true` takes the fused kernels: the test above) -- the sampler's
    own score, the loss of hip_<model> under the plain negative_sampling job to 1e-6."""
    root, folder = data
    plain, l_plain, st = _train_epoch(root, folder, "plain_" + model, "hip_" + model, "negative_sampling", "default")
    off, l_off, _ = _train_epoch(root, folder, "off_" + model, "hip_" + model, "hip_negative_sampling", "default",
                                 opts={"hip_negative_sampling.fused_shared": False}, init_from=st)
    assert counters["shared"] == 0 and counters["sampler"] == 2 * 2 * 16, counters
    assert _rel(l_off, l_plain) <= 1e-6, (l_off, l_plain)
