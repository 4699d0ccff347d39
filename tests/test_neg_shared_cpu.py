"""Shared negative samples (negative_sampling.shared: true) without a GPU: engine.shared_samples against the live
reference's sample objects, the control flow of hip_negative_sampling with a `score_neg_shared` hook against the
reference job, and the argument validation of the new C entry points."""
import os
import random
import shutil
import types

import numpy as np
import pytest
import torch

import ref_harness as rh

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")


def _sampler(shared_type, with_replacement, num_s, num_o):
    rh.import_reference()
    from kge import Config, Dataset
    from kge.util.sampler import KgeSampler
    config = Config()
    config.folder = None
    config.set("console.quiet", True)
    config.set("dataset.name", "dataset_test")
    config.set("negative_sampling.sampling_type", "uniform")
    config.set("negative_sampling.shared", True)
    config.set("negative_sampling.shared_type", shared_type)
    config.set("negative_sampling.with_replacement", with_replacement)
    config.set("negative_sampling.num_samples.s", num_s)
    config.set("negative_sampling.num_samples.o", num_o)
    config.set("negative_sampling.implementation", "batch")  # (what the job resolves "auto" to for shared samples)
    config.set("negative_sampling.filtering.s", False)
    config.set("negative_sampling.filtering.o", False)
    dataset = Dataset.create(config, folder=os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"))
    return KgeSampler.create(config, "negative_sampling", dataset), dataset


def _parts(smp):
    return smp._unique_samples, getattr(smp, "_drop_index", None), smp._repeat_indexes


@needs_reference
@pytest.mark.parametrize("with_replacement", [True, False])
@pytest.mark.parametrize("shared_type", ["naive", "default"])
def test_shared_samples_equal_the_reference_sample_objects(shared_type, with_replacement):
    """engine.shared_samples(unique, drop, repeat, n) == NaiveSharedNegativeSample.samples() /
    DefaultSharedNegativeSample.samples() of objects drawn by KgeUniformSampler._sample_shared on dataset_test: both
    slots, several seeds, few samples (without replacement no repeats: the sampler's empty FLOAT tensor) and more
    samples than entities (with replacement: many repeats); dataset_test has four entities, so the batches of the
    default kind hold positives that are in the unique list, and their column shows the spare."""
    from kge_amd import engine
    seen_repeats = seen_no_repeats = seen_dropped_positive = 0
    for num in ((3, 5), (40, 64)) if with_replacement else ((2, 3), (3, 1)):  # (dataset_test has 4 entities)
        sampler, dataset = _sampler(shared_type, with_replacement, *num)
        triples = dataset.split("train").long()
        for seed in range(4):
            for slot in (0, 2):
                np.random.seed(100 + seed)
                random.seed(200 + seed)
                smp = sampler._sample_shared(triples, slot, int(sampler.num_samples[slot]))
                unique, drop, repeat = _parts(smp)
                want = smp.samples()
                got = engine.shared_samples(unique, drop, repeat, len(triples))
                assert got.shape == want.shape == (len(triples), int(sampler.num_samples[slot]))
                assert torch.equal(got, want)
                if repeat.numel() == 0:
                    assert repeat.dtype == torch.float32  # torch.empty(0): the quirk shared_samples must take
                    seen_no_repeats += 1
                else:
                    seen_repeats += 1
                if drop is not None:
                    uc = unique.numel() - 1
                    in_list = (triples[:, slot].unsqueeze(1) == unique[:uc].unsqueeze(0)).any(dim=1)
                    seen_dropped_positive += int(in_list.sum())
                    # (a positive in the list is never among its own row's samples, unless it is the spare's repeat)
                    rows = torch.nonzero(in_list).view(-1)
                    assert not (got[rows, :uc] == triples[rows, slot].unsqueeze(1)).any()
    assert seen_no_repeats > 0 or with_replacement
    assert seen_repeats > 0 or not with_replacement
    assert seen_dropped_positive > 0 or shared_type == "naive"


def test_shared_samples_rules_by_hand():
    from kge_amd import engine
    unique = torch.tensor([10, 11, 12, 99])
    drop = torch.tensor([3, 0, 2])  # row 0 uses no spare; row 1 drops column 0; row 2 drops column 2
    repeat = torch.tensor([2, 2, 0])
    got = engine.shared_samples(unique, drop, repeat, 3)
    assert got.tolist() == [[10, 11, 12, 12, 12, 10], [99, 11, 12, 12, 12, 99], [10, 11, 99, 99, 99, 10]]
    assert engine.shared_samples(unique, None, torch.empty(0), 2).tolist() == [[10, 11, 12, 99]] * 2
    assert engine.shared_samples(unique, None, None, 1).tolist() == [[10, 11, 12, 99]]


def _job_config(tmp, model, train_type, base=None):
    rh.import_reference()
    from kge import Config
    config = Config()
    config.folder = os.path.join(tmp, f"run_{train_type}_{model}")
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
    if train_type.startswith("hip_"):
        config._import(train_type)
    config.set("train.type", train_type)
    return config


@needs_reference
@pytest.mark.parametrize("reciprocal", [False, "wrapper", "base"])
@pytest.mark.parametrize("shared_type", ["naive", "default"])
def test_shared_negative_sampling_job_follows_the_reference_job(tmp_path, shared_type, reciprocal):
    """Control flow of HipTrainingJobNegativeSampling with shared samples on CPU: with a model whose
    `score_neg_shared` is the reference's own arithmetic (score_spo over engine.shared_samples), one epoch must give the
    reference job's avg_loss and parameters -- the stand-in's slicing of the positives and the drop indexes, the
    positives' column, labels and loss scaling are then the same -- and the hook must have been called for the subject
    and the object slot.  The path is switched on through the job's option, hip_negative_sampling.fused_shared.  Also
    over hip_reciprocal_relations_model: with the stub as the wrapper's hook ("wrapper"), and with the stub as the BASE
    model's hook under the wrapper's own score_neg_shared ("base": its translation of a corrupted subject into the
    corrupted object of the reversed triple (o, p + R, s) is then what is compared with the reference wrapper)."""
    from kge import Dataset
    from kge.job import TrainingJob
    from kge_amd import engine
    data = os.path.join(str(tmp_path), "dataset_test")
    shutil.copytree(os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"), data)
    calls = []

    def score_neg_shared(self, s, p, o, slot, unique, drop=None, repeat=None):
        calls.append(slot)
        n = s.numel()
        if drop is not None:
            assert drop.numel() == n
        neg = engine.shared_samples(unique, drop, repeat, n)
        K = neg.shape[1]
        tr = [x.reshape(-1).long().repeat_interleave(K) for x in (s, p, o)]
        tr[slot] = neg.reshape(-1).long()
        return self.score_spo(tr[0], tr[1], tr[2], direction="spo"[slot]).view(-1, K)

    results = {}
    for train_type in ("negative_sampling", "hip_negative_sampling"):
        hip = train_type.startswith("hip_")
        base = ("hip_" if hip else "") + "distmult"
        if reciprocal:
            config = _job_config(str(tmp_path), ("hip_" if hip else "") + "reciprocal_relations_model", train_type, base)
        else:
            config = _job_config(str(tmp_path), base, train_type)
        config.set("negative_sampling.num_samples.s", 40)
        config.set("negative_sampling.num_samples.o", 7)
        config.set("negative_sampling.shared", True)
        config.set("negative_sampling.shared_type", shared_type)
        config.set("negative_sampling.with_replacement", True)
        if hip:
            config.set("hip_negative_sampling.fused_shared", True)
        torch.manual_seed(21)
        job = TrainingJob.create(config, Dataset.create(config, folder=data))
        if hip:
            assert type(job).__name__ == "HipTrainingJobNegativeSampling"
            if reciprocal == "base":
                base_model = job.model._base_model
                base_model.score_neg_shared = types.MethodType(score_neg_shared, base_model)
                job.model._base_fused = lambda: True  # (no HIP device here: the wrapper would decline before the hook)
            else:
                job.model.score_neg_shared = types.MethodType(score_neg_shared, job.model)
        torch.manual_seed(22)
        np.random.seed(23)   # (the shared samplers draw with numpy / random: sampler.py:640-700)
        random.seed(24)
        job._prepare()
        trace = job.run_epoch()
        results[train_type] = (trace["avg_loss"], [x.detach().clone() for x in job.model.parameters()])
    # (fails without the feature: the shared sample objects kept their own score; under the wrapper's translation the
    # base model is asked for its object slot both times)
    assert set(calls) == ({2} if reciprocal == "base" else {0, 2}) and len(calls) >= 2
    (l_ref, p_ref), (l_hip, p_hip) = results["negative_sampling"], results["hip_negative_sampling"]
    assert abs(l_ref - l_hip) <= 1e-6 * max(1.0, abs(l_ref)), (l_ref, l_hip)
    for a, b in zip(p_ref, p_hip):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-7)


@needs_reference
@pytest.mark.parametrize("option", [None, False, True])
def test_fused_shared_is_the_switch(tmp_path, option):
    """hip_negative_sampling.fused_shared: true asks the model's hook for both slots of every batch; false, and the
    option left alone (its default is false), never ask it."""
    from kge import Dataset
    from kge.job import TrainingJob
    data = os.path.join(str(tmp_path), "dataset_test")
    shutil.copytree(os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"), data)
    calls = []
    config = _job_config(str(tmp_path), "hip_distmult", "hip_negative_sampling")
    config.set("negative_sampling.num_samples.s", 4)
    config.set("negative_sampling.num_samples.o", 3)
    config.set("negative_sampling.shared", True)
    if option is not None:
        config.set("hip_negative_sampling.fused_shared", option)
    job = TrainingJob.create(config, Dataset.create(config, folder=data))

    def hook(self, s, p, o, slot, unique, drop=None, repeat=None):
        calls.append(slot)
        return None  # declined: the sampler's own score

    job.model.score_neg_shared = types.MethodType(hook, job.model)
    job._prepare()
    job.run_epoch()
    assert set(calls) == ({0, 2} if option else set())


def test_shared_entries_validate_arguments_without_a_device():
    """kge_score_neg_shared / kge_score_neg_shared_bwd_accum: NULL tables or output, negative sizes, a slot other than
    0 / 2 and repeats without a list are invalid arguments (-1); n == 0 or K == 0 is a no-op (0) -- all before any
    launch."""
    import ctypes
    from kge_amd import _lib
    from kge_amd._lib import KgeIndex, KgeTables
    _lib.build()
    lib = _lib.lib()
    P = ctypes.c_void_p(16)  # never dereferenced on these paths
    good = KgeIndex(P, 1, 0, 1)
    t = KgeTables(P, P, 0, 2, 10, 3, 32, 32, 32, 32, 1.0, 0)       # f32 TransE
    no_tables = KgeTables(None, None, 0, 2, 10, 3, 32, 32, 32, 32, 1.0, 0)
    T = ctypes.byref(t)

    def fwd(tb=T, n=4, slot=0, unique=P, uc=5, drop=None, repeat=None, nrep=0, out=P, ldo=16):
        return lib.kge_score_neg_shared(tb, good, good, good, n, slot, unique, 1, uc, drop, repeat, nrep, out, ldo, None)

    def bwd(tb=T, n=4, slot=0, unique=P, uc=5, drop=None, repeat=None, nrep=0, gout=P, ge=P, gr=P, ws=P, wsb=1 << 20):
        return lib.kge_score_neg_shared_bwd_accum(tb, good, good, good, n, slot, unique, 1, uc, drop, repeat, nrep, gout,
                                                  16, None, 0, ge, 32, gr, 32, ws, wsb, None)

    for call in (fwd, bwd):
        assert call(tb=None) == -1
        assert call(tb=ctypes.byref(no_tables)) == -1
        assert call(n=-1) == -1
        assert call(uc=-1) == -1
        assert call(nrep=-2) == -1
        assert call(slot=1) == -1 and call(slot=3) == -1
        assert call(nrep=3, repeat=None) == -1
        assert call(unique=None) == -1
        assert call(n=0) == 0
        assert call(uc=0, nrep=0) == 0
        assert call(n=0, unique=None) == 0
    assert fwd(out=None) == -1
    assert fwd(ldo=4) == -1          # ldo < K
    assert bwd(gout=None) == -1 and bwd(ge=None) == -1 and bwd(gr=None) == -1
    bf16 = KgeTables(P, P, 1, 2, 10, 3, 32, 32, 32, 32, 1.0, 0)
    assert bwd(tb=ctypes.byref(bf16)) == -2   # f32 tables only
    assert lib.kge_score_neg_shared_workspace_bytes(T, 4, 5) >= 2 * 4 * 6 * 4
    assert lib.kge_score_neg_shared_workspace_bytes(T, 0, 5) == 0
    assert lib.kge_abi_version() == 1
