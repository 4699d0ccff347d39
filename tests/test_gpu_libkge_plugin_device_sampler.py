"""`hip_negative_sampling.device_sampler` through an UNMODIFIED LibKGE on the MI355X: the sample blocks of the subject
and object slot drawn by kge_amd.sampler.DeviceSampler (kge_neg_sample) in `_prepare_batch` instead of KgeSampler.sample
in the collate function; everything downstream -- DefaultBatchNegativeSample, the fused scoring, the captured step, the
losses -- is what the job runs with the option off.  Toy dataset of tests/test_gpu_libkge_plugin_shared.py (16 batches
of 256, 2 x 64 per-triple negatives, dim 128).  Needs the reference package, like the harness it uses.

The sanity bound against the reference's sampler is no precision bound: the epoch-1 loss with the option on must lie
within the spread of five differently seeded runs with the option off, widened by 50 % (it catches a sampler that draws
from the wrong range or for the wrong slot)."""
import os
import shutil

import numpy as np
import pytest
import torch

import ref_harness as rh
from test_gpu_libkge_plugin_shared import MODULES, data  # noqa: F401  (`data`: the toy dataset fixture)

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")]

S, P, O = 0, 1, 2
ON = {"hip_negative_sampling.device_sampler": True}
OFF = {"hip_negative_sampling.device_sampler": False}
FILTER = {"negative_sampling.filtering.s": True, "negative_sampling.filtering.o": True}
NO_GRAPH = {"hip_negative_sampling.graph_step": False}
HIP_ADAGRAD = {"train.optimizer.default.type": "HipAdagrad"}


@pytest.fixture
def alias_functions(monkeypatch):
    """KgeFrequencySampler.__init__ (sampler.py:761-778) builds its tables with torch._multinomial_alias_setup and draws
    with torch._multinomial_alias_draw; recent torch releases no longer have the two private functions.  Where they are
    missing the reference's sampler gets stand-ins with their contract ((J, q) = setup(probs); draw(q, J, n)) -- the
    reference's own code is untouched."""
    from kge_amd.sampler import alias_setup
    if not hasattr(torch, "_multinomial_alias_setup"):
        def setup(probs):
            q, J = alias_setup(probs.numpy())
            return torch.from_numpy(J), torch.from_numpy(q.astype(np.float64))

        def draw(q, J, n):
            bucket = torch.randint(len(q), (n,))
            return torch.where(torch.rand(n, dtype=q.dtype) < q[bucket], bucket, J[bucket])

        monkeypatch.setattr(torch, "_multinomial_alias_setup", setup, raising=False)
        monkeypatch.setattr(torch, "_multinomial_alias_draw", draw, raising=False)


def _run(data, tag, model, *opts, seed=17, spy=False):
    """One epoch -> (job, epoch loss, record).  record (spy=True): the calls of the reference's sampler per slot and what
    `_process_subbatch` saw of each batch's sample blocks."""
    root, folder = data
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
    config.set("model", model)
    config._import(model)
    config.set("dataset.name", "small")
    config.set("job.device", "cuda")
    config.set("train.max_epochs", 1)
    config.set("train.batch_size", 256)
    config.set("train.num_workers", 0)
    config.set("lookup_embedder.dim", 128)
    for key in ("default", "torch", "numpy", "python"):
        config.set("random_seed." + key, seed)
    config.set("valid.every", 0)
    config._import("hip_negative_sampling")
    config.set("train.type", "hip_negative_sampling")
    config.set("negative_sampling.num_samples.s", 64)
    config.set("negative_sampling.num_samples.o", 64)
    config.set("negative_sampling.shared", False)
    config.set("negative_sampling.implementation", "triple")
    for extra in opts:
        for k, v in extra.items():
            config.set(k, v, create=True)
    seed_from_config(config)
    torch.manual_seed(seed)
    job = TrainingJob.create(config, Dataset.create(config, folder=folder))
    record = {"host_calls": {S: 0, P: 0, O: 0}, "blocks": [], "classes": set()}
    if spy:
        host_sample = job._sampler.sample

        def sample(triples, slot, num_samples=None):
            record["host_calls"][slot] += 1
            return host_sample(triples, slot, num_samples)
        job._sampler.sample = sample
        process = job._process_subbatch

        def process_subbatch(batch_index, batch, subbatch_slice, result):
            for slot in (S, O):
                ns = batch["negative_samples"][slot]
                record["classes"].add(type(ns).__name__)
                record["blocks"].append((slot, batch["triples"].detach().clone(), ns.samples().detach().clone()))
            return process(batch_index, batch, subbatch_slice, result)
        job._process_subbatch = process_subbatch
    torch.manual_seed(seed + 6)
    job._prepare()
    trace = job.run_epoch()
    torch.cuda.synchronize()
    return job, trace["avg_loss"], record


def _train_keys(job, slot):
    """Sorted keys (corrupted entity, and the row's other two ids) of the training triples, for np.isin."""
    tri = job.dataset.split("train").numpy().astype(np.int64)
    E, R = job.dataset.num_entities(), job.dataset.num_relations()
    return np.unique((tri[:, slot] * R + tri[:, P]) * E + tri[:, O if slot == S else S]), E, R


def _check_blocks(job, record, filtered):
    assert record["classes"] == {"DefaultBatchNegativeSample"}
    assert len(record["blocks"]) == 2 * 16
    hits = 0
    for slot, triples, block in record["blocks"]:
        assert block.is_cuda and block.dtype == torch.int64 and tuple(block.shape) == (len(triples), 64)
        keys, E, R = _train_keys(job, slot)
        t, b = triples.cpu().numpy().astype(np.int64), block.cpu().numpy()
        assert b.min() >= 0 and b.max() < E
        other = t[:, O if slot == S else S]
        cand = (b * R + t[:, P, None]) * E + other[:, None]
        hits += int(np.isin(cand, keys).sum())
    if filtered:
        assert hits == 0, f"{hits} samples are training answers of their rows"
    return hits


def test_filtered_uniform_samples_come_from_the_device(data):
    off, l_off, _ = _run(data, "ds_off", "hip_complex", OFF, FILTER, HIP_ADAGRAD)
    on, l_on, rec = _run(data, "ds_on", "hip_complex", ON, FILTER, HIP_ADAGRAD, spy=True)
    assert off._device_sampler is None and off._device_slots == ()
    assert on._device_slots == (S, O) and on._device_sampler.filter == {S: True, O: True}
    _check_blocks(on, rec, filtered=True)
    assert rec["host_calls"][S] == 0 and rec["host_calls"][O] == 0 and rec["host_calls"][P] == 16
    assert on._device_sampler.calls == 2 * 16
    print(f"hip_complex filtered uniform: loss host sampler {l_off:.8g} device sampler {l_on:.8g}; graph batches "
          f"{off.graph_batches} / {on.graph_batches}")
    assert np.isfinite(l_on) and l_on > 0
    assert on.graph_batches == off.graph_batches and on.graph_batches > 0


def test_frequency_samples_come_from_the_device(data, alias_functions):
    on, l_on, rec = _run(data, "ds_freq", "hip_transe", ON, FILTER, {"negative_sampling.sampling_type": "frequency"}, spy=True)
    assert on._device_slots == (S, O) and on._device_sampler.sampling_type == "frequency"
    assert set(on._device_sampler._alias) == {S, O}
    _check_blocks(on, rec, filtered=True)
    assert rec["host_calls"][S] == 0 and rec["host_calls"][O] == 0
    print(f"hip_transe frequency: loss {l_on:.8g}")
    assert np.isfinite(l_on) and l_on > 0


def _same_batches(rec_a, rec_b):
    assert len(rec_a["blocks"]) == len(rec_b["blocks"]) == 2 * 16
    for (sa, ta, ba), (sb, tb, bb) in zip(rec_a["blocks"], rec_b["blocks"]):
        assert sa == sb and torch.equal(ta, tb) and torch.equal(ba, bb)


def test_a_seeded_job_is_reproducible(data):
    """Two runs with the same random_seed.torch, graph_step off: the same batches, the same sample blocks bit for bit,
    and the same epoch loss bit for bit.

    The epoch loss is a function of the samples AND of every step's arithmetic, so the bit comparison needs a step that
    is itself a function of its inputs.  The job therefore trains the reference's `complex` model (torch's scoring,
    autograd and Adagrad: no float atomics in the step) under `hip_negative_sampling` with the device sampler: whatever
    differs between the two runs then comes from the sampler or its seeding.

    The hip_* models are compared on what the sampler controls -- batches and all 32 sample blocks equal bit for bit --
    and their losses are printed: the backward of the fused scoring (kge_score_spo_bwd_accum / kge_score_neg_bwd_accum)
    accumulates into the table gradients with float atomics, whose order differs from run to run, with the host
    sampler as with this one.  Measured on an MI355X for hip_complex: 71.4414746761322 and 71.44147419929504 (6.7e-9
    apart)."""
    a, l_a, rec_a = _run(data, "ds_rep_a", "complex", ON, FILTER, NO_GRAPH, seed=29, spy=True)
    b, l_b, rec_b = _run(data, "ds_rep_b", "complex", ON, FILTER, NO_GRAPH, seed=29, spy=True)
    assert a._device_slots == (S, O) and b._device_slots == (S, O)
    assert a.graph_batches == 0 and b.graph_batches == 0
    assert rec_a["host_calls"][S] == 0 and rec_a["host_calls"][O] == 0
    _same_batches(rec_a, rec_b)
    print(f"reproducibility, complex: {l_a!r} {l_b!r}")
    assert l_a == l_b
    c, l_c, rec_c = _run(data, "ds_rep_c", "complex", ON, FILTER, NO_GRAPH, seed=30, spy=True)
    assert not torch.equal(rec_a["blocks"][0][2], rec_c["blocks"][0][2])  # another seed, other samples
    assert l_c != l_a
    h1, l_h1, rec_h1 = _run(data, "ds_rep_h1", "hip_complex", ON, FILTER, NO_GRAPH, seed=29, spy=True)
    h2, l_h2, rec_h2 = _run(data, "ds_rep_h2", "hip_complex", ON, FILTER, NO_GRAPH, seed=29, spy=True)
    _same_batches(rec_h1, rec_h2)
    _same_batches(rec_a, rec_h1)  # (the samples do not depend on the model)
    print(f"reproducibility, hip_complex (float atomics in the backward): {l_h1!r} {l_h2!r}")
    assert abs(l_h1 - l_h2) <= 16 * 2.0 ** -24 * abs(l_h1)  # (one float32 rounding per step of the 16: not a bit test)


def test_loss_lies_within_the_reference_samplers_spread(data):
    """Five differently seeded runs with the option OFF (the reference's sampler; initial parameters and batch order
    vary with the seed too, as they do for the run with the option on) against one run with it ON."""
    ref = [_run(data, f"ds_spread_{k}", "hip_complex", OFF, FILTER, seed=100 + k)[1] for k in range(5)]
    _, l_on, _ = _run(data, "ds_spread_on", "hip_complex", ON, FILTER, seed=105)
    lo, hi = min(ref), max(ref)
    mid, half = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    print(f"option off, five seeds: {[f'{x:.8g}' for x in ref]}; option on: {l_on:.8g}; accepted [{mid - half:.8g}, "
          f"{mid + half:.8g}]")
    assert mid - half <= l_on <= mid + half


@pytest.mark.parametrize("opts,slots", [({"negative_sampling.shared": True}, ()),
                                        ({"negative_sampling.num_samples.p": 8}, (S, O)),
                                        ({"negative_sampling.num_samples.s": 0}, (O,))])
def test_configurations_that_do_not_qualify_stay_with_the_reference_sampler(data, opts, slots):
    job, loss, rec = _run(data, "ds_nq", "hip_complex", ON, opts, spy=True)
    assert job._device_slots == slots
    for slot in (S, P, O):
        assert (rec["host_calls"][slot] == 0) == (slot in slots), rec["host_calls"]
    print(f"{opts}: device slots {slots}, loss {loss:.8g}")
    assert np.isfinite(loss) and loss > 0
