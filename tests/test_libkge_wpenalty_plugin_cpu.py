"""`fold_weighted_penalties` of the hip_* training jobs without a GPU: the key exists on all three jobs and is off by
default; with it off `_fold_penalties` declines weighted terms exactly as before and touches neither the optimizer nor
`model.penalty`; hip_KvsAll never reads it; on a CPU job the plan is declined (the tables are not on a GPU) and nothing
is changed either.  The plan itself -- which columns of `triples` each table counts, the captured step -- needs the
device: tests/test_gpu_libkge_wpenalty_plugin.py."""
import pytest
import torch

import ref_harness as rh
from test_abi_sparse_adam_cpu import _job

pytestmark = pytest.mark.skipif(not rh.available(), reason="reference package `kge` not on this box")

WEIGHTED = {"train.optimizer.default.type": "HipAdagrad", "lookup_embedder.regularize": "lp",
            "lookup_embedder.regularize_args.weighted": True, "hip_distmult.entity_embedder.regularize_weight": 1e-2,
            "hip_distmult.relation_embedder.regularize_weight": 1e-2}


def test_the_key_exists_on_all_three_jobs_and_is_off(tmp_path):
    for train_type in ("hip_negative_sampling", "hip_1vsAll", "hip_KvsAll"):
        job = _job(tmp_path, "key_" + train_type, {"train.optimizer.default.type": "HipAdagrad"}, train_type=train_type)
        assert job.config.get(f"{train_type}.fold_weighted_penalties") is False


@pytest.mark.parametrize("train_type", ["hip_negative_sampling", "hip_1vsAll", "hip_KvsAll"])
@pytest.mark.parametrize("on", [False, True])
def test_declines_change_nothing(tmp_path, train_type, on):
    opts = dict(WEIGHTED, **{f"{train_type}.fold_weighted_penalties": on})
    job = _job(tmp_path, f"{train_type}_{on}", opts, train_type=train_type)
    from kge_amd.libkge_plugin import train_job as tj  # (after _job put the reference package on the path)
    assert tj._fold_weighted_option(job) is (on and train_type != "hip_KvsAll")
    penalty_before = job.model.penalty
    assert tj._fold_penalties(job) is False            # off: weighted terms; on: the tables are not on a GPU
    assert tj._fold_penalties(job) is False            # (the cached decision)
    assert job.model.penalty == penalty_before and not job.optimizer.has_penalties()
    assert not getattr(job, "_weighted_penalties", None)
    tj._count_weighted(job, None)                      # nothing planned: no launch, `triples` is not looked at
    tj._set_weighted_m(job, 64)


def _plan(tmp_path, monkeypatch, tag, opts, model="hip_distmult", train_type="hip_negative_sampling", alter=None):
    """_fold_penalties on a CPU job whose tables answer `is_cuda` with True (the one condition this box cannot meet) and
    whose optimizer records the set_penalty calls instead of allocating device buffers.
    -> (the decision, the recorded calls, the job)."""
    job = _job(tmp_path, tag, opts, model=model, train_type=train_type)
    from kge_amd.libkge_plugin import train_job as tj
    calls = []
    monkeypatch.setattr(job.optimizer, "set_penalty", lambda w, *a, **k: calls.append((w, a, k)), raising=False)
    monkeypatch.setattr(torch.nn.Parameter, "is_cuda", property(lambda self: True), raising=False)
    if alter is not None:
        alter(job)
    try:
        return tj._fold_penalties(job), calls, job
    finally:
        monkeypatch.undo()


def test_unweighted_terms_are_planned_as_before_whatever_the_option_says(tmp_path, monkeypatch):
    """The unweighted plan does not depend on the new key: `times` 2 for the shared entity embedder, 1 for the relations."""
    plans = []
    for on in (False, True):
        opts = dict(WEIGHTED, **{"lookup_embedder.regularize_args.weighted": False,
                                 "hip_negative_sampling.fold_weighted_penalties": on})
        ok, calls, job = _plan(tmp_path, monkeypatch, f"unweighted_{on}", opts)
        assert ok is True and not job._weighted_penalties
        assert all("weighted" not in k for _w, _a, k in calls)
        plans.append([(k, p, times) for _e, _w, k, p, _wt, times in job._folded_penalties])
    assert plans[0] == plans[1] == [("lp", 2, 1.0), ("lp", 2, 2.0)]


@pytest.mark.parametrize("train_type", ["hip_negative_sampling", "hip_1vsAll"])
@pytest.mark.parametrize("regularize,space,p,kind", [("lp", "euclidean", 1, "lp"), ("lp", "euclidean", 3, "lp"),
                                                     ("n3", "complex", 3, "n3_complex")])
def test_the_weighted_plan(tmp_path, monkeypatch, train_type, regularize, space, p, kind):
    """Relation table: triples[:, P]; shared entity table: the S and the O column; times 1 for both (no doubling);
    set_penalty(..., weighted=True) with the embedder's own weight."""
    rh.import_reference()
    from kge.job.train_negative_sampling import S, P, O
    opts = dict(WEIGHTED, **{"lookup_embedder.regularize": regularize, "lookup_embedder.space": space,
                             "lookup_embedder.regularize_args.p": p,
                             "hip_distmult.entity_embedder.regularize_weight": 0.02,
                             "hip_distmult.relation_embedder.regularize_weight": 0.3,
                             f"{train_type}.fold_weighted_penalties": True})
    ok, calls, job = _plan(tmp_path, monkeypatch, f"plan_{train_type}_{regularize}{p}", opts, train_type=train_type)
    assert ok is True
    rel, ent = job.model.get_p_embedder()._embeddings.weight, job.model.get_s_embedder()._embeddings.weight
    assert [(w is rel, w is ent, cols) for w, cols in job._weighted_penalties] == [(True, False, (P,)),
                                                                                   (False, True, (S, O))]
    assert (S, P, O) == (0, 1, 2)
    assert [(k_, p_, wt, times) for _e, _w, k_, p_, wt, times in job._folded_penalties] == \
        [(kind, p, 0.3, 1.0), (kind, p, 0.02, 1.0)]
    assert [(w is rel, w is ent, a, k) for w, a, k in calls] == [
        (True, False, (kind, p, 0.3, 1.0), {"weighted": True}), (False, True, (kind, p, 0.02, 1.0), {"weighted": True})]
    # the wrapper hands the reference's terms back while no step was taken inside the batch
    assert job.model.penalty.__name__ == "penalty" and job.model.penalty.__qualname__.startswith("_fold_penalties")


def _two_entity_embedders(job):
    import copy
    other = copy.deepcopy(job.model.get_s_embedder())
    job.model.get_o_embedder = lambda: other


def _hip_sparse_adam(job):
    from kge_amd import optim as kopt
    job.optimizer = kopt.SparseAdam([p for p in job.model.parameters()], lr=0.01)


def _n3_on_a_real_space(job):
    for emb in (job.model.get_s_embedder(), job.model.get_p_embedder()):
        emb.regularize = "n3"   # (lookup_embedder.py:158: the weighted branch takes no abs there -- the signed cubes)
        assert emb.space != "complex"


ON = {"hip_negative_sampling.fold_weighted_penalties": True}
DECLINES = {
    "option off": ({"hip_negative_sampling.fold_weighted_penalties": False}, "hip_distmult", None),
    "n3 on a real space": (ON, "hip_distmult", _n3_on_a_real_space),
    "p = 4": (dict(ON, **{"lookup_embedder.regularize_args.p": 4}), "hip_distmult", None),
    "weighted and unweighted mixed": (dict(ON, **{"lookup_embedder.regularize_args.weighted": False,
                                                 "hip_distmult.entity_embedder.regularize_args.weighted": True}),
                                      "hip_distmult", None),
    "subject and object embedders differ": (ON, "hip_distmult", _two_entity_embedders),
    "HipSparseAdam": (ON, "hip_distmult", _hip_sparse_adam),
}


@pytest.mark.parametrize("case", sorted(DECLINES))
def test_every_decline_leaves_optimizer_and_model_alone(tmp_path, monkeypatch, case):
    more, model, alter = DECLINES[case]
    rh.import_reference()
    box = {}

    def alter_and_note(job):
        if alter is not None:
            alter(job)
            if alter is _hip_sparse_adam:  # (the fresh optimizer: record on it too)
                job.optimizer.set_penalty = lambda w, *a, **k: box.setdefault("calls", []).append(w)
        box["penalty"] = job.model.penalty
    ok, calls, job = _plan(tmp_path, monkeypatch, "decline_" + case.replace(" ", "_").replace("=", ""),
                           dict(WEIGHTED, **more), model=model, alter=alter_and_note)
    assert ok is False, case
    assert calls == [] and "calls" not in box and job.model.penalty == box["penalty"]
    assert not job._folded_penalties and not getattr(job, "_weighted_penalties", None)


def test_a_wrapper_with_a_penalty_of_its_own_is_declined(tmp_path, monkeypatch):
    """The reciprocal-relations wrapper splits the relation rows itself (its penalty is not KgeModel.penalty)."""
    rh.import_reference()
    from kge.model import KgeModel

    def wrap(job):
        cls = type("Wrapper", (type(job.model),), {"penalty": lambda self, **kw: KgeModel.penalty(self, **kw)})
        job.model.__class__ = cls
    ok, calls, job = _plan(tmp_path, monkeypatch, "decline_wrapper", dict(WEIGHTED, **ON), alter=wrap)
    assert ok is False and calls == [] and not job._folded_penalties
