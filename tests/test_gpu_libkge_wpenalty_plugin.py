"""`fold_weighted_penalties` of hip_negative_sampling / hip_1vsAll through an unmodified LibKGE epoch on the MI355X.

Every configuration runs twice from the same initial parameters: with the option on (the weighted lp / n3 terms counted
on the device and folded into the optimizer's pass, the step captured) and with it off -- the path of the commit before
the option existed: the reference's torch.unique / gather / autograd terms, which keep the whole job eager.  Epoch loss
and the traced penalty values agree within 2e-5 (the tolerance of the unweighted penalty tests of
tests/test_gpu_libkge_plugin.py); with the option on the step is captured once and replayed."""
import pytest
import torch

from test_gpu_libkge_plugin import DEVICE, _rel, _train_epoch, data  # noqa: F401  (data: the module's dataset fixture)

pytestmark = pytest.mark.gpu

NS = {"negative_sampling.num_samples.s": 16, "negative_sampling.num_samples.o": 16,
      "negative_sampling.implementation": "triple", "train.loss": "kl"}
CASES = {
    "ns_lp2_adagrad": ("distmult", "hip_negative_sampling", 64, dict(NS, **{
        "lookup_embedder.regularize": "lp", "lookup_embedder.regularize_args.p": 2,
        "train.optimizer.default.type": "HipAdagrad"})),
    "ns_lp3_adagrad_touched": ("distmult", "hip_negative_sampling", 64, dict(NS, **{
        "lookup_embedder.regularize": "lp", "lookup_embedder.regularize_args.p": 3,
        "train.optimizer.default.type": "HipAdagrad", "hip_negative_sampling.touched_rows": True})),
    "ns_n3_adam": ("complex", "hip_negative_sampling", 64, dict(NS, **{
        "lookup_embedder.regularize": "n3", "lookup_embedder.space": "complex",
        "train.optimizer.default.type": "HipAdam", "train.optimizer.default.args.device_step": True,
        "train.optimizer.default.args.lr": 0.001})),
    "1vsall_n3_adagrad": ("complex", "hip_1vsAll", 128, {
        "lookup_embedder.regularize": "n3", "lookup_embedder.space": "complex", "train.loss": "kl",
        "train.optimizer.default.type": "HipAdagrad", "hip_complex.score_dtype": "bfloat16",
        "train.optimizer.default.args.bf16_copies": True}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_folded_weighted_terms_follow_the_eager_reference_terms(data, case):
    if DEVICE == "cpu":
        pytest.skip("needs the GPU")
    root, folder = data
    model, job_type, dim, opts = CASES[case]
    opts = dict(opts, **{"lookup_embedder.regularize_args.weighted": True,
                         f"hip_{model}.entity_embedder.regularize_weight": 2e-2,
                         f"hip_{model}.relation_embedder.regularize_weight": 5e-2})
    off, l_off, st = _train_epoch(root, folder, f"wpen_off_{case}", "hip_" + model, job_type, dim, opts)
    on, l_on, _ = _train_epoch(root, folder, f"wpen_on_{case}", "hip_" + model, job_type, dim,
                               dict(opts, **{f"{job_type}.fold_weighted_penalties": True}), init_from=st)
    # the option off: nothing folded, nothing captured (the weighted terms keep the job eager, as before)
    assert not off.optimizer.has_penalties() and off._graph_step is None
    gs = on._graph_step
    assert gs is not None and gs.disabled_reason is None and gs.captures == 1 and gs.replays >= 90, vars(gs)
    assert on.optimizer.has_penalties() and len(on._folded_penalties) == 2 and len(on._weighted_penalties) == 2
    if opts.get("hip_negative_sampling.touched_rows"):
        assert on.touched_rows is True, on.touched_rows_declined
    for w, _cols in on._weighted_penalties:
        assert not on.optimizer.penalty_counts(w).any()
    pen_on, pen_off = on.last_epoch_trace["avg_penalties"], off.last_epoch_trace["avg_penalties"]
    print(case, "loss", l_on, l_off, "penalties", pen_on, pen_off)
    assert sorted(pen_on) == sorted(pen_off) and len(pen_on) == 2
    for k in pen_on:
        assert pen_off[k] > 0 and _rel(pen_on[k], pen_off[k]) <= 2e-5 * max(1.0, abs(pen_off[k])), (k, pen_on[k], pen_off[k])
    assert _rel(l_on, l_off) <= 2e-5, (l_on, l_off)
