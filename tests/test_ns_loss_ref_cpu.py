"""CPU side of kge_ns_loss (the negative-sampling losses kl / margin_ranking / soft_margin / se in one kernel):
tests/_ns_loss_ref.py pinned to the reference's own loss objects, torch's hinge subgradient at an exact tie, the
plumbing of the plugin's stand-in `_HipNsLoss`, and the new entry's place in the C ABI.  Nothing here launches."""
import ctypes
import os
import re

import pytest
import torch

import ref_harness as rh
import _ns_loss_ref as nr
from conftest import ROOT

needs_reference = pytest.mark.skipif(not rh.available(), reason="reference tree not present")


def _block(n=37, c=65, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, c, generator=g) * 5.0


def _reference_loss(kind, margin=1.0):
    rh.import_reference()
    from kge.util import loss as L
    config = rh.make_config("complex", 16)
    config.set("job.device", "cpu")
    config.set("train.type", "negative_sampling")
    if kind == "margin_ranking":
        return L.MarginRankingKgeLoss(config, margin=margin)
    return {"kl": L.KLDivWithSoftmaxKgeLoss, "soft_margin": L.SoftMarginKgeLoss, "se": L.SEKgeLoss}[kind](config)


@needs_reference
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("kind,margin", [("kl", 1.0), ("margin_ranking", 1.0), ("margin_ranking", 0.25),
                                         ("soft_margin", 1.0), ("se", 1.0)])
def test_the_restatement_is_bit_identical_to_the_reference_loss_objects(kind, margin, dtype):
    """_ns_loss_ref.ns_loss against KLDivWithSoftmaxKgeLoss / MarginRankingKgeLoss / SoftMarginKgeLoss / SEKgeLoss
    (kge/util/loss.py:192-274) on the job's label matrix: value and gradient, bit for bit (the same torch ops)."""
    ref = _reference_loss(kind, margin)
    scores = _block().to(dtype)
    scores[1, 0], scores[1, 1] = 2.0, 2.0 - margin   # an exact hinge tie
    labels = torch.zeros(scores.shape)   # (float32, as the job builds them)
    labels[:, 0] = 1
    a = scores.clone().requires_grad_(True)
    la = ref(a, labels.to(dtype) if kind in ("soft_margin", "se") else labels, num_negatives=scores.shape[1] - 1)
    la.backward()
    lb, gb = nr.loss_and_grad(scores, kind, margin)
    assert la.dtype == dtype and torch.equal(la.detach(), lb) and torch.equal(a.grad, gb)


@pytest.mark.parametrize("margin,x_neg", [(1.0, 1.0), (0.25, 1.75)])
def test_torch_hinge_subgradient_at_an_exact_tie_is_active(margin, x_neg):
    """x_0 = 2, x_j = 2 - margin: t = x_0 - x_j = margin and v = -t + margin = 0 exactly in float32.
    torch.nn.MarginRankingLoss's autograd (clamp_min's backward is grad * (v >= 0)) counts the tie as ACTIVE: the
    negative gets 1, the positive -1 -- the convention kge_ns_loss's kind 4 copies (`v >= 0.0f`).  A negative 2^-20
    lower and nothing flows; the loss is 0 in both."""
    tie = torch.tensor([[2.0, x_neg]])
    assert float(-(tie[0, 0] - tie[0, 1]) + torch.tensor(margin)) == 0.0
    loss, grad = nr.loss_and_grad(tie, "margin_ranking", margin)
    assert float(loss) == 0.0 and torch.equal(grad, torch.tensor([[-1.0, 1.0]]))
    below = torch.tensor([[2.0, x_neg - 2.0 ** -20]])   # (t = margin + 2^-20 is exact in float32: v = -2^-20)
    loss, grad = nr.loss_and_grad(below, "margin_ranking", margin)
    assert float(loss) == 0.0 and torch.equal(grad, torch.zeros(1, 2))
    # in a row: the positive's gradient is minus the count of active negatives (tie, active, inactive)
    row = torch.tensor([[2.0, x_neg, 5.0, -7.0]])
    _, grad = nr.loss_and_grad(row, "margin_ranking", margin)
    assert torch.equal(grad, torch.tensor([[-2.0, 1.0, 1.0, 0.0]]))


def test_mse_backward_is_exactly_two_times_the_difference():
    """torch's MSELoss(reduction="sum") backward is 2 (x - y) elementwise with one rounding of the difference (the
    doubling is exact): what kge_ns_loss's kind 6 writes, hence torch.equal in the GPU test."""
    x = _block(9, 13, seed=4) * 3.0
    _, grad = nr.loss_and_grad(x, "se")
    assert torch.equal(grad, 2.0 * (x - nr.labels_of(x)))


def test_float32_soft_margin_overflows_where_the_stable_form_does_not():
    """The reference's log(1 + exp(z)) in float32 is inf from z ~ 89 and its gradient inf / inf: the planted 90 of the
    GPU test.  float64 is finite there, and so is max(z, 0) + log1p(exp(-|z|)) in float32."""
    x = torch.tensor([[40.0, -40.0, 90.0]])
    loss32, grad32 = nr.loss_and_grad(x, "soft_margin")
    loss64, grad64 = nr.loss_and_grad(x.double(), "soft_margin")
    assert torch.isinf(loss32) and torch.isnan(grad32[0, 2])
    assert torch.isfinite(loss64) and torch.isfinite(grad64).all()
    z = torch.tensor([-40.0, -40.0, 90.0])   # z = -t x
    stable = (z.clamp_min(0) + torch.log1p(torch.exp(-z.abs()))).sum()
    assert abs(float(stable) - float(loss64)) <= 1e-5


def _plugin_config():
    rh.import_reference()
    from kge import Config
    config = Config()
    config.folder = None
    config.set("console.quiet", True)
    config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
    config.set("model", "hip_transe")
    config._import("hip_transe")
    config._import("hip_negative_sampling")
    config.set("job.device", "cpu")
    config.set("train.type", "hip_negative_sampling")
    return config


@needs_reference
@pytest.mark.parametrize("kind,margin", [("kl", 1.0), ("margin_ranking", 0.25), ("soft_margin", 1.0), ("se", 1.0)])
def test_ns_loss_stand_in_hands_everything_it_does_not_recognise_to_the_reference_loss(kind, margin):
    """_HipNsLoss wraps the job's loss object: CPU tensors, index labels and a label matrix of another pattern reach
    the reference's object unchanged -- same value, same gradient, no fused call --, its attributes stay readable
    through the wrapper, the margin is the wrapped torch loss's, and a loss built with other torch arguments is not
    taken at all."""
    config = _plugin_config()
    from kge.util import loss as L
    from kge_amd.libkge_plugin.train_job import _HipNsLoss, _other_ns_loss_kind
    ref = (L.MarginRankingKgeLoss(config, margin=margin) if kind == "margin_ranking" else
           {"kl": L.KLDivWithSoftmaxKgeLoss, "soft_margin": L.SoftMarginKgeLoss, "se": L.SEKgeLoss}[kind](config))
    assert _other_ns_loss_kind(ref) == (kind, margin if kind == "margin_ranking" else 0.0)
    w = _HipNsLoss(ref)
    assert w.kind == kind and w.config is config
    if kind == "margin_ranking":
        assert w.arg == margin == w._loss.margin
    scores = _block(9, 13, seed=2)
    labels = torch.zeros(9, 13)
    labels[:, 0] = 1
    a, b = scores.clone().requires_grad_(True), scores.clone().requires_grad_(True)
    la, lb = ref(a, labels, num_negatives=12), w(b, labels, num_negatives=12)   # CPU tensors: the reference's loss
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad) and w.fused_calls == 0
    if kind != "margin_ranking":   # (index labels under margin ranking need num_negatives pairs per row: not a job's call)
        idx = torch.zeros(9, dtype=torch.long)
        assert torch.equal(ref(scores, idx), w(scores, idx)) and w.fused_calls == 0
    if kind in ("kl", "soft_margin", "se"):   # another label pattern: two ones in a row
        other = labels.clone()
        other[:, 5] = 1
        assert torch.equal(ref(scores, other, num_negatives=12), w(scores, other, num_negatives=12))
    # non-default reduction / weight of the inner torch loss: no stand-in
    assert _other_ns_loss_kind(L.SEKgeLoss(config, reduction="mean")) is None
    assert _other_ns_loss_kind(L.SoftMarginKgeLoss(config, reduction="mean")) is None
    assert _other_ns_loss_kind(L.MarginRankingKgeLoss(config, margin=1.0, reduction="mean")) is None
    assert _other_ns_loss_kind(L.KLDivWithSoftmaxKgeLoss(config, reduction="mean")) is None
    assert _other_ns_loss_kind(L.BCEWithLogitsKgeLoss(config)) is None   # (the bce family keeps fused_loss)


@needs_reference
@pytest.mark.parametrize("loss", ["kl", "margin_ranking", "soft_margin", "se"])
@pytest.mark.parametrize("option", [None, False, True])
def test_the_option_ships_off_and_a_cpu_job_keeps_the_reference_loss(tmp_path, loss, option):
    """hip_negative_sampling.fused_other_losses is false in the shipped yaml; with it off -- and on a CPU job whatever
    it says -- the job's loss object is the reference's own."""
    import shutil
    rh.import_reference()
    from kge import Config, Dataset
    from kge.job import TrainingJob
    from kge.util import loss as L
    data = os.path.join(str(tmp_path), "dataset_test")
    shutil.copytree(os.path.join(rh.REFERENCE_ROOT, "tests", "data", "dataset_test"), data)
    config = Config()
    config.folder = os.path.join(str(tmp_path), "run")
    os.makedirs(config.folder)
    config.set("console.quiet", True)
    config.set("modules", ["kge.job", "kge.model", "kge.model.embedder", "kge_amd.libkge_plugin"])
    config.set("model", "hip_transe")
    config._import("hip_transe")
    config._import("hip_negative_sampling")
    config.set("dataset.name", "dataset_test")
    config.set("job.device", "cpu")
    config.set("train.type", "hip_negative_sampling")
    config.set("train.loss", loss)
    config.set("lookup_embedder.dim", 16)
    assert config.get("hip_negative_sampling.fused_other_losses") is False
    assert config.get("hip_negative_sampling.fused_loss") is True
    if option is not None:
        config.set("hip_negative_sampling.fused_other_losses", option)
    job = TrainingJob.create(config, Dataset.create(config, folder=data))
    assert type(job).__name__ == "HipTrainingJobNegativeSampling" and job.graph_batches == 0
    assert type(job.loss) is {"kl": L.KLDivWithSoftmaxKgeLoss, "margin_ranking": L.MarginRankingKgeLoss,
                              "soft_margin": L.SoftMarginKgeLoss, "se": L.SEKgeLoss}[loss]


@pytest.fixture(scope="module")
def lib():
    from kge_amd import _lib
    _lib.build()
    return _lib.lib()


def test_the_header_the_binding_and_the_library_agree_on_kge_ns_loss(lib):
    """The checks of tests/test_abi_cpu.py for the new name: declared in include/kge_amd.h, bound in _lib.PROTOTYPES with
    the declaration's argument count and types, exported by the library; kge_ns_bce_loss is still there."""
    from kge_amd import _lib
    header = open(os.path.join(ROOT, "include", "kge_amd.h")).read()
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(kge_\w+)\s*\(", header, flags=re.M))
    assert {"kge_ns_loss", "kge_ns_bce_loss"} <= declared and declared == set(_lib.PROTOTYPES)
    assert hasattr(lib, "kge_ns_loss") and hasattr(lib, "kge_ns_bce_loss")
    decl = re.search(r"^int\s+kge_ns_loss\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
    params = [" ".join(x.split()) for x in decl.split(",")]
    ctype = lambda p_: (ctypes.c_void_p if "*" in p_ else ctypes.c_int64 if p_.startswith("int64_t") else
                        ctypes.c_float if p_.startswith("float") else ctypes.c_int)
    res, args = _lib.PROTOTYPES["kge_ns_loss"]
    assert res is ctypes.c_int and args == [ctype(p_) for p_ in params], params
    assert [p_.split()[-1].lstrip("*") for p_ in params] == [
        "pos", "pos_stride", "neg", "neg_ld", "n", "K", "kind", "arg", "temperature", "loss_rows", "g_pos", "g_pos_stride",
        "g_neg", "g_neg_ld", "stream"]
    from kge_amd import engine
    assert engine.NS_LOSS_KINDS == {"bce": 0, "bce_mean": 1, "bce_self_adversarial": 2, "kl": 3, "margin_ranking": 4,
                                    "soft_margin": 5, "se": 6}
    assert all(engine.NS_LOSS_KINDS[k] == v for k, v in engine.NS_BCE_KINDS.items())
    assert callable(_lib.ext().ns_loss_parts)


def test_kge_ns_loss_validates_its_arguments_without_a_device(lib):
    """KGE_ERR_INVALID_ARG (-1) for K < 1, an unknown kind, a NULL piece, half a gradient, a leading dimension below K;
    n == 0 is KGE_OK -- all before any launch (no GPU here)."""
    P = ctypes.c_void_p(16)   # never dereferenced on these paths
    call = lambda pos=P, ps=1, neg=P, ld=8, n=4, K=8, kind=3, rows=P, gp=P, gps=1, gn=P, gld=8: lib.kge_ns_loss(
        pos, ps, neg, ld, n, K, kind, 1.0, 1.0, rows, gp, gps, gn, gld, None)
    assert call(K=0, ld=0, gld=0) == -1 and call(K=-3) == -1
    assert call(kind=7) == -1 and call(kind=-1) == -1
    assert call(pos=None) == -1 and call(neg=None) == -1 and call(rows=None) == -1
    assert call(gp=None) == -1 and call(gn=None) == -1           # both NULL or both set
    assert call(ld=7) == -1 and call(gld=7) == -1 and call(gps=0) == -1
    assert call(n=-1) == -1
    for kind in range(7):
        assert call(n=0, kind=kind) == 0
    assert call(n=0, pos=None, neg=None, rows=None, gp=None, gn=None) == 0


def test_engine_ns_loss_has_no_cpu_path(lib):
    from kge_amd import engine
    x = _block(4, 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.ns_loss(x, "kl")
    with pytest.raises(RuntimeError, match="no CPU path"):
        engine.ns_loss_parts(x[:, 0], x[:, 1:], "se")
