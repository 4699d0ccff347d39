"""The reference's negative-sampling losses outside the bce family, restated for the tests of kge_ns_loss: torch's own
modules in the op order of kge/util/loss.py on the label matrix TrainingJobNegativeSampling builds (column 0 = 1, the
rest 0; train_negative_sampling.py:128-137), callable in float32 and float64 (the dtype of `scores` decides):

  kl              KLDivLoss(log_softmax(scores), normalize(labels, p=1))                     loss.py:211-213
  margin_ranking  MarginRankingLoss(margin)(positives repeated K times, negatives, ones)    loss.py:236-252
  soft_margin     SoftMarginLoss(scores.view(-1), (labels * 2 - 1).view(-1))                 loss.py:221-224
  se              MSELoss(scores, labels)                                                    loss.py:272-274

all with reduction "sum".  tests/test_ns_loss_ref_cpu.py pins every one of them to the reference's own loss objects,
bit for bit, where the reference package is importable."""
import torch
import torch.nn.functional as F

KINDS = ("kl", "margin_ranking", "soft_margin", "se")


def labels_of(scores):
    labels = torch.zeros(scores.shape, device=scores.device, dtype=scores.dtype)
    labels[:, 0] = 1
    return labels


def ns_loss(scores, kind, margin=1.0):
    """The scalar loss (differentiable) of a [n, 1 + K] score block."""
    labels = labels_of(scores)
    K = scores.shape[1] - 1
    if kind == "kl":
        return torch.nn.KLDivLoss(reduction="sum")(F.log_softmax(scores, dim=1), F.normalize(labels, p=1, dim=1))
    if kind == "margin_ranking":
        flat = labels.view(-1)
        pos_positives = flat.nonzero().view(-1)
        pos_negatives = (flat == 0).nonzero().view(-1)
        pos_positives = pos_positives.view(-1, 1).repeat(1, K).view(-1)
        positives = scores.view(-1)[pos_positives].view(-1)
        negatives = scores.view(-1)[pos_negatives].view(-1)
        target = torch.ones(positives.size(), device=scores.device, dtype=scores.dtype)
        return torch.nn.MarginRankingLoss(margin=margin, reduction="sum")(positives, negatives, target)
    if kind == "soft_margin":
        return torch.nn.SoftMarginLoss(reduction="sum")(scores.view(-1), (labels * 2 - 1).view(-1))
    if kind == "se":
        return torch.nn.MSELoss(reduction="sum")(scores, labels)
    raise ValueError(kind)


def loss_and_grad(scores, kind, margin=1.0):
    """(loss, d loss / d scores) by torch autograd through ns_loss, in the dtype of `scores`."""
    x = scores.detach().clone().requires_grad_(True)
    loss = ns_loss(x, kind, margin)
    loss.backward()
    return loss.detach(), x.grad
