"""Gradients of the ConvE score in eval mode: float64 autograd of the restated network (torch on the CPU) and an
elementwise bound for a float32 evaluation of the same graph in ANY summation order.

Loss  L = sum_ij G_ij score_sp_ij + sum_i g_i score_spo_i,  scores as in tests/_conve_ref.py (eval mode).

With the ReLU masks fixed, every operation of the graph is linear in each of its operands: a convolution, a scaling by
rsq > 0, a matrix product, an addition.  Replace every input, parameter, running mean and upstream gradient by its
absolute value and every subtraction by an addition, keep the masks and the positive scales: the gradient of that
"absolute graph" with respect to a leaf, A, is the sum over all paths of the products of the ABSOLUTE local factors -- the
quantity a float32 evaluation's rounding errors are relative to (no cancellation left), and the forward values that enter
a backward product (features, query rows) are bounded by their absolute-graph twins.  A float32 evaluation commits one
rounding of relative size u = 2^-24 per operation; along any path from the loss to a leaf, forward values included, there
are at most K of them:

  K = K_fwd + K_bwd
  K_fwd = fs^2 + 1 (conv chain) + 3 + 2 (rsq, bn1) + F + 1 (projection, any order) + 3 + 2 (bn2) + d + 1 (contraction)
  K_bwd = E (g_q: a sum over the targets) + n (g_ent: over the queries) + 2 (bn2) + d (g_feature) + n (g_proj_w) + 2 (bn1)
          + n Ho Wo (g_conv_w: over rows and positions) + 32 fs^2 (g_image) + 2 n (the scatter of row gradients into the
          tables, twice: a row may be subject and target)

so |g32 - g64| <= gamma_K A with gamma_K = K u / (1 - K u) (the standard accumulation of K relative errors), plus FLOOR.
The masks must be the same in both evaluations: `stable` says whether every pre-activation is farther from 0 than its
forward bound (tests/_conve_ref.py); the tests assert it for their inputs.  Nothing is tuned or measured."""
import numpy as np
import torch

import _conve_ref as cr


def _leaves(net, ent, rel, absolute):
    f = (lambda a: np.abs(np.asarray(a, np.float64))) if absolute else (lambda a: np.asarray(a, np.float64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(f(a))).requires_grad_()  # noqa: E731
    fs = net["fs"]
    leaves = dict(ent=t(ent), rel=t(rel), conv_w=t(net["conv_w"].reshape(32, 1, fs, fs)), proj_w=t(net["proj_w"]),
                  proj_b=t(net["proj_b"]))
    if net["conv_b"] is not None:
        leaves["conv_b"] = t(net["conv_b"])
    return leaves


def _loss(net, L, s, p, o, G, g, masks=None):
    """masks None: the true graph (returns the loss and its masks); else the absolute graph under those masks"""
    h, w, pad = net["h"], net["w"], net["pad"]
    ab = masks is not None
    c = (lambda a: torch.from_numpy(np.abs(np.asarray(a, np.float64)))) if ab else \
        (lambda a: torch.from_numpy(np.asarray(a, np.float64)))
    sgn = 1.0 if ab else -1.0
    r1 = torch.from_numpy(1.0 / np.sqrt(np.asarray(net["var1"], np.float64) + net["eps1"]))
    r2 = torch.from_numpy(1.0 / np.sqrt(np.asarray(net["var2"], np.float64) + net["eps2"]))
    e, r = L["ent"][torch.from_numpy(s)], L["rel"][torch.from_numpy(p)]
    img = torch.cat([e[:, 1:].reshape(-1, 1, h, w), r[:, 1:].reshape(-1, 1, h, w)], 2)
    v = torch.nn.functional.conv2d(img, L["conv_w"], L.get("conv_b"), stride=1, padding=pad)
    z1 = (v + sgn * c(net["mean1"]).view(1, -1, 1, 1)) * r1.view(1, -1, 1, 1)
    m1 = (z1 > 0).double() if not ab else masks[0]
    x = (z1 * m1).reshape(len(s), -1) @ L["proj_w"].t() + L["proj_b"]
    z2 = (x + sgn * c(net["mean2"])) * r2
    m2 = (z2 > 0).double() if not ab else masks[1]
    q = z2 * m2
    sp = q @ L["ent"][:, 1:].t() + L["ent"][:, 0]
    eo = L["ent"][torch.from_numpy(o)]
    spo = (q * eo[:, 1:]).sum(-1) + eo[:, 0]
    return (sp * c(G)).sum() + (spo * c(g)).sum(), (m1.detach(), m2.detach())


def gradients(net, ent, rel, s, p, o, G, g):
    """{leaf: (float64 gradient, bound)} and `stable`"""
    n, E = len(s), ent.shape[0]
    Ho, Wo = cr.out_hw(net["h"], net["w"], net["fs"], net["pad"])
    d, fs, F = net["h"] * net["w"], net["fs"], 32 * Ho * Wo
    K = (fs * fs + 1 + 5 + F + 1 + 5 + d + 1) + (E + n + 2 + d + n + 2 + n * Ho * Wo + 32 * fs * fs + 2 * n)
    gamma = K * cr.U / (1.0 - K * cr.U)
    L = _leaves(net, ent, rel, False)
    loss, masks = _loss(net, L, s, p, o, G, g)
    loss.backward()
    A = _leaves(net, ent, rel, True)
    _loss(net, A, s, p, o, G, g, masks)[0].backward()
    z1, e1 = cr.features(net, ent, rel, s, p, defect="no_relu1")
    x, ex = cr._pre_bn2(net, ent, rel, s, p, None, "any")
    z2, e2 = cr._norm_relu(x, ex, net["mean2"], net["var2"], net["eps2"], None, relu=False)
    stable = bool((np.abs(z1) > cr.bound(e1)).all() and (np.abs(z2) > cr.bound(e2)).all())
    return {k: (L[k].grad.numpy(), gamma * A[k].grad.numpy() + cr.FLOOR) for k in L}, stable
