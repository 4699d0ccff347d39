"""One TRAINING-mode score call of ConvE (both dropouts 0, batch statistics on: conve.py:75-101 under Module.train()) in
float64 torch on the CPU, with a bound for a float32 evaluation of the same graph in any summation order: the scores, and
the gradients of  L = sum_ij gout_ij score_ij  for a given upstream gradient gout (what a job's loss hands back).

The method is that of tests/_conve_bwd_ref.py (the ABSOLUTE graph: every input, parameter and upstream gradient replaced
by its absolute value, every subtraction by an addition, ReLU masks and positive scales kept; a float32 evaluation's error
is at most gamma_K times the absolute graph's value, K = the roundings of the longest path), with batch-norm under batch
statistics added.  y_j = (x_j - mu) r,  mu = mean(x),  r = 1 / sqrt(var(x) + eps) depends on every x_i:

  d y_j / d x_i = r ([i == j] - 1 / N - xh_j xh_i / N),   xh = (x - mu) r   (N = the elements the statistics are taken over)

so an error (or a gradient) at x reaches y through three terms, and the absolute graph's batch-norm is

  yA_j = (xA_j + mean(xA)) r + |xh_j| mean(|xh| xA) r      (r, xh: constants from the float64 forward)

whose Jacobian is the absolute value of each term above.  This is first order in the errors (as every bound of this
family); the statistics' own roundings (two reductions over N elements, the add, sqrt and division of r) are counted in K.

ReLU masks: a unit whose pre-activation is within its forward bound gamma_{K_fwd} zA of 0 (forward values see the
forward roundings only; the scores' bound is gamma_{K_fwd} scoreA likewise) may be masked differently by the two
evaluations (with n * 32 * Ho * Wo units per call some are).  Its whole path weight is then charged, not gamma_K of it:
with M the true mask and U the unstable units,  bound = gamma_K A(M + U) + (A(M + U) - A(M - U)),  A(.) the absolute
graph's gradient under a mask -- the second term is the sum over the paths through at least one unstable unit.

  K = K_fwd + K_bwd,  N1 = n Ho Wo,  F = 32 Ho Wo
  K_fwd = fs^2 + 1 + (2 N1 + 6) + F + 1 + (2 n + 6) + d + 1
  K_bwd = E + n + (2 n + 6) + d + n + (2 N1 + 6) + N1 + 32 fs^2 + 2 n

convolution.bias and projection.bias: bn1 / bn2 subtract the batch mean, so their true gradients are 0; the bound is
gamma_K times the absolute graph's (positive) gradient -- the floor the noise has to stay under.  Nothing is tuned or measured."""
import numpy as np
import torch

U = 2.0 ** -24
FLOOR = 2.0 ** -126
NAMES = ("ent", "rel", "conv_w", "conv_b", "proj_w", "proj_b")


def _bn(x, dims, eps):
    mu = x.mean(dims, keepdim=True)
    var = ((x - mu) ** 2).mean(dims, keepdim=True)
    r = 1.0 / torch.sqrt(var + eps)
    return (x - mu) * r, r


def _bn_abs(xA, dims, r, xh):
    return (xA + xA.mean(dims, keepdim=True)) * r + xh * (xh * xA).mean(dims, keepdim=True) * r


def _leaves(P, absolute):
    out = {}
    for k in NAMES:
        if P.get(k) is not None:
            v = torch.as_tensor(np.asarray(P[k], np.float64))
            out[k] = (v.abs() if absolute else v).clone().requires_grad_()
    return out


def node(P, h, w, pad, eps1, eps2, s, p, gout):
    """P: float arrays ent [E, d + 1], rel, conv_w [32, 1, fs, fs], conv_b [32] or None, proj_w [d, F], proj_b [d];
    s, p int arrays [n]; gout [n, E].  -> (scores, score bound, {name: (gradient, bound)}), numpy float64"""
    s, p = torch.as_tensor(np.asarray(s)).long(), torch.as_tensor(np.asarray(p)).long()
    G = torch.as_tensor(np.asarray(gout, np.float64))
    n, E = G.shape
    fs = P["conv_w"].shape[-1]
    d = h * w

    def images(L):
        return torch.cat([L["ent"][s][:, 1:].reshape(n, 1, h, w), L["rel"][p][:, 1:].reshape(n, 1, h, w)], 2)

    L = _leaves(P, False)
    v = torch.nn.functional.conv2d(images(L), L["conv_w"], L.get("conv_b"), padding=pad)
    z1, r1 = _bn(v, (0, 2, 3), eps1)
    x = torch.relu(z1).reshape(n, -1) @ L["proj_w"].t() + L["proj_b"]
    z2, r2 = _bn(x, (0,), eps2)
    sp = torch.relu(z2) @ L["ent"][:, 1:].t() + L["ent"][:, 0]
    (sp * G).sum().backward()
    Ho, Wo = v.shape[2], v.shape[3]
    N1, F = n * Ho * Wo, 32 * Ho * Wo
    Kf = fs * fs + 1 + 2 * N1 + 6 + F + 1 + 2 * n + 6 + d + 1
    K = Kf + (E + n + 2 * n + 6 + d + n + 2 * N1 + 6 + N1 + 32 * fs * fs + 2 * n)
    gamma, gamma_f = K * U / (1.0 - K * U), Kf * U / (1.0 - Kf * U)
    c = dict(r1=r1.detach(), h1=z1.detach().abs(), r2=r2.detach(), h2=z2.detach().abs())

    def absolute(m1, m2):
        A = _leaves(P, True)
        vA = torch.nn.functional.conv2d(images(A), A["conv_w"], A.get("conv_b"), padding=pad)
        z1A = _bn_abs(vA, (0, 2, 3), c["r1"], c["h1"])
        xA = (z1A * m1).reshape(n, -1) @ A["proj_w"].t() + A["proj_b"]
        z2A = _bn_abs(xA, (0,), c["r2"], c["h2"])
        spA = (z2A * m2) @ A["ent"][:, 1:].t() + A["ent"][:, 0]
        (spA * G.abs()).sum().backward()
        return {k: A[k].grad.numpy() for k in A}, z1A.detach(), z2A.detach(), spA.detach()

    on1, on2 = (z1.detach() > 0).double(), (z2.detach() > 0).double()
    _, z1A, z2A, _ = absolute(on1, on2)
    u1 = (z1.detach().abs() <= gamma_f * z1A).double()
    u2 = (z2.detach().abs() <= gamma_f * z2A).double()
    hi, _, _, spA = absolute(torch.clamp(on1 + u1, max=1.0), torch.clamp(on2 + u2, max=1.0))
    lo = absolute(on1 * (1 - u1), on2 * (1 - u2))[0]
    grads = {k: (L[k].grad.numpy(), gamma * hi[k] + (hi[k] - lo[k]) + FLOOR) for k in L}
    return sp.detach().numpy(), gamma_f * spA.numpy() + FLOOR, grads, int(u1.sum() + u2.sum())
