"""ConvE's evaluation network and score (kge/model/conve.py:75-101, eval mode) restated in numpy float64 for the tests (no
torch, no GPU), with an elementwise float32 rounding bound carried along the evaluation.

  images      ent[s][1:], rel[p][1:] as h x w, stacked to 2h x w (subject on top)
  conv        v = b_c + sum_{ky,kx} img[y + ky - pad][x + kx - pad] w_c[ky][kx]      (zero padding, stride 1)
  bn / relu   f = max((v - mean) * rsq, 0),  rsq = 1 / sqrt(var + eps)
  projection  x_j = sum_k f_k W[j][k] + b_j,  k = c Ho Wo + y Wo + x
  bn2 / relu  as above, per output j
  score       q' . ent[o] with q' = [1 | x]  ==  x . ent[o][1:] + ent[o][0]

The bound follows the rules of tests/_rescal_ref.py (u = 2^-24 per written operation, inputs exact, `dot` / `prod`,
SLACK, FLOOR), with these additions, each derived, none tuned or measured:

  fma chain from a start value   v = b + sum of K products: K roundings, each on a partial sum that is at most
                                 |b| + sum |a_k b_k| in magnitude:  e = K u (|b| + sum |a_k b_k|)
  rsq                            t = var + eps:     e_t = u t
                                 r = sqrt(t):       |sqrt(t + x) - sqrt(t)| = |x| / (sqrt(t + x) + sqrt(t)) <= |x| / sqrt(t)
                                                    e_r = e_t / sqrt(t) + u (sqrt(t) + e_t / sqrt(t))     (one sqrt)
                                 y = 1 / r:         |1 / (r + x) - 1 / r| <= |x| / (r (r - |x|))
                                                    e_y = e_r / (r (r - e_r)) + u / (r - e_r)              (one division)
  a - b                          e = e_a + e_b + u (|a - b| + e_a + e_b)
  relu                           1-Lipschitz: the error passes through unchanged
  projection                     K_proj roundings per term: the kernel's chain of one channel (Ho Wo fmas), the 31
                                 additions of the channel partials and the bias: K_proj = Ho Wo + 32 (`order="kernel"`);
                                 a sum of all F + 1 terms in ANY order: K_proj = F + 1 (`order="any"`: library GEMMs)
"""
import numpy as np

from _rescal_ref import FLOOR, SLACK, U, bound, dot, prod  # noqa: F401  (the shared rules)

CHANNELS = 32
DEFECTS = ("swapped_stack", "transposed_image", "bias_from_the_end", "spatial_major", "eps_dropped", "var_without_sqrt",
           "no_relu1", "no_relu2", "flipped_taps", "q0_not_one")


def out_hw(h, w, fs, pad):
    return 2 * h - fs + 2 * pad + 1, w - fs + 2 * pad + 1


def make_tables(E, R, d, seed):
    rng = np.random.default_rng(seed)
    ent = rng.standard_normal((E, d + 1)).astype(np.float32)
    rel = rng.standard_normal((R, d + 1)).astype(np.float32)
    return ent, rel


def make_net(h, w, fs=3, pad=0, bias=True, seed=0):
    """float32 parameters and running statistics of a network whose ReLUs both kill and keep a non-trivial share (the
    statistics of the second norm are those of a sample batch); the running variance of channel 5 is near 0"""
    rng = np.random.default_rng(seed + 1000)
    d = h * w
    Ho, Wo = out_hw(h, w, fs, pad)
    F = CHANNELS * Ho * Wo
    net = dict(h=h, w=w, fs=fs, pad=pad,
               conv_w=(0.5 * rng.standard_normal((CHANNELS, fs, fs))).astype(np.float32),
               conv_b=(0.1 * rng.standard_normal(CHANNELS)).astype(np.float32) if bias else None,
               mean1=(0.3 * rng.standard_normal(CHANNELS)).astype(np.float32),
               var1=rng.uniform(0.5, 1.5, CHANNELS).astype(np.float32), eps1=1e-5,
               proj_w=(rng.standard_normal((d, F)) / np.sqrt(F)).astype(np.float32),
               proj_b=(0.1 * rng.standard_normal(d)).astype(np.float32),
               mean2=np.zeros(d, np.float32), var2=np.ones(d, np.float32), eps2=1e-5)
    net["var1"][5] = 1e-7
    ent, rel = make_tables(16, 16, d, seed + 2000)
    x = _pre_bn2(net, ent, rel, np.arange(16), np.arange(16)[::-1], None, "kernel")[0]
    net["mean2"] = x.mean(0).astype(np.float32)
    net["var2"] = (x.var(0) + 1e-3).astype(np.float32)
    return net


def _rsq(var, eps, defect=None):
    var = np.asarray(var, np.float64)
    if defect == "eps_dropped":
        eps = 0.0
    t = var + eps
    et = U * t
    if defect == "var_without_sqrt":
        return 1.0 / t, et / (t * (t - et)) + U / (t - et)
    r = np.sqrt(t)
    er = et / r + U * (r + et / r)
    return 1.0 / r, er / (r * (r - er)) + U / (r - er)


def _sub(a, ea, b):
    x = a - b
    return x, ea + U * (np.abs(x) + ea)


def _norm_relu(v, ev, mean, var, eps, defect, relu=True):
    x, ex = _sub(v, ev, np.asarray(mean, np.float64))
    y, ey = _rsq(var, eps, defect)
    z, ez = prod(x, ex, y, ey)
    return (np.maximum(z, 0.0) if relu else z), ez


def features(net, ent, rel, s, p, defect=None):
    """(f [n, 32, Ho, Wo], e): the feature map behind the first ReLU"""
    h, w, fs, pad = net["h"], net["w"], net["fs"], net["pad"]
    d = h * w
    e, r = np.asarray(ent, np.float64)[np.asarray(s)], np.asarray(rel, np.float64)[np.asarray(p)]
    if defect == "swapped_stack":
        e, r = r, e
    e, r = (e[:, :d], r[:, :d]) if defect == "bias_from_the_end" else (e[:, 1:], r[:, 1:])
    n = e.shape[0]
    if defect == "transposed_image":
        e, r = (x.reshape(n, w, h).transpose(0, 2, 1) for x in (e, r))
    img = np.concatenate([e.reshape(n, h, w), r.reshape(n, h, w)], 1)
    img = np.pad(img, ((0, 0), (pad, pad), (pad, pad)))
    win = np.lib.stride_tricks.sliding_window_view(img, (fs, fs), axis=(1, 2))  # [n, Ho, Wo, fs, fs]
    cw = np.asarray(net["conv_w"], np.float64)
    if defect == "flipped_taps":
        cw = cw[:, ::-1, ::-1]
    cb = np.zeros(CHANNELS) if net["conv_b"] is None else np.asarray(net["conv_b"], np.float64)
    v = np.einsum("nyxab,cab->ncyx", win, cw) + cb[None, :, None, None]
    ev = fs * fs * U * (np.einsum("nyxab,cab->ncyx", np.abs(win), np.abs(cw)) + np.abs(cb)[None, :, None, None])
    sh = (1, CHANNELS, 1, 1)
    return _norm_relu(v, ev, net["mean1"].reshape(sh), net["var1"].reshape(sh), net["eps1"], defect,
                      relu=defect != "no_relu1")


def _pre_bn2(net, ent, rel, s, p, defect, order):
    f, ef = features(net, ent, rel, s, p, defect)
    n, _, Ho, Wo = f.shape
    if defect == "spatial_major":
        f, ef = f.transpose(0, 2, 3, 1), ef.transpose(0, 2, 3, 1)
    f, ef = f.reshape(n, -1), ef.reshape(n, -1)
    W = np.asarray(net["proj_w"], np.float64)
    b = np.asarray(net["proj_b"], np.float64)
    K = Ho * Wo + CHANNELS if order == "kernel" else f.shape[1] + 1
    x = f @ W.T + b
    ex = ef @ np.abs(W).T + K * U * ((np.abs(f) + ef) @ np.abs(W).T + np.abs(b))
    return x, ex


def queries(net, ent, rel, s, p, defect=None, order="kernel"):
    """(q' [n, d + 1], e): the augmented query rows [1 | x]"""
    x, ex = _pre_bn2(net, ent, rel, s, p, defect, order)
    z, ez = _norm_relu(x, ex, net["mean2"], net["var2"], net["eps2"], defect, relu=defect != "no_relu2")
    one = np.zeros((z.shape[0], 1)) if defect == "q0_not_one" else np.ones((z.shape[0], 1))
    if defect == "bias_from_the_end":
        return np.concatenate([z, one], 1), np.concatenate([ez, 0 * one], 1)
    return np.concatenate([one, z], 1), np.concatenate([0 * one, ez], 1)


def score_sp(net, ent, rel, s, p, targets=None, defect=None, order="kernel"):
    q, eq = queries(net, ent, rel, s, p, defect, order)
    t = np.asarray(ent, np.float64)
    if targets is not None:
        t = t[np.asarray(targets)]
    return dot(q[:, None, :], eq[:, None, :], t[None, :, :], None)


def score_spo(net, ent, rel, s, p, o, defect=None, order="kernel"):
    q, eq = queries(net, ent, rel, s, p, defect, order)
    return dot(q, eq, np.asarray(ent, np.float64)[np.asarray(o)], None)


def shares(net, ent, rel, s, p):
    """(share of features that die at the first ReLU, share of outputs that die at the second)"""
    f = features(net, ent, rel, s, p)[0]
    q = queries(net, ent, rel, s, p)[0][:, 1:]
    return float((f == 0).mean()), float((q == 0).mean())


# the cases of tests/test_gpu_conve.py: (h, w, fs, pad, bias).  The smallest at which each piece can go wrong: (2, 4)
# F = 128 with one output row per image seam; (3, 5) an odd d; (10, 20) the default with F = 10,368; fs = 1 (with pad 2:
# a slice that needs more LDS than a launch gets without asking), fs = 5 with pad 2; pad 1; no conv bias
GPU_CASES = {
    "seam": (2, 4, 3, 0, True),
    "odd_d": (3, 5, 3, 0, True),
    "default": (10, 20, 3, 0, True),
    "fs1": (3, 5, 1, 0, True),
    "fs1_pad2_big_slice": (10, 20, 1, 2, True),
    "fs5_pad2": (3, 5, 5, 2, True),
    "pad1": (3, 5, 3, 1, True),
    "fs2": (3, 5, 2, 0, True),
    "fs4_pad1": (3, 5, 4, 1, True),
    "no_bias": (3, 5, 3, 0, False),
    "seam_no_bias": (2, 4, 3, 0, False),
}
GPU_E, GPU_R = 23, 7


def gpu_case(name, n=40, seed=0):
    """(net, ent, rel, s, p, o) of a named case; rows 0 and n - 1 hold the same (s, p) pair"""
    h, w, fs, pad, bias = GPU_CASES[name]
    net = make_net(h, w, fs, pad, bias, seed)
    ent, rel = make_tables(GPU_E, GPU_R, h * w, seed + 7)
    rng = np.random.default_rng(seed + 11)
    s, p, o = rng.integers(0, GPU_E, n), rng.integers(0, GPU_R, n), rng.integers(0, GPU_E, n)
    s[-1], p[-1] = s[0], p[0]
    return net, ent, rel, s, p, o
