"""kge_ns_loss on the MI355X: LibKGE's negative-sampling losses kl / margin_ranking / soft_margin / se (and the bce
family's kinds 0-2) from one kernel, on a [n, 1 + K] block and on its two pieces, against tests/_ns_loss_ref.py -- the
reference's op sequence built from torch's own modules (pinned to the reference's loss objects by
tests/test_ns_loss_ref_cpu.py) -- in float32 on the GPU and in float64.

Exact comparisons: the margin-ranking gradient (0 / 1 / -count, the hinge decided in torch's float32 order, the exact
tie v = 0 ACTIVE as in torch's clamp_min backward) and the se gradient (2 (x - y)) are torch.equal to float32 torch
autograd through the reference's op sequence on the same scores.

Bounded comparisons (the kl and soft_margin gradients, all four loss values) follow the project's rule (DESIGN.md
sections 15-18): per case the float32 torch op sequence's OWN error against float64 on the same inputs is measured --
err = max |got - want| / max(1, max |want|) -- and the kernel is allowed 4 x that, with half a float32 ulp (2^-24) as the
floor of a measured error.  The float32 sequence gives inf (gradient: nan) on the planted soft-margin row (z = 90): that
row is compared with float64 directly and bounded by the measured error of the finite rows / elements.
Measured on an MI355X over the cases below (float32 torch op sequence -> kernel; worst kernel / max(torch, 2^-24); the
bound 4 x was therefore):
  kl gradient             5.9e-43 .. 2.55e-7 -> at most 2.51e-7;  1.06;  2.38e-7 .. 1.02e-6
  soft_margin gradient    1.2e-25 .. 8.86e-8 (finite elements) -> at most 8.90e-8, planted row included;  1.27;  2.38e-7 .. 3.54e-7
  kl value                0 .. 6.77e-8 -> at most 7.32e-8;  1.23;  2.38e-7 .. 2.71e-7
  margin_ranking value    0 .. 8.08e-8 -> at most 8.08e-8;  1.00;  2.38e-7 .. 3.23e-7
  soft_margin value       2.5e-25 .. 5.59e-8 (finite rows) -> at most 5.82e-8, planted row at most 7.05e-8;  1.18;  2.38e-7
  se value                0 .. 8.04e-8 -> at most 7.68e-8;  1.29;  2.38e-7 .. 3.22e-7
(DESIGN.md section 19); every figure is printed by the tests before it is asserted (pytest -s)."""
import ctypes
import functools

import pytest
import torch

import _ns_loss_ref as nr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24  # half a float32 ulp at the scale the errors are taken relative to: the floor of a measured error

# one negative; the lane edge at 64 / 65 columns; a workgroup (4 rows) with a short row tail (n = 1, 5, 77); several
# workgroups and column rounds; the workload's own width (n = 512, K = 1000)
SHAPES = [(1, 2), (77, 2), (5, 64), (5, 65), (1, 65), (300, 130), (512, 1001)]
MARGINS = [1.0, 0.25]


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


@functools.lru_cache(maxsize=None)
def _scores(n, c, margin=1.0):
    """randn * 6 (saturating on both sides); row 0 planted 40, -40, 90 (past float32 exp overflow for the naive
    soft-margin form); row 1 an exact hinge tie (x_0 = 2, x_1 = 2 - margin: v = 0 in float32); row 2 with no active
    negative (x_0 = 100).  Shared and never modified."""
    g = torch.Generator().manual_seed(n * 1000 + c)
    scores = torch.randn(n, c, generator=g) * 6.0
    scores[0, :min(c, 3)] = torch.tensor([40.0, -40.0, 90.0])[:min(c, 3)]
    if n > 1:
        scores[1, 0], scores[1, 1] = 2.0, 2.0 - margin
    if n > 2:
        scores[2, 0] = 100.0
    return scores


@functools.lru_cache(maxsize=None)
def _refs(kind, n, c, margin=1.0):
    """(float64 loss, float64 gradient [on the GPU], float32 loss, float32 gradient) of the reference's op sequence;
    the float32 one runs on the GPU.  Computed once per case."""
    x = _scores(n, c, margin)
    l64, g64 = nr.loss_and_grad(x.double(), kind, margin)
    l32, g32 = nr.loss_and_grad(x.to(DEV), kind, margin)
    return float(l64), g64.to(DEV), float(l32), g32


def _err(got, want):
    got, want = got.double(), want.double()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1.0))


def _value_check(tag, got, want64, got32):
    e_k, e_32 = abs(got - want64) / max(1.0, abs(want64)), abs(got32 - want64) / max(1.0, abs(want64))
    print(f"VALUE {tag}: float64 {want64:.9g} kernel err {e_k:.3e} float32 torch err {e_32:.3e} bound {4 * max(e_32, EPS):.3e}")
    assert e_k <= 4 * max(e_32, EPS), (tag, e_k, e_32)


@pytest.mark.parametrize("margin", MARGINS)
@pytest.mark.parametrize("n,c", SHAPES)
def test_margin_ranking_gradient_equals_torch_autograd(eng, n, c, margin):
    x = _scores(n, c, margin).to(DEV)
    l64, _, l32, g32 = _refs("margin_ranking", n, c, margin)
    rows, grad = eng.ns_loss(x, "margin_ranking", margin)
    assert torch.equal(grad, g32), int((grad != g32).sum())
    if n > 1:   # the planted tie is active: the positive's gradient counts it
        assert float(grad[1, 1]) == 1.0 and float(grad[1, 0]) == -float((grad[1, 1:] == 1).sum())
    if n > 2:   # no active negative: a row of zeros and a zero loss
        assert not grad[2].any() and float(rows[2]) == 0.0
    _value_check(f"margin_ranking m={margin} n={n} c={c}", float(rows.sum()), l64, l32)


@pytest.mark.parametrize("n,c", SHAPES)
def test_se_gradient_equals_torch_autograd(eng, n, c):
    x = _scores(n, c).to(DEV)
    l64, _, l32, g32 = _refs("se", n, c)
    rows, grad = eng.ns_loss(x, "se")
    assert torch.equal(grad, g32), int((grad != g32).sum())
    _value_check(f"se n={n} c={c}", float(rows.sum()), l64, l32)


@pytest.mark.parametrize("n,c", SHAPES)
def test_kl_against_float64(eng, n, c):
    x = _scores(n, c).to(DEV)
    l64, g64, l32, g32 = _refs("kl", n, c)
    rows, grad = eng.ns_loss(x, "kl")
    e_k, e_32 = _err(grad, g64), _err(g32, g64)
    print(f"GRAD kl n={n} c={c}: kernel err {e_k:.3e} float32 torch err {e_32:.3e} bound {4 * max(e_32, EPS):.3e}")
    assert e_k <= 4 * max(e_32, EPS), (e_k, e_32)
    _value_check(f"kl n={n} c={c}", float(rows.sum()), l64, l32)


@pytest.mark.parametrize("n,c", SHAPES)
def test_soft_margin_against_float64(eng, n, c):
    x_cpu = _scores(n, c)
    x = x_cpu.to(DEV)
    l64, g64, l32, g32 = _refs("soft_margin", n, c)
    rows, grad = eng.ns_loss(x, "soft_margin")
    assert torch.isfinite(rows).all() and torch.isfinite(grad).all()   # the kernel does not overflow
    finite = torch.isfinite(g32)
    assert bool(finite.all()) == (c < 3)   # (the planted 90 is column 2: the float32 sequence's nan)
    e_32 = _err(g32[finite], g64[finite])
    e_k = _err(grad, g64)                  # every element, the planted row's included
    print(f"GRAD soft_margin n={n} c={c}: kernel err {e_k:.3e} float32 torch err (finite elements) {e_32:.3e} "
          f"bound {4 * max(e_32, EPS):.3e}")
    assert e_k <= 4 * max(e_32, EPS), (e_k, e_32)
    if c < 3:
        _value_check(f"soft_margin n={n} c={c}", float(rows.sum()), l64, l32)
        return
    assert l32 == float("inf")
    # the finite rows 1.. against the float32 sequence's own error on them; row 0 against float64 at that bound
    e_fin = 0.0
    if n > 1:
        w64, w32 = float(nr.ns_loss(x_cpu[1:].double(), "soft_margin")), float(nr.ns_loss(x[1:], "soft_margin"))
        e_fin = abs(w32 - w64) / max(1.0, abs(w64))
        _value_check(f"soft_margin rows 1.. n={n} c={c}", float(rows[1:].sum()), w64, w32)
    w0 = float(nr.ns_loss(x_cpu[:1].double(), "soft_margin"))
    e_0 = abs(float(rows[0]) - w0) / max(1.0, abs(w0))
    print(f"VALUE soft_margin planted row n={n} c={c}: float64 {w0:.9g} kernel err {e_0:.3e} bound {4 * max(e_fin, EPS):.3e}")
    assert e_0 <= 4 * max(e_fin, EPS), (e_0, e_fin)


@pytest.mark.parametrize("kind,arg,temperature", [("bce", 0.7, 1.0), ("bce_mean", -1.5, 1.0), ("bce_self_adversarial", 0.3, 0.5)])
@pytest.mark.parametrize("n,c", [(77, 2), (5, 65), (300, 130), (512, 1001)])
def test_bce_kinds_are_bit_equal_to_ns_bce_loss(eng, kind, arg, temperature, n, c):
    x = _scores(n, c).to(DEV)
    rows_a, grad_a = eng.ns_bce_loss(x, kind, arg, temperature)
    rows_b, grad_b = eng.ns_loss(x, kind, arg, temperature)
    assert torch.equal(rows_a, rows_b) and torch.equal(grad_a, grad_b)


KIND_ARGS = [("kl", 0.0), ("margin_ranking", 0.25), ("soft_margin", 0.0), ("se", 0.0), ("bce_self_adversarial", 0.3)]


@pytest.mark.parametrize("kind,arg", KIND_ARGS)
@pytest.mark.parametrize("n,c", [(1, 2), (5, 65), (77, 2), (300, 130)])
def test_parts_strides_and_repeat_runs(eng, kind, arg, n, c):
    """ns_loss_parts on separate tensors -- a strided `pos` (every third element of a vector), a `neg` that is a slice
    of a wider matrix -- is bit-equal to ns_loss on their cat; a strided block (a slice of a wider matrix) too;
    want_grad=False gives the same rows; a second run gives the same bits."""
    x = _scores(n, c, 0.25).to(DEV)
    rows, grad = eng.ns_loss(x, kind, arg, 0.5)
    pos_wide = torch.full((3 * n,), 7.0, device=DEV)
    pos_wide[::3] = x[:, 0]
    neg_wide = torch.full((n, c + 6), -3.0, device=DEV)
    neg_wide[:, 4:3 + c] = x[:, 1:]
    pos, neg = pos_wide[::3], neg_wide[:, 4:3 + c]
    assert n == 1 or (pos.stride(0) == 3 and neg.stride(0) == c + 6)
    r2, g_pos, g_neg = eng.ns_loss_parts(pos, neg, kind, arg, 0.5)
    assert torch.equal(r2, rows) and torch.equal(g_pos, grad[:, 0]) and torch.equal(g_neg, grad[:, 1:])
    r3, none_p, none_n = eng.ns_loss_parts(pos, neg, kind, arg, 0.5, want_grad=False)
    assert none_p is None and none_n is None and torch.equal(r3, rows)
    wide = torch.zeros(n, c + 5, device=DEV)
    wide[:, 2:2 + c] = x
    r4, none = eng.ns_loss(wide[:, 2:2 + c], kind, arg, 0.5, want_grad=False)
    assert none is None and torch.equal(r4, rows)
    r5, g5 = eng.ns_loss(x, kind, arg, 0.5)
    assert torch.equal(r5, rows) and torch.equal(g5, grad)


@pytest.mark.parametrize("kind,arg", KIND_ARGS)
def test_canary_columns_beside_a_strided_gradient_block_are_untouched(eng, kind, arg):
    n, c = 77, 65
    x = _scores(n, c, 0.25).to(DEV)
    rows, grad = eng.ns_loss(x, kind, arg, 0.5)
    canary = 12345.0
    g_wide = torch.full((n, c + 7), canary, device=DEV)      # [canaries 0..2 | g_pos | canary | g_neg | canaries]
    gp_wide = torch.full((2 * n + 1,), canary, device=DEV)   # g_pos on every second element
    r2, g_pos, g_neg = eng.ns_loss_parts(x[:, 0], x[:, 1:], kind, arg, 0.5, g_pos=gp_wide[1::2], g_neg=g_wide[:, 5:4 + c])
    assert torch.equal(r2, rows) and torch.equal(g_neg, grad[:, 1:]) and torch.equal(g_pos, grad[:, 0])
    assert g_neg.data_ptr() == g_wide[:, 5:].data_ptr()
    assert bool((g_wide[:, :5] == canary).all()) and bool((g_wide[:, 4 + c:] == canary).all())
    assert bool((gp_wide[0::2] == canary).all())


def test_invalid_arguments_return_their_status_without_a_launch(eng):
    from kge_amd import _lib
    lib = _lib.lib()
    n, K = 8, 16
    x = _scores(300, 130)[:n, :K + 1].contiguous().to(DEV)
    rows = torch.full((n,), -1.0, device=DEV)
    g = torch.full((n, K + 1), -1.0, device=DEV)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = eng._stream_handle(x.device)
    call = lambda pos=P(x), neg=P(x[:, 1:]), ld=K + 1, nn=n, k=K, kind=3, r=P(rows), gp=P(g), gn=P(g[:, 1:]), gld=K + 1: \
        lib.kge_ns_loss(pos, K + 1, neg, ld, nn, k, kind, 1.0, 1.0, r, gp, K + 1, gn, gld, st)
    assert call(k=0) == -1 and call(kind=7) == -1 and call(kind=-1) == -1
    assert call(pos=None) == -1 and call(neg=None) == -1 and call(r=None) == -1
    assert call(gp=None) == -1 and call(gn=None) == -1 and call(ld=K - 1) == -1 and call(gld=K - 1) == -1
    assert call(nn=0) == 0 and call(nn=0, pos=None, neg=None, r=None, gp=None, gn=None) == 0
    torch.cuda.synchronize()
    assert bool((rows == -1).all()) and bool((g == -1).all())   # nothing ran
    assert call() == 0
    want_rows, want_grad = eng.ns_loss(x, "kl")
    assert torch.equal(rows, want_rows) and torch.equal(g, want_grad)
    with pytest.raises(ValueError):
        eng.ns_loss(x[:, :1], "kl")                 # no negative
    with pytest.raises(ValueError):
        eng.ns_loss(x.double(), "kl")
    with pytest.raises(KeyError):
        eng.ns_loss(x, "hinge")
    with pytest.raises(ValueError):
        eng.ns_loss_parts(x[:, 0], x[:, 1:], "kl", g_pos=g[:, 0])   # half a gradient
