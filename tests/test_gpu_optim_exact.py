"""The optimizer kernels (kge_amd/csrc/optim.hip) on the MI355X against tests/_optim_ref.py, through the C ABI.

The contract: parameters, accumulators and moments carry the BITS of the op-by-op float32 restatement
(-ffp-contract=off, IEEE division and square root, denormals kept), the bf16 copy the bits of the round-to-nearest-even
recipe of common.hpp.  Every comparison below is equality of the uint32 / uint16 views; positions where both sides are
NaN count as equal (a NaN's sign and payload are not part of the contract).  The one bounded comparison is the penalty
term's value: float32 per-thread partials (restated exactly) added in float64 in another order than the kernel's --
non-negative terms, so count * 2^-52 relative.

Every buffer lives in an arena: the arrays of all cases of a test side by side, each 16-byte aligned, at least 8
elements of a sentinel pattern behind each (and in front of the first).  The arena is compared WHOLE with the expected
arena, so a write behind `count`, or into a segment that has no bf16 copy, fails the comparison like a wrong value."""
import numpy as np
import pytest
import torch

import _optim_ref as orf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 8
SENT32 = np.array([0xDEADBEEF], dtype=np.uint32).view(np.float32)[0]  # a normal float32, not a NaN
SENT16 = np.uint16(0xBEEF)
SENT64 = 12345.678

COUNTS = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 1027, 2048, 2051]


@pytest.fixture(scope="module")
def L():
    from kge_amd import _lib
    from kge_amd.engine import _stream
    return _lib, _stream(torch.device(DEV))


# ---- arenas -----------------------------------------------------------------------------------------------------
class Arena:
    """Offsets of `counts` elements each, multiples of 4 elements (16 bytes of float32, 8 bytes of bf16), GUARD
    elements between and around them."""

    def __init__(self, counts):
        self.counts = list(counts)
        self.offs, off = [], GUARD
        for c in self.counts:
            self.offs.append(off)
            off += (c + GUARD + 3) // 4 * 4
        self.total = off

    def pack(self, arrays, dtype, sentinel):
        """arrays[i]: `counts[i]` values, or None (the region keeps the sentinel)."""
        buf = np.full(self.total, sentinel, dtype=dtype)
        for a, c, o in zip(arrays, self.counts, self.offs):
            if a is not None:
                buf[o:o + c] = np.asarray(a, dtype=dtype).reshape(-1)
        return buf

    def f32(self, arrays):
        return torch.from_numpy(self.pack(arrays, np.float32, SENT32)).to(DEV)

    def u16(self):
        return torch.from_numpy(self.pack([None] * len(self.counts), np.uint16, SENT16).view(np.int16)).to(DEV)

    def ptr(self, t, i):
        return t.data_ptr() + self.offs[i] * t.element_size()


def _bits_equal(got, want, what):
    """got: device tensor (float32 or int16); want: numpy array (float32 or uint16).  Bit equality, NaN == NaN."""
    if want.dtype == np.float32:
        g = got.cpu().numpy()
        gb, wb = g.view(np.uint32), want.view(np.uint32)
        ok = (gb == wb) | (np.isnan(g) & np.isnan(want))
    else:
        gb, wb = got.cpu().numpy().view(np.uint16), want
        as_f = lambda b: (b.astype(np.uint32) << np.uint32(16)).view(np.float32)
        ok = (gb == wb) | (np.isnan(as_f(gb)) & np.isnan(as_f(wb)))
    if not ok.all():
        bad = np.flatnonzero(~ok)
        raise AssertionError(f"{what}: {bad.size} of {ok.size} words differ, first at {bad[0]}: got {gb[bad[0]]:#x} "
                             f"want {wb[bad[0]]:#x}")


class Case:
    """One table: inputs, hyper-parameters, whether it has a bf16 copy, and (penalty launches) its penalty."""

    def __init__(self, p, g, s, minus_clr=-0.05, wd=0.0, eps=1e-10, copy=True, kind=0, pp=0, weight=0.0, row_dim=0):
        self.p, self.g, self.s = (np.asarray(x, dtype=np.float32) for x in (p, g, s))
        self.n = self.p.size
        self.minus_clr, self.wd, self.eps, self.copy = minus_clr, wd, eps, copy
        self.kind, self.pp, self.weight, self.row_dim = kind, pp, weight, row_dim


def _run_adagrad(L, cases, api):
    """api: "single" (kge_adagrad_step per case), "multi" (kge_adagrad_step_multi, eight cases per launch), "pen"
    (kge_adagrad_step_multi_penalty, eight per launch).  Compares param, sum, copy arenas with the restatement of every
    case under ITS OWN arguments, and (pen) the value slots."""
    lib, st = L
    ar = Arena([c.n for c in cases])
    P, G, S, C = ar.f32([c.p for c in cases]), ar.f32([c.g for c in cases]), ar.f32([c.s for c in cases]), ar.u16()
    V = torch.full((len(cases) + 2 * GUARD,), SENT64, dtype=torch.float64, device=DEV)
    for i, c in enumerate(cases):
        if c.kind != 0:
            V[GUARD + i] = 0.0
    want = [orf.adagrad_penalty(c.p, c.g, c.s, c.minus_clr, c.wd, c.eps, c.kind, c.pp, c.weight, c.row_dim)
            if api == "pen" else orf.adagrad(c.p, c.g, c.s, c.minus_clr, c.wd, c.eps) + (0.0,) for c in cases]
    segs = [lib.KgeAdagradSeg(ar.ptr(P, i), ar.ptr(G, i), ar.ptr(S, i), ar.ptr(C, i) if c.copy else None, c.n,
                              c.minus_clr, c.wd, c.eps) for i, c in enumerate(cases)]
    pens = [lib.KgePenaltySeg(c.kind, c.pp, c.weight, c.row_dim,
                              V.data_ptr() + 8 * (GUARD + i) if c.kind != 0 else None) for i, c in enumerate(cases)]
    if api == "single":
        for s_ in segs:
            lib.check(lib.lib().kge_adagrad_step(s_.param, s_.grad, s_.state_sum, s_.count, s_.minus_clr,
                                                 s_.weight_decay, s_.eps, s_.bf16_copy, st), "kge_adagrad_step")
    else:
        for i in range(0, len(segs), 8):
            n = len(segs[i:i + 8])
            sa = (lib.KgeAdagradSeg * n)(*segs[i:i + 8])
            if api == "multi":
                lib.check(lib.lib().kge_adagrad_step_multi(sa, n, st), "kge_adagrad_step_multi")
            else:
                lib.check(lib.lib().kge_adagrad_step_multi_penalty(sa, (lib.KgePenaltySeg * n)(*pens[i:i + 8]), n, st),
                          "kge_adagrad_step_multi_penalty")
    torch.cuda.synchronize()
    _bits_equal(P, ar.pack([w[0] for w in want], np.float32, SENT32), f"{api}: param")
    _bits_equal(S, ar.pack([w[1] for w in want], np.float32, SENT32), f"{api}: sum")
    _bits_equal(G, ar.pack([c.g for c in cases], np.float32, SENT32), f"{api}: grad (read only)")
    _bits_equal(C, ar.pack([orf.bf16_rne_bits(w[0]) if c.copy else None for w, c in zip(want, cases)], np.uint16,
                           SENT16), f"{api}: bf16 copy")
    v = V.cpu().numpy()
    for i, (w, c) in enumerate(zip(want, cases)):
        if api == "pen" and c.kind != 0:
            assert abs(v[GUARD + i] - w[2]) <= c.n * 2.0 ** -52 * w[2], (i, c.kind, c.pp, v[GUARD + i], w[2])
            v[GUARD + i] = SENT64
    assert (v == SENT64).all(), "a value slot of a segment without a penalty, or a guard slot, was written"


def _run_adam(L, cases, beta1, beta2, step):
    """cases: (p, g, m1, m2, wd, eps, copy); one kge_adam_step each."""
    lib, st = L
    lr = 0.05
    step_size, bc2_sqrt = lr / (1.0 - beta1 ** step), (1.0 - beta2 ** step) ** 0.5
    ar = Arena([len(c[0]) for c in cases])
    P, G, A, B = (ar.f32([c[k] for c in cases]) for k in range(4))
    C = ar.u16()
    want = [orf.adam(c[0], c[1], c[2], c[3], step_size, bc2_sqrt, beta1, beta2, c[4], c[5]) for c in cases]
    for i, c in enumerate(cases):
        lib.check(lib.lib().kge_adam_step(ar.ptr(P, i), ar.ptr(G, i), ar.ptr(A, i), ar.ptr(B, i), len(c[0]), step_size,
                                          bc2_sqrt, beta1, beta2, c[4], c[5], ar.ptr(C, i) if c[6] else None, st),
                  "kge_adam_step")
    torch.cuda.synchronize()
    for k, (t, name) in enumerate(((P, "param"), (A, "exp_avg"), (B, "exp_avg_sq"))):
        _bits_equal(t, ar.pack([w[k] for w in want], np.float32, SENT32), f"adam: {name}")
    _bits_equal(G, ar.pack([c[1] for c in cases], np.float32, SENT32), "adam: grad (read only)")
    _bits_equal(C, ar.pack([orf.bf16_rne_bits(w[0]) if c[6] else None for w, c in zip(want, cases)], np.uint16, SENT16),
                "adam: bf16 copy")


def _normal(rng, n, scale=1.0):
    return (scale * rng.standard_normal(n)).astype(np.float32)


# ---- counts and paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("api,kind,pp", [("single", 0, 0), ("multi", 0, 0), ("pen", 0, 0), ("pen", 1, 1), ("pen", 1, 2),
                                         ("pen", 1, 3)])
def test_adagrad_every_count_with_and_without_copy(L, api, kind, pp, wd):
    """Whole blocks, one element more or less, pure scalar tails, body + tail: 12 counts x (copy, no copy); in the multi
    launches these are 24 segments in three launches of eight, so block-aligned counts (1024, 2048) sit in front of
    other segments."""
    rng = np.random.default_rng(10 + pp)
    cases = []
    for j, n in enumerate(COUNTS + COUNTS[::-1]):
        p = _normal(rng, n)
        p[::5] = 0.0
        p[1::7] = -0.0
        cases.append(Case(p, _normal(rng, n, 0.3), np.abs(_normal(rng, n)), minus_clr=-0.05, wd=wd, eps=1e-10,
                          copy=j < len(COUNTS), kind=kind, pp=pp, weight=0.02 * (j + 1), row_dim=8))
    _run_adagrad(L, cases, api)


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_adam_every_count_with_and_without_copy(L, wd):
    rng = np.random.default_rng(20)
    cases = [(_normal(rng, n), _normal(rng, n, 0.3), _normal(rng, n, 0.1), np.abs(_normal(rng, n, 0.01)), wd, 1e-8,
              j < len(COUNTS)) for j, n in enumerate(COUNTS + COUNTS[::-1])]
    _run_adam(L, cases, 0.9, 0.99, 3)


# ---- value edges ------------------------------------------------------------------------------------------------
F = np.float32
NAN, INF = F(np.nan), F(np.inf)
EDGE_G = [0.0, -0.0, 1e-20, -1e-20, 1e-30, 1e20, -1e20, INF, -INF, NAN, 0.37, 1e19]
# g*g: 0, 0, subnormal 1e-40 (kept), the same, underflow to 0, inf, inf, inf, inf, NaN, normal, 1e38 (inf with sum 3.4e38)
EDGE_P = [1.5, -0.0, 0.0, 1e-40, -1.4e-45, 3e38]   # normal, -0, 0, subnormal, the smallest subnormal, near FLT_MAX
EDGE_S = [0.0, 1.0, 3.4e38, 1e-40]                 # 0 (0/0 with g = 0, eps = 0), normal, near FLT_MAX, subnormal


def _grid(*axes):
    g = np.meshgrid(*[np.array(a, dtype=np.float32) for a in axes], indexing="ij")
    return [x.reshape(-1) for x in g]


def _body_and_tails(arrays):
    """Every combination in a four-element body (one case, padded to a multiple of four by repeating the start), and
    every combination again in a scalar tail: cases of three elements."""
    n = arrays[0].size
    body = [np.concatenate([a, a[:(-n) % 4]]) for a in arrays]
    out = [body]
    for j in range(0, n, 3):
        idx = np.arange(j, j + 3) % n
        out.append([a[idx] for a in arrays])
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("eps", [1e-10, 0.0])
@pytest.mark.parametrize("api", ["single", "multi", "pen"])
def test_adagrad_value_edges_in_body_and_tail(L, api, eps, wd):
    """Zero over zero, subnormal and vanishing and overflowing squares, inf and NaN gradients, an accumulator near
    FLT_MAX, subnormal and -0 parameters: the kernel and numpy's IEEE float32 give the same bits (NaN where numpy
    gives NaN)."""
    cases = [Case(p, g, s, minus_clr=-0.05, wd=wd, eps=eps, copy=True) for p, g, s in
             _body_and_tails(_grid(EDGE_P, EDGE_G, EDGE_S))]
    assert cases[0].n % 4 == 0 and all(c.n == 3 for c in cases[1:])
    _run_adagrad(L, cases, api)


@pytest.mark.parametrize("wd", [0.0, 1e-3])
@pytest.mark.parametrize("eps", [1e-8, 0.0])
@pytest.mark.parametrize("beta1", [0.9, 0.3])
def test_adam_value_edges_in_body_and_tail(L, beta1, eps, wd):
    """The gradient edges above against first moments 0 / normal / subnormal and second moments 0 (g = 0, eps = 0:
    0/0) / normal / near FLT_MAX / subnormal."""
    grid = _grid([1.5, -0.0, 1e-40, 3e38], EDGE_G, [0.0, 0.1, -1e-40], [0.0, 1.0, 3.4e38, 1e-40])
    cases = [(p, g, a, b, wd, eps, True) for p, g, a, b in _body_and_tails(grid)]
    _run_adam(L, cases, beta1, 0.999, 2)


# ---- the bf16 copy over every rounding case -----------------------------------------------------------------------
def _all_bf16_roundings():
    hi = np.arange(65536, dtype=np.uint32) << np.uint32(16)
    lo = np.array([0x0000, 0x0001, 0x7fff, 0x8000, 0x8001, 0xffff], dtype=np.uint32)
    return (hi[:, None] | lo[None, :]).reshape(-1).view(np.float32)


HARD = np.array([0x3f808000, 0x3f818000, 0x3f808001,    # ties: to even down, to even up; just above a tie
                 0x3f807fff, 0x3fffffff, 0x7f7fffff,    # just below; carry into the exponent; overflow to inf
                 0x00008000, 0x00018000, 0x00008001,    # bf16 subnormals: tie to 0, tie up to 2, above the tie
                 0x00000001, 0x0000ffff, 0x007fffff,    # float32 subnormals
                 0x80000000, 0x80008000, 0xff7fffff,    # -0, a negative subnormal tie, overflow to -inf
                 0x7f800000, 0xff800000, 0x00000000,    # +-inf, +0
                 0x7fc00000, 0x7f800001, 0xffffffff,    # NaNs (payload only in the low half: still a NaN)
                 0x7f7f8000, 0x807f8000, 0x3f7fffff],   # tie up into inf; subnormal tie up to the smallest normal; 1 - ulp
                dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("api", ["single", "multi", "pen", "adam"])
def test_bf16_copy_of_every_rounding_case_vector_and_tail_path(L, api):
    """grad = 0 with sum = 1 (Adam: moments 0 and 1) leaves the parameter as it is, -0 included, so the copy is
    the kernel's bf16 rounding of a CHOSEN float32: all 65536 upper halves x 6 lower halves through the vector path
    (393216 elements, no tail), and the hardest patterns three at a time through the scalar tail."""
    sweep = _all_bf16_roundings()
    assert sweep.size == 393216
    arrays = [sweep] + [HARD[j:j + 3] for j in range(0, HARD.size, 3)] + [np.concatenate([sweep[:1024], HARD[:3]])]
    zeros, ones = (lambda a: np.zeros(a.size, np.float32)), (lambda a: np.ones(a.size, np.float32))
    if api == "adam":
        _run_adam(L, [(a, zeros(a), zeros(a), ones(a), 0.0, 1e-8, True) for a in arrays], 0.9, 0.999, 1)
    else:
        _run_adagrad(L, [Case(a, zeros(a), ones(a), minus_clr=-0.1, wd=0.0, eps=1e-10, copy=True) for a in arrays], api)
    # (what the run compared the copy with is the rounding of the UNCHANGED parameter)
    w = orf.adagrad(HARD, np.zeros(HARD.size), np.ones(HARD.size), -0.1, 0.0, 1e-10)[0]
    ok = (w.view(np.uint32) == HARD.view(np.uint32)) | np.isnan(HARD)
    assert ok.all()


# ---- multi launch: per-segment arguments ------------------------------------------------------------------------
def test_multi_launch_every_segment_under_its_own_arguments(L):
    """Eight segments, no two with the same minus_clr / weight_decay / eps, boundaries on whole blocks (1024, 2048 in
    front of other segments), empty segments in the middle, the bf16 copy on every other one."""
    rng = np.random.default_rng(30)
    counts = [1024, 0, 1, 2048, 1025, 0, 3, 1027]
    mclr = [-0.05, -0.9, -0.011, -0.3, -0.0007, -0.6, -0.123, -0.02]
    wds = [0.0, 1e-3, 0.02, 0.0, 5e-4, 0.0, 0.3, 0.0]
    epss = [1e-10, 1e-3, 0.0, 1e-6, 0.5, 1e-10, 1e-8, 2e-4]
    cases = [Case(_normal(rng, n), _normal(rng, n, 0.3), np.abs(_normal(rng, n)), minus_clr=m, wd=w, eps=e,
                  copy=j % 2 == 0) for j, (n, m, w, e) in enumerate(zip(counts, mclr, wds, epss))]
    _run_adagrad(L, cases, "multi")


def test_penalty_launch_every_segment_under_its_own_penalty(L):
    """One launch: no penalty, lp with p = 1, 2, 3, n3 over rows of 8 and of 24 columns, an empty segment; every
    segment its own weight, value slot and hyper-parameters.  lp counts end in a scalar tail; n3: count / 2 = 1200 and
    1080 real parts (not multiples of a workgroup's 1024), 300 and 90 rows, with row_dim 8 every quad of real parts is
    followed directly by its imaginary quad.  Exact zeros and -0 among the parameters (whole complex pairs too:
    |z| = 1e-7)."""
    rng = np.random.default_rng(31)
    spec = [  # (count, kind, p, weight, row_dim, minus_clr, wd, eps)
        (1027, 0, 0, 0.0, 0, -0.05, 0.0, 1e-10),
        (1027, 1, 1, 0.013, 0, -0.3, 1e-3, 1e-6),
        (0, 1, 2, 0.5, 0, -0.1, 0.0, 1e-10),
        (2051, 1, 2, 0.4, 0, -0.011, 0.0, 1e-3),
        (300 * 8, 2, 3, 0.07, 8, -0.2, 5e-4, 1e-10),
        (7, 1, 3, 1.5, 0, -0.6, 0.02, 0.0),
        (90 * 24, 2, 3, 0.9, 24, -0.02, 0.0, 1e-8),
        (1025, 1, 3, 0.21, 0, -0.123, 0.0, 2e-4),
    ]
    cases = []
    for j, (n, kind, pp, w, rd, m, wd, e) in enumerate(spec):
        p = _normal(rng, n)
        p[::5] = 0.0
        p[1::7] = -0.0
        if kind == 2:
            rows = p.reshape(-1, rd)
            rows[1, :] = 0.0           # a row of zero pairs
            rows[2, :rd // 2] = -0.0   # real parts -0 ...
            rows[2, rd // 2:] = 0.0    # ... with imaginary parts 0
        cases.append(Case(p, _normal(rng, n, 0.1), np.abs(_normal(rng, n)), minus_clr=m, wd=wd, eps=e,
                          copy=j % 2 == 1, kind=kind, pp=pp, weight=w, row_dim=rd))
    _run_adagrad(L, cases, "pen")


# ---- rows -------------------------------------------------------------------------------------------------------
def _table(rows, ld, dim, values, dtype, sentinel):
    """[rows, ld] with `values` in the first `dim` columns, the sentinel in the pad columns and in GUARD elements
    behind the last row."""
    buf = np.full(rows * ld + GUARD, sentinel, dtype=dtype)
    buf[:rows * ld].reshape(rows, ld)[:, :dim] = values
    return buf


def _run_rows(L, P0, G0, S0, ids, lds, minus_clr=-0.05, eps=1e-10, copy=True):
    lib, st = L
    E, dim = P0.shape
    nr = len(ids)
    ld_p, ld_g, ld_s, ld_c = lds
    C0 = orf.bf16_rne_bits(P0).reshape(E, dim)  # a fresh copy, as the optimizer keeps it
    dev = lambda a: torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(DEV)
    P, G, S = dev(_table(E, ld_p, dim, P0, np.float32, SENT32)), dev(_table(nr, ld_g, dim, G0, np.float32, SENT32)), \
        dev(_table(E, ld_s, dim, S0, np.float32, SENT32))
    C = dev(_table(E, ld_c, dim, C0, np.uint16, SENT16))
    R = torch.from_numpy(np.concatenate([np.asarray(ids, dtype=np.int64), np.full(GUARD, -1, dtype=np.int64)])).to(DEV)
    lib.check(lib.lib().kge_adagrad_step_rows(P.data_ptr(), ld_p, G.data_ptr(), ld_g, S.data_ptr(), ld_s, R.data_ptr(),
                                              nr, dim, minus_clr, eps, C.data_ptr() if copy else None,
                                              ld_c if copy else 0, st), "kge_adagrad_step_rows")
    torch.cuda.synchronize()
    if nr and dim:
        wp, ws = orf.adagrad_rows(P0, G0, S0, ids, minus_clr, eps)
    else:
        wp, ws = P0, S0
    wc = C0.copy()
    if copy and nr and dim:
        wc[ids] = orf.bf16_rne_bits(wp[ids]).reshape(nr, dim)
    tag = f"rows dim={dim} nr={nr} lds={lds}"
    # touched rows: the restatement's bits; every other row, every pad column, the guards: the bits they had
    _bits_equal(P, _table(E, ld_p, dim, wp, np.float32, SENT32), tag + " param")
    _bits_equal(S, _table(E, ld_s, dim, ws, np.float32, SENT32), tag + " sum")
    _bits_equal(G, _table(nr, ld_g, dim, G0, np.float32, SENT32), tag + " grad (read only)")
    _bits_equal(C, _table(E, ld_c, dim, wc, np.uint16, SENT16), tag + " bf16 copy")


def _row_ids(rng, nr, E):
    """Unsorted unique ids with row 0 and the last row (nr = 1: the last row; row 0 is the caller's second run)."""
    if nr == 1:
        return np.array([E - 1])
    ids = np.concatenate([[E - 1, 0], 1 + rng.permutation(E - 2)[:nr - 2]])
    ids = ids[rng.permutation(nr)]
    if nr > 2 and (np.diff(ids) > 0).all():
        ids = ids[::-1].copy()
    return ids


@pytest.mark.parametrize("nr", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("dim", [1, 63, 64, 65, 130])
def test_rows_every_leading_dimension_touched_and_untouched(L, dim, nr):
    """One wave per listed row, 64 columns per round: dim below / at / above a round and over two, row counts around
    the four rows of a workgroup; the leading dimensions of param, gradient rows, sum and copy each at dim and at
    dim + 3, in all 16 combinations."""
    rng = np.random.default_rng(40 + dim + 1000 * nr)
    E = nr + 4
    P0 = _normal(rng, E * dim).reshape(E, dim)
    P0[:, ::5] = -0.0
    S0 = np.abs(_normal(rng, E * dim)).reshape(E, dim)
    G0 = _normal(rng, nr * dim, 0.3).reshape(nr, dim)
    for k in range(16):
        lds = tuple(dim + 3 * ((k >> b) & 1) for b in range(4))
        ids = _row_ids(rng, nr, E)
        if nr == 1 and k % 2:
            ids = np.array([0])
        _run_rows(L, P0, G0, S0, ids, lds, copy=k != 5)


def test_rows_nothing_to_do_writes_nothing(L):
    rng = np.random.default_rng(41)
    E, dim = 6, 10
    P0, S0 = _normal(rng, E * dim).reshape(E, dim), np.abs(_normal(rng, E * dim)).reshape(E, dim)
    _run_rows(L, P0, np.zeros((0, dim), np.float32), S0, np.zeros(0, np.int64), (dim, dim, dim, dim))       # num_rows = 0
    _run_rows(L, P0[:, :0], np.zeros((3, 0), np.float32), S0[:, :0], np.array([5, 0, 2]), (3, 3, 3, 3))     # dim = 0


def test_rows_bf16_copy_of_the_hardest_roundings_and_value_edges(L):
    """The rows kernel rounds every element through the scalar form of the pack: the hardest patterns as a parameter
    row (grad 0, sum 1), and the gradient / accumulator edges as another."""
    p, g, s = _grid(EDGE_P, EDGE_G, EDGE_S)
    dim = p.size
    hard = np.resize(HARD, dim)
    P0 = np.stack([hard, p, hard])
    G0 = np.stack([g, np.zeros(dim, np.float32)])
    S0 = np.stack([np.ones(dim, np.float32), s, np.ones(dim, np.float32)])
    for eps in (1e-10, 0.0):
        _run_rows(L, P0, G0, S0, np.array([1, 0]), (dim + 3, dim, dim + 3, dim), eps=eps)


# ---- through the classes: parameters and gradients that are views at an odd element offset ------------------------
def _misaligned(shape, seed):
    """A contiguous tensor of `shape` that starts one element into a flat buffer: data_ptr() % 16 == 4."""
    n = int(np.prod(shape))
    flat = torch.randn(n + 8, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))
    v = flat[1:1 + n].view(shape)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("which", ["param", "grad"])
@pytest.mark.parametrize("name", ["adagrad", "adam"])
def test_classes_hand_a_misaligned_view_to_torch_and_keep_the_rest_on_the_kernel(name, which):
    """The C ABI refuses pointers that are not 16-byte aligned; the classes must not hand such a parameter (or one
    with such a gradient) to it but to torch's own update, as for every parameter the kernel does not cover -- and the
    aligned parameters of the same optimizer stay on the kernel (their bf16 copy is there)."""
    from kge_amd.optim import Adagrad, Adam, bf16_copy_of
    torch.manual_seed(7)
    shape = (6, 5)
    odd0 = _misaligned(shape, 1).clone() if which == "grad" else _misaligned(shape, 1)
    got = [torch.randn(33, 8, device=DEV).requires_grad_(True), torch.nn.Parameter(odd0),
           torch.randn(9, 4, device=DEV).requires_grad_(True)]
    assert (got[1].data_ptr() % 16 == 4) == (which == "param")
    ref = [g.detach().clone().requires_grad_(True) for g in got]
    if name == "adagrad":
        o_ref = torch.optim.Adagrad(ref, lr=0.1, weight_decay=1e-3, eps=1e-10)
        o_got = Adagrad(got, lr=0.1, weight_decay=1e-3, eps=1e-10, bf16_copies=True)
        tol = dict(rtol=2e-6, atol=1e-7)      # tests/test_gpu_optim.py: test_adagrad_matches_torch
    else:
        o_ref = torch.optim.Adam(ref, lr=0.05, betas=(0.9, 0.99), eps=1e-8)
        o_got = Adam(got, lr=0.05, betas=(0.9, 0.99), eps=1e-8, bf16_copies=True)
        tol = dict(rtol=5e-6, atol=2e-6)      # tests/test_gpu_optim.py: test_adam_matches_torch
    for step in range(3):
        for r, g in zip(ref, got):
            grad = torch.randn_like(r)
            r.grad, g.grad = grad.clone(), grad.clone()
        if which == "grad":
            buf = _misaligned(shape, 100 + step)
            buf.copy_(got[1].grad)
            got[1].grad = buf
            assert got[1].grad.data_ptr() % 16 == 4
        before = got[1].detach().clone()
        o_got.step()
        o_ref.step()
        assert not torch.equal(got[1].detach(), before)  # stepped
        for r, g in zip(ref, got):
            torch.testing.assert_close(g.detach(), r.detach(), **tol)
        assert bf16_copy_of(got[1]) is None
        for g in (got[0], got[2]):
            c = bf16_copy_of(g)
            assert c is not None and torch.equal(c, g.detach().to(torch.bfloat16))


def test_misaligned_parameter_with_a_fused_penalty_is_refused_by_name():
    from kge_amd.optim import Adagrad
    torch.manual_seed(8)
    p = torch.nn.Parameter(_misaligned((6, 8), 2))
    q = torch.randn(4, 8, device=DEV).requires_grad_(True)
    opt = Adagrad([p, q], lr=0.1)
    opt.set_penalty(p, "lp", 2, 0.1)
    p.grad, q.grad = torch.randn_like(p), torch.randn_like(q)
    with pytest.raises(RuntimeError, match="left the kernel path"):
        opt.step()
