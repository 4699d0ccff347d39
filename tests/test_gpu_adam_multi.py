"""kge_adam_step_multi (kge_amd/csrc/optim.hip: adam_clock_kernel + adam_multi_kernel) on the MI355X against
tests/_adam_multi_ref.py, through the C ABI, and kge_amd.optim.Adam(device_step=True) under GraphedStep.

The contract is the one of tests/test_gpu_optim_exact.py (whose arena helpers are used here): parameters, moments, the
bf16 copy AND the 32-byte clock records carry the BITS of the restatement -- the clock's float64 products, the IEEE
float64 division and square root and their rounding to float32 included.  The one bounded comparison is the penalty
term's value: float32 per-thread partials (restated exactly) added in float64 in another order than the kernel's,
non-negative terms, so count * 2^-52 relative (derived there).

Arenas: all arrays of a test side by side, 16-byte aligned, sentinels between and around them, compared WHOLE; the
clock records sit in an int64 arena with sentinel words around every record, the value slots in a float64 one."""
import struct

import numpy as np
import pytest
import torch

import _adam_multi_ref as amr
import _optim_ref as orf
from test_gpu_optim_exact import GUARD, SENT16, SENT32, SENT64, Arena, _bits_equal, _normal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTQ = 0x5A5A5A5A5A5A5A5A
REC = 4 + 2  # int64 words per clock slot: the record and two sentinel words behind it


@pytest.fixture(scope="module")
def L():
    from kge_amd import _lib
    from kge_amd.engine import _stream
    return _lib, _stream(torch.device(DEV))


class Case:
    def __init__(self, p, g, a, b, lr=0.05, beta1=0.9, beta2=0.99, wd=0.0, eps=1e-8, copy=True, T=0, kind=0, pp=0,
                 weight=0.0, row_dim=0):
        self.p, self.g, self.a, self.b = (np.asarray(x, dtype=np.float32) for x in (p, g, a, b))
        self.n = self.p.size
        self.lr, self.beta1, self.beta2, self.wd, self.eps, self.copy, self.T = lr, beta1, beta2, wd, eps, copy, T
        self.kind, self.pp, self.weight, self.row_dim = kind, pp, weight, row_dim


def _clock_arena(clocks):
    """int64 words: a sentinel word, then per record its four words and two sentinel words."""
    buf = np.full(1 + REC * len(clocks), SENTQ, dtype=np.int64)
    for i, c in enumerate(clocks):
        buf[1 + REC * i:1 + REC * i + 4] = np.frombuffer(amr.clock_bytes(c), dtype=np.int64)
    return buf


class Run:
    """The device state of a list of cases and what the restatement expects of it; `launch()` steps both."""

    def __init__(self, L, cases, pens=False):
        self.lib, self.st = L
        self.cases, self.pens = cases, pens
        ar = self.ar = Arena([c.n for c in cases])
        self.P, self.G, self.A, self.B = (ar.f32([getattr(c, k) for c in cases]) for k in "pgab")
        self.C = ar.u16()
        self.want = [(c.p.reshape(-1), c.a.reshape(-1), c.b.reshape(-1)) for c in cases]
        self.stepped = [False] * len(cases)
        self.clocks = [amr.clock_seed(c.T, c.beta1, c.beta2) for c in cases]
        self.K = torch.from_numpy(_clock_arena(self.clocks)).to(DEV)
        self.V = torch.full((len(cases) + 2 * GUARD,), SENT64, dtype=torch.float64, device=DEV)
        self.values = [None] * len(cases)

    def clock_ptr(self, i):
        return self.K.data_ptr() + 8 * (1 + REC * i)

    def seg(self, i):
        c, ar = self.cases[i], self.ar
        return self.lib.KgeAdamSeg(ar.ptr(self.P, i), ar.ptr(self.G, i), ar.ptr(self.A, i), ar.ptr(self.B, i),
                                   ar.ptr(self.C, i) if c.copy else None, self.clock_ptr(i), c.n, c.lr, c.beta1,
                                   c.beta2, c.wd, c.eps)

    def launch(self):
        lib, cases = self.lib, self.cases
        for i, c in enumerate(cases):
            if self.pens and c.kind != 0:
                self.V[GUARD + i] = 0.0
        for i0 in range(0, len(cases), 8):
            idx = list(range(i0, min(i0 + 8, len(cases))))
            segs = (lib.KgeAdamSeg * len(idx))(*[self.seg(i) for i in idx])
            pens = None
            if self.pens:
                pens = (lib.KgePenaltySeg * len(idx))(*[lib.KgePenaltySeg(
                    cases[i].kind, cases[i].pp, cases[i].weight, cases[i].row_dim,
                    self.V.data_ptr() + 8 * (GUARD + i) if cases[i].kind != 0 else None) for i in idx])
            lib.check(lib.lib().kge_adam_step_multi(segs, pens, len(idx), self.st), "kge_adam_step_multi")
        for i, c in enumerate(cases):
            if c.n == 0:
                continue  # an empty segment: nothing moves, its clock included
            w = self.want[i]
            pen = (c.kind, c.pp, c.weight, c.row_dim) if self.pens else (0, 0, 0.0, 0)
            p, a, b, v, self.clocks[i] = amr.adam_multi_segment(w[0], c.g, w[1], w[2], self.clocks[i], c.lr, c.beta1,
                                                                c.beta2, c.wd, c.eps, *pen)
            self.want[i], self.values[i], self.stepped[i] = (p, a, b), v, True

    def check_clocks(self, what=""):
        got = self.K.cpu().numpy()
        want = _clock_arena(self.clocks)
        if not (got == want).all():
            bad = int(np.flatnonzero(got != want)[0])
            i, word = divmod(bad - 1, REC)
            raise AssertionError(f"{what}: clock arena word {bad} (record {i}, word {word}): got {got[bad]:#x} want "
                                 f"{want[bad]:#x}; record got {struct.unpack('<qddff', got[1 + REC * i:][:4].tobytes())} "
                                 f"want {self.clocks[i]}")

    def check(self, what=""):
        torch.cuda.synchronize()
        ar, cases = self.ar, self.cases
        for k, (t, name) in enumerate(((self.P, "param"), (self.A, "exp_avg"), (self.B, "exp_avg_sq"))):
            _bits_equal(t, ar.pack([w[k] for w in self.want], np.float32, SENT32), f"{what}: {name}")
        _bits_equal(self.G, ar.pack([c.g for c in cases], np.float32, SENT32), f"{what}: grad (read only)")
        _bits_equal(self.C, ar.pack([orf.bf16_rne_bits(w[0]) if c.copy and s else None
                                     for w, c, s in zip(self.want, cases, self.stepped)], np.uint16, SENT16),
                    f"{what}: bf16 copy")
        self.check_clocks(what)
        v = self.V.cpu().numpy()
        for i, c in enumerate(cases):
            if self.pens and c.kind != 0:
                w = self.values[i] if c.n else 0.0
                assert abs(v[GUARD + i] - w) <= c.n * 2.0 ** -52 * w, (what, i, c.kind, c.pp, v[GUARD + i], w)
                v[GUARD + i] = SENT64
        assert (v == SENT64).all(), "a value slot of a segment without a penalty, or a guard slot, was written"


def _case(rng, n, **kw):
    p = _normal(rng, n)
    p[::5] = 0.0
    p[1::7] = -0.0
    return Case(p, _normal(rng, n, 0.3), _normal(rng, n, 0.1), np.abs(_normal(rng, n, 0.01)), **kw)


COUNTS = [0, 1, 3, 4, 5, 1023, 1024, 1025, 2500]


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_every_count_with_and_without_copy(L, wd):
    """Empty, pure scalar tails, whole blocks and one element around them, body + tail over several blocks: 9 counts x
    (copy, no copy) = 18 segments in three launches, so block-aligned counts sit in front of other segments; two steps,
    the second from moments and clocks the first one left."""
    rng = np.random.default_rng(50)
    cases = [_case(rng, n, wd=wd, copy=j < len(COUNTS)) for j, n in enumerate(COUNTS + COUNTS[::-1])]
    run = Run(L, cases)
    run.launch()
    run.check("step 1")
    run.launch()
    run.check("step 2")


def test_eight_segments_under_their_own_arguments_and_an_empty_one_between(L):
    rng = np.random.default_rng(51)
    counts = [1024, 3, 2048, 0, 1025, 1, 2500, 1027]
    lrs = [0.05, 1e-3, 0.2, 0.7, 0.011, 0.3, 2e-4, 0.09]
    b1s = [0.9, 0.5, 0.8, 0.3, 0.95, 0.0, 0.99, 0.7]
    b2s = [0.999, 0.9999, 0.99, 0.5, 0.9, 0.98, 0.0, 0.95]
    wds = [0.0, 1e-3, 0.02, 0.0, 5e-4, 0.0, 0.3, 0.0]
    epss = [1e-8, 1e-3, 0.0, 1e-6, 0.5, 1e-10, 1e-8, 2e-4]
    Ts = [0, 7, 0, 5, 1000, 0, 3, 0]
    cases = [_case(rng, n, lr=lr, beta1=b1, beta2=b2, wd=wd, eps=e, copy=j % 2 == 0, T=T)
             for j, (n, lr, b1, b2, wd, e, T) in enumerate(zip(counts, lrs, b1s, b2s, wds, epss, Ts))]
    run = Run(L, cases)
    for k in range(3):
        run.launch()
        run.check(f"step {k + 1}")
    assert run.clocks[3] == amr.clock_seed(5, 0.3, 0.5)  # the empty segment's clock did not move (checked on the device above)
    lib = L[0]
    nine = (lib.KgeAdamSeg * 9)(*([run.seg(j) for j in range(8)] + [run.seg(0)]))
    assert lib.lib().kge_adam_step_multi(nine, None, 9, L[1]) == -1
    run.check("after the refused call")  # ... which launched nothing


def test_nothing_to_do_launches_nothing(L):
    rng = np.random.default_rng(52)
    run = Run(L, [_case(rng, 0, T=4), _case(rng, 0)])
    run.launch()
    run.check("all empty")


def test_clock_over_300_calls_and_from_a_restored_step_count(L):
    """Records of three hyper-parameter sets from T = 0 and one seeded at T = 1000, read back after EVERY call: t, both
    float64 powers and both floats are the restatement's bits -- the device's float64 division and square root must be
    correctly rounded for that.  The parameters after 300 steps are compared too."""
    rng = np.random.default_rng(53)
    hyper = [(1e-3, 0.9, 0.999, 0), (0.05, 0.9, 0.99, 0), (0.2, 0.5, 0.9999, 0), (1e-3, 0.9, 0.999, 1000)]
    run = Run(L, [_case(rng, 5, lr=lr, beta1=b1, beta2=b2, T=T, copy=False) for lr, b1, b2, T in hyper])
    for k in range(300):
        run.launch()
        run.check_clocks(f"call {k + 1}")
    assert [c[0] for c in run.clocks] == [300, 300, 300, 1300]
    run.check("after 300 calls")


@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_same_bits_as_kge_adam_step_given_the_clocks_two_floats(L, wd):
    lib, st = L
    rng = np.random.default_rng(54)
    cases = [_case(rng, n, wd=wd, copy=j % 2 == 0, T=T, lr=0.05, beta1=0.9, beta2=0.99)
             for j, (n, T) in enumerate([(1, 0), (1027, 0), (2500, 9), (4, 2), (1024, 0)])]
    run = Run(L, cases)
    run.launch()
    torch.cuda.synchronize()
    old = Run(L, cases)
    words = run.K.cpu().numpy()
    for i, c in enumerate(cases):
        _t, _b1, _b2, step_size, bc2 = struct.unpack("<qddff", words[1 + REC * i:][:4].tobytes())
        ar = old.ar
        lib.check(lib.lib().kge_adam_step(ar.ptr(old.P, i), ar.ptr(old.G, i), ar.ptr(old.A, i), ar.ptr(old.B, i), c.n,
                                          step_size, bc2, c.beta1, c.beta2, c.wd, c.eps,
                                          ar.ptr(old.C, i) if c.copy else None, st), "kge_adam_step")
    torch.cuda.synchronize()
    for a, b in ((run.P, old.P), (run.A, old.A), (run.B, old.B), (run.C, old.C)):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                           b.view(torch.int32) if b.dtype == torch.float32 else b)
    run.check("multi")


def test_penalties_every_segment_its_own_weight_and_value_slot(L):
    """lp with p = 1, 2, 3 on counts that end in a scalar tail, n3 over a [150, 16] table (1200 real parts: more than a
    workgroup's 1024), a segment without a penalty and an empty one in the same launch; exact zeros and -0 among the
    parameters, whole zero complex pairs too."""
    rng = np.random.default_rng(55)
    spec = [  # (count, kind, p, weight, row_dim, lr, wd, eps)
        (1027, 0, 0, 0.0, 0, 0.05, 0.0, 1e-8),
        (1027, 1, 1, 0.013, 0, 0.3, 1e-3, 1e-6),
        (0, 1, 2, 0.5, 0, 0.1, 0.0, 1e-8),
        (2051, 1, 2, 0.4, 0, 0.011, 0.0, 1e-3),
        (150 * 16, 2, 3, 0.07, 16, 0.2, 5e-4, 1e-8),
        (7, 1, 3, 1.5, 0, 0.6, 0.02, 0.0),
        (1025, 1, 3, 0.21, 0, 0.123, 0.0, 2e-4),
        (3, 1, 2, 0.9, 0, 0.02, 0.0, 1e-8),
    ]
    cases = []
    for j, (n, kind, pp, w, rd, lr, wd, e) in enumerate(spec):
        c = _case(rng, n, lr=lr, wd=wd, eps=e, copy=j % 2 == 1, kind=kind, pp=pp, weight=w, row_dim=rd)
        if kind == 2:
            rows = c.p.reshape(-1, rd)
            rows[1, :] = 0.0
            rows[2, :rd // 2] = -0.0
            rows[2, rd // 2:] = 0.0
        cases.append(c)
    run = Run(L, cases, pens=True)
    run.launch()
    run.check("penalty step 1")
    run.launch()
    run.check("penalty step 2")


# ---- through the class: capture ------------------------------------------------------------------------------------
def _steps(mode, n, resume_at=None):
    """loss = (w * x).sum() on a [64, 48] parameter with a static x: no scatter atomics, the same gradient every step.
    mode: "host" (eager, host-side bias correction), "device" (eager device_step), "graph" (device_step, GraphedStep)."""
    from kge_amd import optim as kopt
    from kge_amd.train_graph import GraphedStep
    g = torch.Generator().manual_seed(5)
    w = torch.nn.Parameter(torch.randn(64, 48, generator=g).to(DEV))
    x = torch.randn(64, 48, generator=g).to(DEV)
    make = lambda: kopt.Adam([w], lr=1e-3, device_step=mode != "host")
    opt = make()
    step = GraphedStep(lambda xx: (w * xx).sum(), opt, warmup=2, enabled=mode == "graph")
    for k in range(n):
        if k == resume_at:
            sd = opt.state_dict()
            assert sorted(sd["state"][0]) == ["exp_avg", "exp_avg_sq", "step"]
            opt = make()
            opt.load_state_dict(sd)
            step = GraphedStep(lambda xx: (w * xx).sum(), opt, enabled=False)
        step(x)
    torch.cuda.synchronize()
    return w.detach().clone(), opt, step, w


def test_captured_device_step_takes_the_eager_and_the_host_steps():
    w_h, _, _, _ = _steps("host", 12)
    w_d, opt_d, _, p_d = _steps("device", 12)
    w_g, opt_g, step, p_g = _steps("graph", 12)
    assert step.disabled_reason is None and step.replays == 10 and step.captures == 1
    assert torch.equal(w_g.view(torch.int32), w_d.view(torch.int32))
    # (a bias correction frozen at the capture step would be off by a factor above 2 at step 12)
    assert torch.equal(w_g.view(torch.int32), w_h.view(torch.int32))
    for opt, p in ((opt_d, p_d), (opt_g, p_g)):
        assert float(opt.state[p]["step"]) == 12 == opt.device_step_count(p)
    # a checkpoint at step 12, loaded into a fresh optimizer, and 3 more steps = 15 uninterrupted steps
    w_15, opt_15, _, p_15 = _steps("device", 15)
    w_r, opt_r, _, p_r = _steps("device", 15, resume_at=12)
    assert torch.equal(w_r.view(torch.int32), w_15.view(torch.int32))
    assert float(opt_r.state[p_r]["step"]) == 15 == opt_r.device_step_count(p_r) == opt_15.device_step_count(p_15)
