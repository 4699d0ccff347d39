"""kge_sparse_adam_step_touched (kge_amd/csrc/touched.hip) on the MI355X through the ctypes binding: parameter, both
moments, the bf16 copy and the 32-byte clock record must carry the BITS of the float32 restatement
(tests/_sparse_adam_ref.py), over three consecutive calls with fresh row sets, from a fresh record and from one restored
at T = 7.

Shapes: num_rows on both sides of a bitmap word and of the 256-row chunk of a workgroup (1, 31, 32, 33, 257, 1000); row
widths for both lane routes and a row longer than one trip of its lanes (1, 3, 4, 8, 130).  Layouts: contiguous; pitch
dim + 4 (keeps the four-float route where dim % 4 == 0); pitch dim + 3 and a base pointer one float off 16 bytes (both
force the one-float route).  Bitmaps: empty, full, a single bit, the last bit of a word, random, and bits set beyond
num_rows in the last word (ignored, cleared).  Rows whose bit is clear hold sentinel bit patterns in parameter, moments
(NaN payloads) and copy; they, the pitch padding and the guard rows of all five arrays must come back bit-identical.
The gradient (zero outside the marked rows on entry, as the contract says) and the bitmap are all zero on return."""
import struct

import numpy as np
import pytest
import torch

import _sparse_adam_ref as sar
import _touched_ref as tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROWS = [1, 31, 32, 33, 257, 1000]
DIMS = [1, 3, 4, 8, 130]
LAYOUTS = ["contiguous", "pitch4", "pitch3", "offset1"]
LR, BETAS, EPS = 0.01, (0.9, 0.999), 1e-8
SENT = {"p": 0xDEADBEEF, "m": 0x7FC12345, "v": 0xFFC0BEEF, "g": 0xDEADBEEF}
SENT_C = 0xBEEF


def _array(E, dim, layout, sentinel, dtype=np.uint32):
    """-> (whole allocation as a device tensor, the [E, dim] view handed to the library): one guard row in front and
    behind, pitch padding, all sentinel."""
    pitch = {"contiguous": dim, "pitch4": dim + 4, "pitch3": dim + 3, "offset1": dim + 4}[layout]
    off = 1 if layout == "offset1" else 0
    t = {np.uint32: torch.int32, np.uint16: torch.int16}[dtype]
    whole = torch.from_numpy(np.full((E + 2) * pitch + 8, sentinel, dtype=dtype).view(
        {np.uint32: np.int32, np.uint16: np.int16}[dtype]).copy()).to(DEV)
    assert t == whole.dtype
    typed = whole.view(torch.float32) if dtype is np.uint32 else whole  # (the same memory: `whole` is compared as bits)
    return whole, typed[off + pitch: off + pitch + E * pitch].view(E, pitch)[:, :dim]


def _bitmaps(E, rng):
    w = (E - 1) // 32
    out = {"empty": [], "full": list(range(E)), "single": [int(rng.integers(0, E))],
           "last_of_word": [r for r in (31, 32 * w + 31) if r < E] or [E - 1],
           "random": sorted(set(rng.integers(0, E, max(1, E // 3)).tolist()) | {0, E - 1})}
    return out


def _clock_tensor(T):
    rec = struct.pack("<qddff", T, BETAS[0] ** T, BETAS[1] ** T, 0.0, 0.0)
    return torch.frombuffer(bytearray(rec), dtype=torch.int64).to(DEV)


def _run(E, dim, layout, kind_order, T, seed, with_copy=True):
    """Three calls -> per call (param, m, v, copy, clock bytes) as numpy, from the device and from the restatement."""
    from kge_amd import engine
    rng = np.random.default_rng(seed)
    words = tr.bitmap_bytes(E) // 4
    # host state: sentinel everywhere, real values are written into the rows a call marks (their first time)
    hp = np.full((E, dim), SENT["p"], np.uint32).view(np.float32)
    hm = np.full((E, dim), SENT["m"], np.uint32).view(np.float32)
    hv = np.full((E, dim), SENT["v"], np.uint32).view(np.float32)
    hc = np.full((E, dim), SENT_C, np.uint16)
    live = np.zeros(E, bool)
    wp, P = _array(E, dim, layout, SENT["p"])
    wm, M = _array(E, dim, layout, SENT["m"])
    wv, V = _array(E, dim, layout, SENT["v"])
    wg, G = _array(E, dim, layout, SENT["g"])
    wc, C = _array(E, dim, layout, SENT_C, np.uint16)
    G.zero_()  # the contract: zero outside the marked rows (padding and guards keep their sentinel)
    guards = [w.clone() for w in (wp, wm, wv, wg, wc)]
    clock_dev = _clock_tensor(T)
    clock = sar.clock_seed(T, *BETAS)
    out = []
    for call, kind in enumerate(kind_order):
        rows = _bitmaps(E, rng)[kind]
        fresh = [r for r in rows if not live[r]]
        if fresh:  # rows entering the live set get real values on both sides
            hp[fresh] = rng.standard_normal((len(fresh), dim)).astype(np.float32)
            hm[fresh] = (rng.standard_normal((len(fresh), dim)) * 0.1).astype(np.float32)
            hv[fresh] = (rng.random((len(fresh), dim)) * 0.01).astype(np.float32)
            idx = torch.tensor(fresh, device=DEV)
            P[idx] = torch.from_numpy(hp[fresh]).to(DEV)
            M[idx] = torch.from_numpy(hm[fresh]).to(DEV)
            V[idx] = torch.from_numpy(hv[fresh]).to(DEV)
            C[idx] = torch.from_numpy(tr.bf16_rne_bits(hp[fresh]).view(np.int16)).to(DEV)
            hc[fresh] = tr.bf16_rne_bits(hp[fresh])
            live[fresh] = True
        hg = np.zeros((E, dim), np.float32)
        if rows:
            hg[rows] = rng.standard_normal((len(rows), dim)).astype(np.float32)
            hg[rows[0]] = 0.0  # a marked row whose gradient is exactly zero: it still moves
            G[torch.tensor(rows, device=DEV)] = torch.from_numpy(hg[rows]).to(DEV)
        bm = tr.mark(rows, E)
        dev_bm = bm.copy()
        if E % 32:  # bits beyond num_rows in the last live word: ignored, and cleared
            dev_bm[(E - 1) // 32] |= np.uint32((0xFFFFFFFF << (E % 32)) & 0xFFFFFFFF)
        bitmap = torch.from_numpy(dev_bm.view(np.int32).copy()).to(DEV)
        assert bitmap.numel() == words
        engine.sparse_adam_step_touched(P, G, M, V, bitmap, clock_dev, LR, BETAS[0], BETAS[1], EPS,
                                        C if with_copy else None)
        torch.cuda.synchronize()
        hp, _, hm, hv, _, hc2, clock = sar.step_touched(hp, hg, hm, hv, bm, clock, LR, BETAS[0], BETAS[1], EPS,
                                                        hc if with_copy else None)
        if with_copy:
            hc = hc2
        assert not G.any(), (kind, "grad not zero on return")
        assert not bitmap.any(), (kind, "bitmap not zero on return")
        got = (P.cpu().numpy().view(np.uint32).copy(), M.cpu().numpy().view(np.uint32).copy(),
               V.cpu().numpy().view(np.uint32).copy(), C.cpu().numpy().view(np.uint16).copy(),
               bytes(clock_dev.cpu().numpy().tobytes()))
        want = (hp.view(np.uint32).copy(), hm.view(np.uint32).copy(), hv.view(np.uint32).copy(), hc.copy(),
                sar.clock_bytes(clock))  # (copies: the next call writes its fresh rows into hp, hm, hv, hc in place)
        out.append((kind, got, want))
    # padding, guard rows and the slack around them: byte-equal to before (the [E, dim] views excluded)
    for w, g, view in zip((wp, wm, wv, wg, wc), guards, (P, M, V, G, C)):
        view.copy_(torch.zeros_like(view))
        g2 = g.clone()
        pitch = view.stride(0) if E > 1 else (dim if layout == "contiguous" else dim + (3 if layout == "pitch3" else 4))
        off = 1 if layout == "offset1" else 0
        g2[off + pitch: off + pitch + E * pitch].view(E, pitch)[:, :dim] = 0  # (int 0 = the bits of 0.0f)
        assert torch.equal(w, g2), "a write outside the [E, dim] view"
    return out


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("E", ROWS)
def test_three_calls_carry_the_restatements_bits(E, dim):
    orders = [("random", "full", "single"), ("empty", "last_of_word", "random")]
    for li, layout in enumerate(LAYOUTS):
        for oi, order in enumerate(orders):
            T = 7 if (li + oi) % 2 else 0  # a fresh record, or one restored at T = 7
            for kind, got, want in _run(E, dim, layout, order, T, seed=E * 1000 + dim * 10 + li):
                for name, a, b in zip(("param", "exp_avg", "exp_avg_sq", "copy"), got, want):
                    bad = np.argwhere(a != b)
                    assert bad.size == 0, (layout, order, kind, T, name, bad[:4].tolist(),
                                           [hex(int(x)) for x in a[a != b][:4]], [hex(int(x)) for x in b[a != b][:4]])
                assert got[4] == want[4], (layout, order, kind, T, "clock", struct.unpack("<qddff", got[4]),
                                           struct.unpack("<qddff", want[4]))


def test_two_runs_give_identical_bits_and_the_copy_is_optional():
    a = _run(257, 8, "pitch4", ("random", "full", "random"), 0, seed=11)
    b = _run(257, 8, "pitch4", ("random", "full", "random"), 0, seed=11)
    for (_, ga, _), (_, gb, _) in zip(a, b):
        assert all(np.array_equal(x, y) for x, y in zip(ga[:4], gb[:4])) and ga[4] == gb[4]
    for kind, got, want in _run(33, 4, "contiguous", ("full", "single", "empty"), 7, seed=12, with_copy=False):
        assert all(np.array_equal(x, y) for x, y in zip(got[:4], want[:4])) and got[4] == want[4]  # (copy: untouched)


def test_the_clock_ticks_for_an_empty_table_and_not_for_a_declined_call():
    from kge_amd import _lib, engine
    clock_dev = _clock_tensor(3)
    with torch.cuda.device(DEV):
        st = engine._stream(DEV)
        rc = _lib.lib().kge_sparse_adam_step_touched(None, 4, None, 4, None, 4, None, 4, None, 0, 4, clock_dev.data_ptr(),
                                                     LR, BETAS[0], BETAS[1], EPS, None, 0, st)
        assert rc == 0
        torch.cuda.synchronize()
        want = sar.clock_tick(sar.clock_seed(3, *BETAS), LR, *BETAS)
        assert bytes(clock_dev.cpu().numpy().tobytes()) == sar.clock_bytes(want)
        rc = _lib.lib().kge_sparse_adam_step_touched(16, 4, 16, 4, 16, 4, 16, 4, 16, 256 << 31, 4, clock_dev.data_ptr(),
                                                     LR, BETAS[0], BETAS[1], EPS, None, 0, st)
        assert rc == -2
        rc = _lib.lib().kge_sparse_adam_step_touched(16, 4, 16, 4, 16, 4, 16, 4, 16, 8, 4, clock_dev.data_ptr(),
                                                     LR, 1.0, BETAS[1], EPS, None, 0, st)
        assert rc == -1
        torch.cuda.synchronize()
        assert bytes(clock_dev.cpu().numpy().tobytes()) == sar.clock_bytes(want)
