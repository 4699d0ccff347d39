"""The next group's query build in the tail of pairs_bf16_v8_kernel (d = 512), in CLAIMED slices.

Who writes which fragment changes -- a workgroup that is done with its scores takes slices of 512 items by ticket from a
counter pair the library keeps per stream -- not one byte of a fragment or a score.  Bars:
  * the raw fragment buffer a launch builds = build_queries_group's for the same triples (torch.equal), the scores of
    the launch = the fixed-slice arm's (switch V8_TAIL_FIXED = 1) bit for bit: ComplEx and DistMult, split and single-pass
    queries, two-sided, E in {33, 300}, n in {1, 17, 130}, L in {1, 3} (8 .. 96 slices for the 256 workgroups), and n = 530
    x L = 5 (360 slices with split queries, 400 without: more than workgroups);
  * the counters clean themselves: six launches back to back on one stream, every built buffer exact, the pair {0, 0};
  * two streams, a launch in flight on each: both buffers exact, two different pairs;
  * a captured launch, replayed three times, builds through the fixed slices (no claimed launch counted, exact fragments);
  * a launch without a next group leaves the pair alone (a planted sentinel survives) and scores like the fixed arm.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D, R = 512, 7
BIG = (530, 5)  # 5 x 18 (split) row groups x 2,048 items = 360 slices of 512 for 256 workgroups


@pytest.fixture(scope="module")
def eng():
    from kge_amd import engine
    return engine


_TABLES = {}


def _tables(eng, scorer, E, split):
    """One pair of tables per (scorer, E, split), shared by every test that needs it and never written."""
    key = (scorer, E, split)
    if key not in _TABLES:
        g = torch.Generator().manual_seed(2000 + E + (7 if scorer == "distmult" else 0))
        ent = (torch.randn(E, D, generator=g) * 0.3).bfloat16().to(DEV)
        rel = (torch.randn(R, D, generator=g) * 0.3).bfloat16().to(DEV)
        _TABLES[key] = eng.Tables(scorer, ent, rel, flags=eng.FLAG_SPLIT_QUERY if split else 0)
    return _TABLES[key]


def _triples(E, rows, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(hi, (rows,), generator=g) for hi in (E, R, E)], dim=1).to(DEV).contiguous()


def _flags(eng, split):
    return eng.FLAG_SPLIT_QUERY if split else None


def _group(eng, T, n, L, split):
    q = eng.QueriesGroup(T, "sp_po", n, L, flags=_flags(eng, split))
    q.buf.zero_()  # (the padding between two batches' fragments is nobody's)
    return q


def _reference(eng, T, trip, n, L, split):
    return eng.build_queries_group(T, "sp_po", trip, n, L, out=_group(eng, T, n, L, split))


def _claimed_launches():
    from kge_amd import _lib
    return _lib.lib().kge_debug_launch_count(2)


def _pair(stream=None, plant=None):
    """{next ticket, workgroups done} of the stream's counter pair (None: the stream has none); plant = (a, b): written
    behind the read."""
    from kge_amd import _lib
    fn = _lib.lib().kge_debug_v8_claim_counters
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    st = (stream or torch.cuda.current_stream(torch.device(DEV))).cuda_stream
    got = (ctypes.c_uint32 * 2)()
    put = (ctypes.c_uint32 * 2)(*plant) if plant is not None else None
    rc = fn(ctypes.c_void_p(st), put, got)
    assert rc in (0, 1), rc
    return (int(got[0]), int(got[1])) if rc == 1 else None


def _launch(eng, T, q, E, nxt=None, nq=None):
    out = torch.empty(q.num_batches, q.n, 2 * E, device=DEV)
    eng.score_queries_group(T, q, out, next_batch=nxt, next_queries=nq)
    return out


def _check_shape(eng, kge_switch, scorer, split, E, n, L, seed):
    T = _tables(eng, scorer, E, split)
    g0, g1 = _triples(E, n * L, seed), _triples(E, n * L, seed + 1)
    cur, want = _reference(eng, T, g0, n, L, split), _reference(eng, T, g1, n, L, split)
    what = f"{scorer} split={split} E={E} n={n} L={L}"
    kge_switch.set("V8", 1)  # (a group of one takes the persistent kernel too)
    kge_switch.set("V8_TAIL_FIXED", 1)
    c0 = _claimed_launches()
    fixed_q = _group(eng, T, n, L, split)
    fixed = _launch(eng, T, cur, E, g1, fixed_q)
    assert _claimed_launches() == c0, f"{what}: V8_TAIL_FIXED = 1 took the claimed slices"
    kge_switch.unset("V8_TAIL_FIXED")
    claimed_q = _group(eng, T, n, L, split)
    claimed = _launch(eng, T, cur, E, g1, claimed_q)
    assert _claimed_launches() == c0 + 1, f"{what}: the launch did not take the claimed slices"
    torch.cuda.synchronize()
    assert torch.equal(fixed_q.buf, want.buf), f"{what}: fixed slices differ from build_queries_group"
    assert torch.equal(claimed_q.buf, want.buf), f"{what}: claimed slices differ from build_queries_group"
    assert torch.equal(claimed.view(torch.int32), fixed.view(torch.int32)), f"{what}: scores differ from the fixed arm's"
    assert _pair() == (0, 0), f"{what}: the counters were not set back"


@pytest.mark.parametrize("split", [True, False], ids=["split", "single"])
@pytest.mark.parametrize("scorer", ["complex", "distmult"])
def test_fragments_and_scores_against_the_fixed_slices(eng, scorer, split, kge_switch):
    """8 .. 72 slices (split) / 16 .. 96 (single-pass) for 256 workgroups: most workgroups' first claim fails."""
    for E in (33, 300):
        for n in (1, 17, 130):
            for L in (1, 3):
                _check_shape(eng, kge_switch, scorer, split, E, n, L, seed=17 * E + 3 * n + L)


@pytest.mark.parametrize("split", [True, False], ids=["split-360-slices", "single-400-slices"])
def test_more_slices_than_workgroups(eng, split, kge_switch):
    n, L = BIG
    _check_shape(eng, kge_switch, "complex", split, 300, n, L, seed=71)


@pytest.mark.parametrize("shape", [(130, 3), BIG], ids=["72-slices", "360-slices"])
def test_six_launches_back_to_back_clean_the_counters(eng, shape, kge_switch):
    """The bench's rotation: launch k scores buffer k % 2 and builds group k + 1 into the other one.  No host-side reset
    between the launches: launch k + 1 starts from the 0 launch k left."""
    n, L = shape
    E = 300
    T = _tables(eng, "complex", E, True)
    kge_switch.set("V8", 1)
    groups = [_triples(E, n * L, 300 + k) for k in range(7)]
    want = [_reference(eng, T, g, n, L, True) for g in groups]
    qs = [_group(eng, T, n, L, True) for _ in range(2)]
    eng.build_queries_group(T, "sp_po", groups[0], n, L, out=qs[0])
    c0 = _claimed_launches()
    built = []
    for k in range(6):
        _launch(eng, T, qs[k % 2], E, groups[k + 1], qs[1 - k % 2])
        built.append(qs[1 - k % 2].buf.clone())  # (stream-ordered: before launch k + 2 builds into it again)
    torch.cuda.synchronize()
    assert _claimed_launches() == c0 + 6
    for k in range(6):
        assert torch.equal(built[k], want[k + 1].buf), f"launch {k} of six: built fragments differ"
    assert _pair() == (0, 0)


def test_two_streams_never_share_a_pair(eng, kge_switch):
    """A group launch in flight on each of two streams: each stream claims from its own pair."""
    n, L = BIG
    E = 300
    T = _tables(eng, "complex", E, True)
    kge_switch.set("V8", 1)
    g0 = _triples(E, n * L, 400)
    nxt = [_triples(E, n * L, 401 + i) for i in range(2)]
    cur = _reference(eng, T, g0, n, L, True)
    want = [_reference(eng, T, t, n, L, True) for t in nxt]
    got = [_group(eng, T, n, L, True) for _ in range(2)]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device=DEV) for _ in range(2)]
    outs = []
    for rep in range(3):  # (three rounds: the pairs are also left clean with a neighbour running)
        for i, st in enumerate(streams):
            with torch.cuda.stream(st):
                outs.append(_launch(eng, T, cur, E, nxt[i], got[i]))
    torch.cuda.synchronize()
    for i in range(2):
        assert torch.equal(got[i].buf, want[i].buf), f"stream {i}: built fragments differ"
        assert _pair(streams[i]) == (0, 0), f"stream {i}: counters not set back"
        assert torch.equal(outs[i].view(torch.int32), outs[0].view(torch.int32))
    # two pairs: a sentinel planted in one is not seen through the other
    try:
        _pair(streams[0], plant=(5, 0))
        assert _pair(streams[1]) == (0, 0), "the two streams share a counter pair"
        assert _pair(streams[0]) == (5, 0)
    finally:
        _pair(streams[0], plant=(0, 0))


def test_captured_launch_builds_through_the_fixed_slices(eng, kge_switch):
    """A captured launch may be replayed on any stream, next to another replay: it must not use a stream's pair."""
    n, L = 130, 3
    E = 300
    T = _tables(eng, "complex", E, True)
    kge_switch.set("V8", 1)
    g0, g1 = _triples(E, n * L, 500), _triples(E, n * L, 501)
    cur, want = _reference(eng, T, g0, n, L, True), _reference(eng, T, g1, n, L, True)
    got = _group(eng, T, n, L, True)
    out = torch.empty(L, n, 2 * E, device=DEV)
    eager = _launch(eng, T, cur, E)
    torch.cuda.synchronize()
    c0 = _claimed_launches()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        eng.score_queries_group(T, cur, out, next_batch=g1, next_queries=got)
    assert _claimed_launches() == c0, "the captured launch took a stream's counter pair"
    for rep in range(3):
        got.buf.zero_()
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(got.buf, want.buf), f"replay {rep}: built fragments differ"
        assert torch.equal(out.view(torch.int32), eager.view(torch.int32)), f"replay {rep}: scores differ"
    assert _claimed_launches() == c0


def test_launch_without_a_next_group_leaves_the_counters_alone(eng, kge_switch):
    n, L = 130, 3
    E = 300
    T = _tables(eng, "complex", E, True)
    kge_switch.set("V8", 1)
    g0, g1 = _triples(E, n * L, 600), _triples(E, n * L, 601)
    cur = _reference(eng, T, g0, n, L, True)
    with_build = _launch(eng, T, cur, E, g1, _group(eng, T, n, L, True))  # (the stream has a pair from here on)
    kge_switch.set("V8_TAIL_FIXED", 1)
    fixed = _launch(eng, T, cur, E)
    kge_switch.unset("V8_TAIL_FIXED")
    assert _pair() == (0, 0)
    c0 = _claimed_launches()
    try:
        _pair(plant=(12345, 7))
        plain = _launch(eng, T, cur, E)
        assert _pair() == (12345, 7), "a launch without a next group touched the counters"
    finally:
        _pair(plant=(0, 0))
    assert _claimed_launches() == c0
    assert torch.equal(plain.view(torch.int32), fixed.view(torch.int32))
    assert torch.equal(plain.view(torch.int32), with_build.view(torch.int32))
