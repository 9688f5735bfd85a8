"""No GPU: the guard pool's own arithmetic over a numpy-backed pool (tests/abi_pool.py), every ArapFlow_*ScratchBytes
function through ctypes against what include/arap_opt.h states of it, and the table of tests/abi_cases.py: every row
describes its call, its twin covers every output, and its case and decoy give different outputs."""
import itertools

import numpy as np
import pytest

import abi_cases
from abi_pool import BASE, FILL, GUARD, Layout, Pool, place
from arap_flow_amd import capi


# ---- the pool -------------------------------------------------------------------------------------------------------------
ALIGNS = (1, 2, 4, 8, 16, 64, 256, 512)


def test_place_keeps_the_guard_and_the_alignment_and_no_more():
    for align in ALIGNS:
        for cursor in list(range(0, 70)) + [255, 256, 257, 4095, 4096, 4097, 12345]:
            o = place(cursor, align)
            assert o - cursor >= GUARD and o % align == 0
            assert o - cursor < GUARD + 2 * align                       # (no further than it has to be)
            if align < 256:
                assert o % (2 * align) == align, (cursor, align, o)     # an odd multiple: not aligned to twice as much


def test_layout_guards_before_between_and_after():
    rng = np.random.default_rng(0)
    for _ in range(50):
        L = Layout()
        sizes = [int(v) for v in rng.integers(1, 3000, rng.integers(1, 8))]
        for k, n in enumerate(sizes):
            L.add("b%d" % k, n, int(rng.choice(ALIGNS)), "output")
        spans = sorted((o, o + n) for o, n, _, _ in L.parts.values())
        assert spans[0][0] >= GUARD and L.total - spans[-1][1] == GUARD
        for (_, e), (s, _) in zip(spans, spans[1:]):
            assert s - e >= GUARD
        g = L.guard_mask()
        assert g.size == L.total and int((~g).sum()) == sum(sizes)       # exactly the bytes asked: no rounding inside a buffer
        for s, e in spans:
            assert not g[s:e].any() and g[s - GUARD:s].all() and g[e:e + GUARD].all()


def small_pool():
    p = Pool("numpy")
    p.carve("in", 100, 1, "input")
    p.carve("out", 37, 8, "output")
    p.carve("scratch", 512, 256, "scratch")
    p.allocate()
    data = np.arange(100, dtype=np.uint8)
    p.upload("in", data)
    return p, data


def test_pool_addresses_and_a_clean_check():
    p, data = small_pool()
    assert p.base % BASE == 0 and p.ptr("in") % 2 == 1 and p.ptr("out") % 16 == 8 and p.ptr("scratch") % 256 == 0
    assert p.ptr("never carved") is None                                 # a NULL output has no bytes of its own
    snap = p.snapshot()
    assert (p.read("in", snap) == data).all() and (p.read("out", snap) == FILL).all() and (p.read("scratch", snap) == FILL).all()
    p.check()
    p.check(pristine=True)
    p.view("out")[:] = 3                                                 # a call writes its output and its scratch ...
    p.view("scratch")[5] = 0
    p.check()
    with pytest.raises(AssertionError, match="output out"):             # ... which a refused call may not
        p.check(pristine=True)


def test_pool_check_finds_every_single_stray_byte():
    """one byte before and one past every buffer, the pool's first and last byte, a changed input byte"""
    p, _ = small_pool()
    total = p.layout.total
    spots = [0, total - 1]
    for o, n, _, _ in p.layout.parts.values():
        spots += [o - 1, o + n, o - GUARD, o + n + GUARD - 1]
    for at in spots:
        q, _ = small_pool()
        q.store[at] = 0
        with pytest.raises(AssertionError, match="guard bytes"):
            q.check()
    for at in (0, 50, 99):
        q, _ = small_pool()
        q.view("in")[at] ^= 1
        with pytest.raises(AssertionError, match="input in"):
            q.check()
    q = Pool("numpy")
    q.carve("in", 4, 4, "input")
    q.allocate()
    with pytest.raises(AssertionError, match="never uploaded"):
        q.check()
    with pytest.raises(AssertionError):
        q.upload("in", np.zeros(5, np.uint8))                            # not the bytes carved


def test_pool_a_guard_byte_that_holds_the_fill_value_again_is_the_only_blind_spot():
    """check() compares with 0xA5: a stray store of exactly that byte cannot show.  The outputs are compared with the twin
    and the inputs with the upload, so this concerns the guards alone, and a kernel's stray row is not all 0xA5."""
    p, _ = small_pool()
    p.store[0] = FILL
    p.check()


# ---- the scratch size functions -----------------------------------------------------------------------------------------------
def r256(n):
    return -(-int(n) // 256) * 256


T_MAX, S_MAX, G, K_MAX = capi.MAX_SNAPSHOTS + 1, capi.MAX_BLUR_SAMPLES, capi.BLUR_CHUNK, capi.INTERP_MAX_TIMES
FRAMES = sorted({(5, 1), (7, 5), (10, 8), (21, 3), (64, 4), (67, 9), (70, 9), (71, 9), (65, 4), (13, 6), (300, 5), (70, 50), (129, 65), (130, 70)})

# per function: the arguments after (W, H) as {name: values, smallest first}, which of them the header says do not matter,
# the least the buffer must hold -- the parts include/arap_opt.h names (per pixel, per point, per state), each rounded to
# the 256 bytes its parts are aligned to, plus 256 for the job the warp family, the tracks and the segment maps keep behind
# them -- and the argument values the header says the call refuses (the size is then 0)
SIZES = {
    "Warp": dict(args={}, least=lambda N: r256(8 * N) + 256),
    "WarpEx": dict(args={}, least=lambda N: r256(8 * N) + r256(4 * (N + 1)) + r256(4 * N) + r256(16 * N) + 256),
    "WarpLayers": dict(args=dict(n=(1, 2, 5, 255)), free=("n",),
                       least=lambda N, n: r256(8 * N) + r256(4 * (N + 1)) + r256(4 * N) + r256(16 * N) + r256(N) + 256),
    "WarpLayersStep": dict(args=dict(n=(1, 2, 5, 255)), free=("n",),
                           least=lambda N, n: max(48 * N, r256(8 * N) + r256(4 * (N + 1)) + r256(4 * N) + 2 * r256(16 * N) + 256)),
    "TrackPoints": dict(args=dict(T=(1, 2, T_MAX), P=(1, 40, 257, 403, 5000)),
                        least=lambda N, T, P: max(T * (4 * (N + 1) + 37 * P) + 32 * P,
                                                  T * (r256(4 * (N + 1)) + r256(4 * P) + r256(16 * P) + r256(P)) + r256(T * 16 * P) + r256(32 * P) + 256),
                        refused=dict(T=(0, T_MAX + 1), P=(0, (1 << 24) + 1))),
    "BlurLayers": dict(args=dict(n=(1, 3, 255), samples=(1, 2, 5, G, G + 1, S_MAX)), free=("n",),
                       least=lambda N, n, S: r256(8 * min(S, G) * N) + (r256(8 * N) if S > G else 0),
                       refused=dict(n=(0, 256), samples=(0, S_MAX + 1))),
    "SegMaps": dict(args=dict(n=(1, 3, 255)), free=("n",), least=lambda N, n: max(18 * N, 2 * r256(8 * N) + 2 * r256(N) + 256),
                    refused=dict(n=(0, 256))),
    "MapScore": dict(args={}, least=lambda N: max(7 * N, 3 * r256(N) + 2 * r256(2 * N)), refused={}),
    "Interp": dict(args=dict(K=(1, 3, K_MAX)), least=lambda N, K: r256(8 * K * N), refused=dict(K=(0, K_MAX + 1))),
}
SIZE_FN = {"Warp": "WarpScratchBytes", "WarpEx": "WarpExScratchBytes", "WarpLayers": "WarpLayersScratchBytes",
           "WarpLayersStep": "WarpLayersStepScratchBytes", "TrackPoints": "TrackPointsScratchBytes",
           "BlurLayers": "BlurLayersScratchBytes", "SegMaps": "SegMapsScratchBytes", "MapScore": "MapScoreScratchBytes",
           "Interp": "InterpScratchBytes"}


def size_fn(name):
    return getattr(capi.load(), "ArapFlow_" + SIZE_FN[name])


def test_every_size_function_of_the_header_is_listed():
    declared = {n[len("ArapFlow_"):] for n, _, _ in capi.SYMBOLS if n.endswith("ScratchBytes")}
    assert declared == set(SIZE_FN.values())
    used = {b.call.scratch.fn[len("ArapFlow_"):] for r in abi_cases.ROWS for b in [r.build(r.first)] if b.call.scratch}
    assert used == declared                                              # and every one of them sizes a row of the table


@pytest.mark.parametrize("name", list(SIZES))
def test_size_is_a_multiple_of_256_holds_what_the_header_states_and_grows(name):
    f, spec = size_fn(name), SIZES[name]
    names = list(spec["args"])
    grid = list(itertools.product(*spec["args"].values()))
    for W, H in FRAMES:
        for extra in grid:
            s = f(W, H, *extra)
            assert s > 0 and s % 256 == 0, (W, H, extra)
            assert s >= spec["least"](W * H, *extra), (W, H, extra, s, spec["least"](W * H, *extra))
            for k, v in enumerate(extra):                                # monotone in each of its own arguments ...
                vals = spec["args"][names[k]]
                nxt = vals[vals.index(v) + 1:vals.index(v) + 2]
                if nxt:
                    bigger = f(W, H, *extra[:k], nxt[0], *extra[k + 1:])
                    assert bigger >= s, (W, H, extra, names[k])
                    if names[k] in spec.get("free", ()):                 # ... and unchanged by those that do not matter
                        assert bigger == s, (W, H, extra, names[k])
            assert f(W + 1, H, *extra) >= s and f(W, H + 1, *extra) >= s  # ... and in the frame's


@pytest.mark.parametrize("name", list(SIZES))
def test_size_meets_the_bound_where_nothing_is_rounded(name):
    """at a frame and sizes where every part is a multiple of 256 by itself the bound is the size: 256 bytes fewer would
    not hold the parts the header names"""
    f, spec = size_fn(name), SIZES[name]
    big = tuple(v[-2] if len(v) > 1 else v[0] for v in spec["args"].values())
    if name == "TrackPoints":
        big = (2, 256)
    s, least = f(64, 4, *big), spec["least"](256, *big)
    assert s >= least and s - least <= 256, (s, least)                  # (the two jobs of this track call take 512 bytes)
    if name != "TrackPoints":
        assert s == least


@pytest.mark.parametrize("name", [n for n in SIZES if "refused" in SIZES[n]])
def test_size_is_zero_exactly_where_the_call_refuses(name):
    f, spec = size_fn(name), SIZES[name]
    names = list(spec["args"])
    ok = tuple(v[0] for v in spec["args"].values())
    assert f(7, 5, *ok) > 0 and f(1, 1, *ok) > 0
    for W, H in ((0, 5), (5, 0), (1 << 16, 1 << 15)):                    # a zero size, W * H = 2^31
        assert f(W, H, *ok) == 0
    assert f((1 << 16) - 1, 1 << 15, *tuple(v[0] for v in spec["args"].values())) > 0 or name == "Interp"       # just below
    for k, arg in enumerate(names):
        for bad in spec["refused"].get(arg, ()):
            assert f(7, 5, *ok[:k], bad, *ok[k + 1:]) == 0, (arg, bad)
        for good in spec["args"][arg]:                                   # every value of the grid, the limits included
            assert f(7, 5, *ok[:k], good, *ok[k + 1:]) > 0, (arg, good)
    if name == "Interp":                                                 # K * W * H < 2^31 too
        assert f(1 << 15, 1 << 11, 32) == 0 and f(1 << 15, 1 << 11, 31) > 0


def test_the_sizes_of_the_table_are_the_functions_answers():
    for r in abi_cases.ROWS:
        for shape in r.shapes:
            s = r.build(shape).call.scratch
            if s is not None:
                assert s.nbytes == getattr(capi.load(), s.fn)(*s.args) > 0, (r.name, shape)


# ---- the table --------------------------------------------------------------------------------------------------------------
def test_the_table_holds_every_entry_point_on_caller_owned_memory():
    takes_buffers = {"Warp", "WarpEx", "WarpStep", "WarpDiag", "WarpLayers", "WarpLayersStep", "TrackPoints", "Background",
                     "BackgroundSeq", "Texture", "BlurLayers", "Relight", "SegMaps", "FlowScore", "TrackScore", "ChainFlows",
                     "FrameScore", "LabelScore", "MapScore", "InterpFrames", "AugmentPairs"}
    assert [r.name for r in abi_cases.ROWS] and {r.name for r in abi_cases.ROWS} == takes_buffers
    assert all(hasattr(capi.load(), "ArapFlow_" + r.name) for r in abi_cases.ROWS)


@pytest.mark.parametrize("name", [r.name for r in abi_cases.ROWS])
def test_row_describes_its_call_and_case_and_decoy_differ(name):
    r = abi_cases.BY_NAME[name]
    case, decoy = r.build(r.first), r.decoy()
    outs = case.call.outputs()
    assert outs and set(abi_cases.flat(case.twin)) == set(outs)          # the twin covers every output, and nothing else
    for b in case.call.bufs("output"):
        assert np.ascontiguousarray(abi_cases.flat(case.twin)[b.name]).nbytes == b.nbytes, b.name
    same_layout = lambda a, b: [(x.name, x.kind, x.nbytes, x.align) for x in a.call.bufs()] == [(x.name, x.kind, x.nbytes, x.align) for x in b.call.bufs()]
    assert same_layout(case, decoy)
    assert set(abi_cases.differ(case.twin, decoy.twin)) == set(outs), "case and decoy agree on an output"
    for a, b in zip(case.call.bufs("input"), decoy.call.bufs("input")):  # a read of any input before its time reads other bytes
        assert not np.array_equal(Pool.raw(a.data), Pool.raw(b.data)), "case and decoy agree on input %s" % a.name
    if r.minimal is not None:
        assert set(r.minimal) < set(outs)
    if r.third is not None:
        third = r.third()
        assert set(third.call.outputs()) <= set(outs)
        for other in (case, decoy):
            assert abi_cases.differ(third.twin, other.twin) == third.call.outputs()
    for b in case.call.bufs():
        assert b.align in (1, 2, 4, 8), (b.name, b.align)                # an element type's alignment, never more
    if r.vec:
        assert {b.align for b in abi_cases.built(name, r.first, "vec").call.bufs()} == {16}
    for shape in r.shapes:                                               # every shape builds, and its twin fits
        b = r.build(shape)
        assert set(abi_cases.flat(b.twin)) == set(b.call.outputs()), shape
