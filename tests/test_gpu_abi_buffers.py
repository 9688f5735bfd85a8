"""GPU: every entry point of tests/abi_cases.py called the way a C caller does -- on the null stream, every buffer carved
out of ONE guarded pool (tests/abi_pool.py) at the alignment the header allows and no more, the scratch exactly the bytes
its size function answers and full of 0xA5, the outputs full of 0xA5 too.  Per case:
  * every output asked, and then the smallest legal set of outputs with every other one NULL: return code 0, the outputs
    byte for byte the twin's, every guard byte untouched, every input as uploaded;
  * the same call again on the same pool, nothing refilled: the scratch holds the first call's leftovers, the outputs its
    results -- identical bytes;
and per row a refused call: -1, and every output, the scratch and every guard still 0xA5."""
import numpy as np
import pytest
import torch

import abi_cases
from abi_pool import Pool

pytestmark = pytest.mark.gpu


def one_nan(raw):
    """float32 bytes with every NaN the same NaN"""
    bits = raw.view(np.uint32)
    return np.where(np.isnan(raw.view(np.float32)), np.uint32(0x7fc00000), bits).view(np.uint8)


def same(call, pool, snap, twin, tag="", only=None):
    """the outputs of a call (those `only` names) against the twin's, byte for byte"""
    want = abi_cases.flat(twin)
    for b in call.bufs("output"):
        if only is not None and b.name not in only:
            continue
        got, ref = pool.read(tag + b.name, snap), np.ascontiguousarray(want[b.name])
        assert got.size == ref.nbytes, b.name
        ref = np.frombuffer(ref.tobytes(), np.uint8)
        if b.name in abi_cases.BY_NAME[call.name].nan_any:
            got, ref = one_nan(got), one_nan(ref)
        diff = np.flatnonzero(got != ref)
        assert not diff.size, "%s %s: %d bytes differ from the twin's, the first at byte %d" % (call.name, b.name, diff.size, diff[0])


def run(st, b, only=None, repeat=True):
    """one pool, one call (and one more on the same pool): rc, twin, guards"""
    pool = Pool()
    b.call.carve(pool, only=only)
    pool.allocate()
    b.call.upload(pool)
    torch.cuda.synchronize()
    outs = [x.name for x in b.call.bufs("output") if only is None or x.name in only]
    first = None
    for again in range(2 if repeat else 1):
        assert b.call.invoke(st.lib, st.handle, pool) == 0
        torch.cuda.synchronize()
        snap = pool.snapshot()
        same(b.call, pool, snap, b.twin, only=only)
        pool.check(snap)
        got = [pool.read(n, snap).tobytes() for n in outs]
        if again:                                    # the scratch's leftovers and the outputs' old contents change nothing
            assert got == first
        first = got


@pytest.mark.parametrize("name,shape,aligns", abi_cases.CASES, ids=["%s-%s-%s" % c for c in abi_cases.CASES])
def test_guards_twin_and_repeat(gpu_state, name, shape, aligns):
    b = abi_cases.built(name, shape, aligns)
    run(gpu_state, b)
    minimal = abi_cases.BY_NAME[name].minimal
    if minimal is not None:
        run(gpu_state, b, only=set(minimal))


@pytest.mark.parametrize("name", [r.name for r in abi_cases.ROWS])
def test_a_refused_call_touches_nothing(gpu_state, name):
    r = abi_cases.BY_NAME[name]
    b = r.build(r.first)
    pool = Pool()
    b.call.carve(pool)
    pool.allocate()
    b.call.upload(pool)
    torch.cuda.synchronize()
    how, what = r.refuse
    kw = dict(null=what) if how == "null" else dict(values=what)
    assert b.call.invoke(gpu_state.lib, gpu_state.handle, pool, **kw) == -1
    torch.cuda.synchronize()
    pool.check(pristine=True)
    assert b.call.invoke(gpu_state.lib, gpu_state.handle, pool) == 0    # (the same arguments, unspoilt, are accepted)
    torch.cuda.synchronize()
    snap = pool.snapshot()
    same(b.call, pool, snap, b.twin)
    pool.check(snap)
