"""GPU: every entry point of tests/abi_cases.py with the state on a side stream, the configuration the production hosts
run (run_lines.py and arap_deform call use_own_stream()): the calls are "asynchronous on the state's stream"
(include/arap_opt.h), so every memset, copy and kernel of a call must be ordered behind what that stream holds, and a
call must not disturb the one before it that is still in flight.

Late inputs.  The input buffers hold a decoy, a second valid input set whose twin differs (asserted on the CPU by
tests/test_abi_host.py and again here).  On the side stream: a delay of ordinary torch work, at least ten times the call's
own duration and at least 5 ms, measured with events and asserted; then the scratch and the outputs are filled with 0xA5
again; then device-to-device copies bring the real inputs in; then the call, with no synchronisation before it returns.
A part of the call on another stream reads the decoy, or clears scratch that is dirtied again behind it, or writes an
output that is filled again behind it: the outputs then differ from the real case's twin.  Both input sets are valid, so a
mis-ordered read gives wrong bytes, never a wild index.

Whether the call came back to the host while the delay was still running is recorded per row, not asserted: the runtime
may make a call that holds a pageable hipMemcpyAsync wait for the stream (csrc/host_resident.h notes it), and
ArapFlow_WarpStep is documented to return when its outputs are written.  test_report prints the table.

Two calls in flight.  The case and the decoy, each into outputs of its own, through ONE scratch buffer, back to back on
the side stream, one synchronisation at the end; for the calls that rewrite a table the state owns (ArapFlow_WarpDiag's job
and accumulators, the texture, light and augmentation tables) a third call whose table differs."""
import math

import numpy as np
import pytest
import torch

import abi_cases
from abi_pool import FILL, Pool
from arap_flow_amd import opt
from test_gpu_abi_buffers import same

pytestmark = pytest.mark.gpu
NAMES = [r.name for r in abi_cases.ROWS]
FACTOR, FLOOR_MS = 10.0, 5.0
RETURNED_EARLY = {}                      # row -> the call returned while the delay was running


@pytest.fixture()
def side_state():
    st = opt.State()
    side = torch.cuda.Stream()
    try:
        st.set_stream(side)
        yield st, side
    finally:
        torch.cuda.synchronize()
        st.close()


class Delay:
    """ordinary torch work on a stream that ends by itself: matrix products of fixed operands"""

    def __init__(self, side):
        self.side = side
        with torch.cuda.stream(side):
            self.a = torch.full((2048, 2048), 1.0 / 2048, device="cuda")
            self.b = torch.ones(2048, 2048, device="cuda")
            self.c = torch.empty(2048, 2048, device="cuda")
            self.run(3)                                       # the first product loads its kernel
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(side)
            self.run(8)
            e1.record(side)
        e1.synchronize()
        self.unit_ms = e0.elapsed_time(e1) / 8

    def run(self, n):
        for _ in range(n):
            torch.mm(self.a, self.b, out=self.c)

    def enqueue(self, ms):
        """at least `ms` of work (twice that by the calibration), between two events"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(self.side):
            e0.record(self.side)
            self.run(int(math.ceil(2.0 * ms / self.unit_ms)) + 1)
            e1.record(self.side)
        return e0, e1


@pytest.mark.parametrize("name", NAMES)
def test_late_inputs(side_state, name):
    st, side = side_state
    r = abi_cases.BY_NAME[name]
    case, decoy = r.build(r.first), r.decoy()
    assert set(abi_cases.differ(case.twin, decoy.twin)) == set(case.call.outputs())        # (no GPU touched yet)
    pool = Pool()
    case.call.carve(pool)
    pool.allocate()
    staged = {}
    for real, fake in zip(case.call.bufs("input"), decoy.call.bufs("input")):
        assert (real.name, real.nbytes) == (fake.name, fake.nbytes)
        pool.upload(real.name, fake.data)                     # the buffers start out holding the decoy ...
        pool.expect(real.name, real.data)                     # ... and must hold the case in the end
        staged[real.name] = torch.from_numpy(Pool.raw(real.data).copy()).cuda()
    delay = Delay(side)
    torch.cuda.synchronize()
    # how long the call takes on an idle stream: sizes the delay, is never an expected value
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record(side)
    assert case.call.invoke(st.lib, st.handle, pool) == 0
    t1.record(side)
    t1.synchronize()
    need = max(FACTOR * t0.elapsed_time(t1), FLOOR_MS)
    torch.cuda.synchronize()

    d0, d1 = delay.enqueue(need)
    arrived = torch.cuda.Event()
    with torch.cuda.stream(side):
        for b in case.call.bufs("output"):
            pool.view(b.name).fill_(FILL)
        if case.call.scratch is not None:
            pool.view("scratch").fill_(FILL)
        for k, t in staged.items():
            pool.view(k).copy_(t, non_blocking=True)
        arrived.record(side)
    rc = case.call.invoke(st.lib, st.handle, pool)
    early = not arrived.query()                               # read at once: is the stream still behind the copies?
    side.synchronize()
    assert rc == 0
    took = d0.elapsed_time(d1)
    assert took >= need, "the delay ran %.3f ms, the call needs %.3f ms of it: nothing was shown" % (took, need)
    RETURNED_EARLY[name] = early
    snap = pool.snapshot()
    same(case.call, pool, snap, case.twin)
    pool.check(snap)


@pytest.mark.parametrize("name", NAMES)
def test_two_calls_in_flight(side_state, name):
    st, side = side_state
    r = abi_cases.BY_NAME[name]
    calls = [("a.", r.build(r.first)), ("b.", r.decoy())] + ([("c.", r.third())] if r.third is not None else [])
    pool = Pool()
    for tag, b in calls:
        b.call.carve(pool, tag=tag)                           # its own inputs and outputs, the one scratch
    pool.allocate()
    for tag, b in calls:
        b.call.upload(pool, tag=tag)
    torch.cuda.synchronize()
    rcs = [b.call.invoke(st.lib, st.handle, pool, tag=tag) for tag, b in calls]      # back to back, nothing waited for
    side.synchronize()
    assert rcs == [0] * len(calls)
    snap = pool.snapshot()
    for tag, b in calls:
        same(b.call, pool, snap, b.twin, tag=tag)
    pool.check(snap)


def test_report():
    """row -> shown / not shown: did the call return to the host while its stream was still busy?  Not asserted."""
    for name in NAMES:
        if name in RETURNED_EARLY:
            print("ASYNC %-16s %s" % (name, "shown" if RETURNED_EARLY[name] else "not shown"))
