"""Where in a block a lane of the record-light decoder stalls (rc_dec6.hip:
16 common steps, then the rare phase; with -DDEC6_TAIL=K the last K steps run
behind the record loads of the lanes stalled by then), on the GPU, for
whichever DEC6_TAIL the library was built with: a lane's first stall on every
step of a block -- the looped steps, the step at which the loads are issued,
the steps behind them -- a second stall directly after, a stall on the
packet's last byte, stalls in a bucket holding 8, 9, 24 and 25 elements
(rc_dec6_rare.h's record boundaries) and a whole wavefront stalling in one
step (the block ends early: no lane can step).

Layout and checks as in tests/test_gpu_limits.py: batches of 256 packets (one
workgroup, lane = index), 200-B noise packets around the case at lanes 0, 31
and 63 of the first and last wavefront; decompress of the oracle's streams
equals the oracle at capacity N and 4096, nothing takes the exact path and
the decoder hands nothing to the lane kernels -- a zero that comes from
tests/limit_cases.py dec6_leaves on the CPU, never from a GPU run.  Bit-exact
or wrong: no tolerance.
"""
import pytest

from tests import dec6_tail_cases as tc
from tests import limit_cases as lc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_limits import _check  # noqa: E402
from tests.test_gpu_wide import _coder  # noqa: E402

GROUPS = {
    "first_repeat": lambda: lc.case_batches(tc.first_repeat_cases()),
    "second_repeat": lambda: lc.case_batches(tc.second_repeat_cases()),
    "last_byte": lambda: lc.case_batches([tc.last_byte_case()]),
    "record_edges": lambda: lc.case_batches(tc.record_edge_cases()),
    "whole_wave": tc.whole_wave_batches,
}


@pytest.fixture(scope="module")
def fast():
    c = _coder()
    yield c
    c.close()


def test_cases_sit_where_planned():
    for c in tc.all_cases():
        assert tc.repeats(c.packet)[0] == tc.planned_first_repeat(c), c.name
    for b in tc.whole_wave_batches():
        r = int(b.name.split("_r")[1])
        assert all(tc.repeats(p)[0] == tc.BASE + r for p in b.packets[:64]), b.name
        assert len(set(b.packets[:64])) == 1


@pytest.mark.parametrize("group", list(GROUPS))
def test_tail_stalls_exact_and_kept(fast, group):
    for b in GROUPS[group]():
        assert b.dec_lanes == 0 and not any(lc.dec6_leaves(p) for p in b.packets), b.name
        _check(fast, b, routed=True, compress=False)
