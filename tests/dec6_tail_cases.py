"""Packets whose first stall in the record-light decoder falls on a chosen
step of a block -- TEST INFRASTRUCTURE (tests/test_gpu_dec6_tail.py,
tests/test_dec6_tail_host.py).

rc_dec6.hip decodes one byte per common step and stalls a lane at position j
when the bigram (x[j-1], x[j]) has occurred before in the packet (an order-1
hit, or an order-2 hit directly behind one).  Every DEC6_BLOCK = 16 steps the
wavefront serves its stalled lanes; the last DEC6_TAIL steps of a block run
behind the record loads of the lanes stalled by then.  A packet without any
repeated bigram before position 32 + r therefore takes its first stall in
step r of the third block, whatever its lane.

Plain Python on tests/limit_cases.py's fixed noise: the same packets everywhere.
"""
from __future__ import annotations

from functools import lru_cache
from typing import List

import numpy as np

from tests import limit_cases as lc

BLOCK = 16                # rc_dec6.hip DEC6_BLOCK
BASE = 32                 # the planted repeats sit in the third block
LENGTH = 200              # tests/limit_cases.py's filler length
RECORD_EDGES = (lc.DEC6_REC1_ELEMS, lc.DEC6_REC1_ELEMS + 1, 24, 25)   # rc_dec6_rare.h rec_load: t1 > 8, t1 > 24


def repeats(p: bytes) -> List[int]:
    """Positions j whose bigram (p[j-1], p[j]) occurred at an earlier position (numpy)."""
    x = np.frombuffer(p, np.uint8).astype(np.int64)
    if len(x) < 2:
        return []
    bg = x[:-1] * 256 + x[1:]
    _, first = np.unique(bg, return_index=True)
    again = np.ones(len(bg), bool)
    again[first] = False
    return [int(i) + 1 for i in np.flatnonzero(again)]


@lru_cache(maxsize=None)
def planted(pos: int, second: bool = False, n: int = LENGTH) -> bytes:
    """n noise bytes whose only repeated bigram sits at position pos (second:
    and the one at pos + 1, the trigram before it repeating), copied from
    positions 4-6."""
    want = [pos, pos + 1] if second else [pos]
    for seed in range(5000, 5400):
        x = bytearray(lc.noise(n, seed))
        if repeats(bytes(x)):
            continue
        x[pos - 1], x[pos] = x[4], x[5]
        if second:
            x[pos + 1] = x[6]
        if repeats(bytes(x)) == want:
            return bytes(x)
    raise AssertionError(("no seed plants", pos, second))


def record_edge(k: int) -> bytes:
    """tests/limit_cases.py o1_elements' bucket 0 with k order-1 elements, then
    the bigram (0, 1) again: the stall finds k elements in the bucket's records."""
    return bytes([b for i in range(k) for b in (0, 1 + i, 100 + i)] + [0, 1])


def case(name: str, p: bytes) -> lc.Case:
    c = lc._case(name, p)
    assert not c.dec_leaves, name              # (from lc.dec6_leaves: the decoder keeps it)
    return c


def first_repeat_cases() -> List[lc.Case]:
    return [case(f"tail/first_r{r}", planted(BASE + r)) for r in range(BLOCK)]


def second_repeat_cases() -> List[lc.Case]:
    return [case(f"tail/second_r{r}", planted(BASE + r, True)) for r in (12, 13, 14, 15)]


def last_byte_case() -> lc.Case:
    return case("tail/last_byte", planted(LENGTH - 1))


def record_edge_cases() -> List[lc.Case]:
    return [case(f"tail/bucket_k{k}", record_edge(k)) for k in RECORD_EDGES]


def planned_first_repeat(c: lc.Case) -> int:
    """Where the case's first repeat was planned, from its name."""
    kind = c.name.split("/")[1]
    if kind.startswith(("first_r", "second_r")):
        return BASE + int(kind.split("_r")[1])
    if kind == "last_byte":
        return LENGTH - 1
    return 3 * int(kind.split("_k")[1]) + 1


def all_cases() -> List[lc.Case]:
    return first_repeat_cases() + second_repeat_cases() + [last_byte_case()] + record_edge_cases()


def whole_wave_batches() -> List[lc.Batch]:
    """All 64 lanes of the first wavefront stall in the same step (r = 3: the
    block ends early, no lane can step; r = 15: in a block's last step)."""
    out = []
    for r in (3, 15):
        c = case(f"tail/wave_r{r}", planted(BASE + r))
        out.append(lc.make_batch(c.name, [(i, c, 0, None) for i in range(64)]))
    return out
