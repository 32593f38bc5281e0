#!/usr/bin/env python3
"""A schedule model of one decoding wavefront of rc_decompress_dec6s on random
packets (C2) -- a model, not a measurement; numpy only, no GPU:

    python tools/dec6_sched_model.py [--block 16] [--tail 0] [--rare 4.1] [--hidden 2.0]
                                     [--phase 0.74] [--waves 32] [--size 1200] [--sweep]

64 lanes, one packet each.  A lane stalls at position j when the bigram
(x[j-1], x[j]) occurred before in its packet (rc_dec6.hip: an order-1 hit, or
the order-2 context behind one), about j / 65536 per position.  The wavefront
takes common steps -- one cost unit each -- until `block` of them are done or
no lane can step, then serves its stalled lanes in one rare iteration (`rare`
units; a second stall directly behind the first is ignored: rare on random
data) and pays `phase` units per phase.  With --tail K the records of the
lanes stalled after block - K steps are requested there; the phase serves
those at `hidden` units, the lanes that stalled in the last K steps wait for
the next phase (DEC6_TAIL), and a block no lane can finish serves everyone
at the full `rare`.

Printed: stalls per packet, rare iterations per wavefront, lanes served per
iteration, common steps and the wavefront's length in step units (mean over
the waves).  Calibration against the round-4 phase stamps
(profiles/r4_dec6s_phase_c2.log): rare = 12.2 k / 2.95 k cycles = 4.1,
phase = 0.74; the model gives 79.6 iterations of 8.75 lanes, the stamps 83.7
of 8.4.
"""
import argparse

import numpy as np

LANES = 64


def packet_stalls(rng, n):
    """stall[j]: the bigram ending at position j of a random n-byte packet occurred before."""
    x = rng.integers(0, 256, n, dtype=np.int64)
    bg = x[:-1] * 256 + x[1:]
    _, first = np.unique(bg, return_index=True)
    st = np.ones(n, bool)
    st[0] = False
    st[first + 1] = False
    return st


def wave(stalls, block, tail, rare, hidden, phase):
    n = stalls.shape[1]
    pos = np.zeros(LANES, int)
    stalled = np.zeros(LANES, bool)
    ready = np.zeros(LANES, bool)
    t, iters, served, common = 0.0, 0, 0, 0
    while (pos < n).any():
        s = 0
        early = False
        ready[:] = False
        while True:
            go = ~stalled & (pos < n)
            idx = np.flatnonzero(go)
            at = np.zeros(LANES, bool)
            at[idx] = stalls[idx, pos[idx]]
            stalled |= at
            pos[go & ~at] += 1
            t += 1
            common += 1
            s += 1
            if tail and s == block - tail:
                ready = stalled.copy()
            if not (~stalled & (pos < n)).any():
                early = s < block - tail or not tail
                break
            if s >= block:
                break
        if tail and not early:
            who, cost = ready, hidden
        else:
            who, cost = stalled.copy(), rare
        if who.any():
            idx = np.flatnonzero(who)
            pos[idx] += 1
            stalled[idx] = False
            iters += 1
            served += len(idx)
            t += cost
        t += phase
    return t, iters, served, common


def run(waves, **kw):
    r = np.array([wave(w, **kw) for w in waves])
    return {"step units": r[:, 0].mean(), "max": r[:, 0].max(), "rare iterations": r[:, 1].mean(),
            "lanes per iteration": r[:, 2].sum() / max(r[:, 1].sum(), 1), "common steps": r[:, 3].mean()}


def show(name, res):
    print(f"{name:34s} {res['step units']:7.1f} units (max {res['max']:7.1f})  iterations {res['rare iterations']:5.1f}"
          f"  lanes/iteration {res['lanes per iteration']:5.2f}  common steps {res['common steps']:7.1f}")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--block", type=int, default=16)
    ap.add_argument("--tail", type=int, default=0)
    ap.add_argument("--rare", type=float, default=4.1)
    ap.add_argument("--hidden", type=float, default=2.0)
    ap.add_argument("--phase", type=float, default=0.74)
    ap.add_argument("--waves", type=int, default=32)
    ap.add_argument("--size", type=int, default=1200)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--sweep", action="store_true", help="block lengths, rare costs and tails around the arguments")
    a = ap.parse_args()
    rng = np.random.default_rng(a.seed)
    waves = [np.array([packet_stalls(rng, a.size) for _ in range(LANES)]) for _ in range(a.waves)]
    print(f"stalls per packet {np.mean([w.sum() / LANES for w in waves]):.2f}")
    kw = dict(block=a.block, tail=a.tail, rare=a.rare, hidden=a.hidden, phase=a.phase)
    show(f"block {a.block} tail {a.tail} rare {a.rare}", run(waves, **kw))
    if a.sweep:
        for b in (8, 12, 16, 20, 24, 32):
            show(f"block {b} tail 0 rare {a.rare}", run(waves, **{**kw, "block": b, "tail": 0}))
        for r in (3.0, 2.0):
            show(f"block {a.block} tail 0 rare {r}", run(waves, **{**kw, "tail": 0, "rare": r}))
        for k in (1, 2, 3):
            for h in (a.hidden, (a.hidden + a.rare) / 2):
                show(f"block {a.block} tail {k} hidden {h:.2f}", run(waves, **{**kw, "tail": k, "hidden": h}))


if __name__ == "__main__":
    main()
