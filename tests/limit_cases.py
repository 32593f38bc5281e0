"""Packets that sit on a fast-path limit and one past it -- TEST INFRASTRUCTURE.

Both directions run a fast kernel first and hand what it cannot take to the
next one; every hand-over sits at a hard-coded limit that is also the size of
a fixed array (an LDS field, a per-lane record).  The generators here are
exact, not random draws: each returns named packets on a limit and one past
it, with what the host models say about each.  tests/test_limit_cases.py
checks every claim against the oracle, tests/proto/twopass.py and the host
build of the per-lane code; tests/test_gpu_limits.py runs the same packets
through the kernels and compares the routing with these claims.

Plain Python: no GPU, no fixtures.  Where a packet needs bytes that mean
nothing, they come from noise() (a fixed LCG), never from a library's random
generator, so that the packets are the same everywhere.
"""
from __future__ import annotations

from functools import lru_cache
from typing import List, NamedTuple

from tests.proto import twopass

# ---- the limits, as the kernels spell them (file, constant)
DEC6_O1_ELEMS = 28        # rc_dec6_rare.h kTabCap: order-1 elements a bucket's two records hold
DEC6_REC1_ELEMS = 8       # rc_dec6_rare.h rec_addr: elements 0-7 in the 16-B record, 8-27 in the 48-B one
DEC6_O1_HITS = 7          # rc_dec6.hip rare phase: (st >> 5) >= 7 leaves (3 bits of the bucket byte)
DEC6_O2_HITS = 4          # rc_dec6.hip hl[4]: order-2 hits of a model segment kept in registers
DEC6_RESETS = 2           # rc_dec6.hip can_reset6: segments after the first, each starting below 4096
DEC6_WAVE_BAIL = 16       # rc_dec6.hip kWaveBail6: leavers of a wavefront after which the rest follow
VERIFY_FAST_DWORDS = 512  # rc_dec6.hip 64 * kVerDw: output dwords of rc_dec6_verify's pipelined path
ENC2_BUCKET = 64          # rc_enc2.hip kE2Bucket: positions per bucket of the narrow scan
ENC2_RCP_TOP = 441        # rc_enc2.hip kRcpTab - 1 = 5 * 63 + 2 * 63: the largest total of a narrow record
ENC2_MAX_LEN = 1919       # rc_enc2.hip kE2MaxLen: no model reset below 1920 B
ENC2_SLOT_MAX = 4096      # rc_enc2.hip kE2SlotMax
ENC2_WINDOW = 2048        # rc_enc2.hip scan_main: a narrow window holds 2048 - (input address mod 16) bytes
ENC2_SCAN_LAYOUTS = (1216, 1408, 2048)      # rc_enc2.hip kWideSmallL, kScanMidL, the full layout (by max_len)
ENC2_WSCAN_LAYOUTS = (1216, 2048, 4096)     # rc_enc2.hip WScanLdsT<L>: rc_enc2_wscan_s, _wscan, _wscan_l
WIDE_DENSE = 32           # rc_enc2.hip kWideDense: longer runs of a big bucket take the dense walk
SUB_RESCALE_COUNT = 251   # compress.c:313: a count above it halves the context (126 visits, then every 63)
LANE3_O1_SYMS = 12        # rc_lane3.hip ctx_update cap = 4 * NV, NV = 3: symbols of an order-1 record, then dense
LANE3_O2_SYMS = 24        # rc_lane3.hip ctx_update cap = 4 * NV, NV = 6: symbols of a big order-2 record, then dense


class Case(NamedTuple):
    name: str
    packet: bytes
    dec_leaves: bool      # the record-light decoder (rc_dec6.hip) leaves it to the lane kernels
    narrow: bool          # the narrow scan takes it (twopass.scan); else the wide mode (twopass.scan_wide)


def noise(n: int, seed: int, lo: int = 0, hi: int = 256) -> bytes:
    """n bytes in [lo, hi) from a fixed LCG (Numerical Recipes' constants)."""
    s = (seed * 2654435761 + 12345) & 0xFFFFFFFF
    out = bytearray()
    for _ in range(n):
        s = (s * 1664525 + 1013904223) & 0xFFFFFFFF
        out.append(lo + ((s >> 16) * (hi - lo) >> 16))
    return bytes(out)


# ---------------------------------------------------------------- host models

@lru_cache(maxsize=64)
def _scan(p: bytes):
    """(order 2 found, order 1 found, reset point) of p as one model segment."""
    _, f2, f1 = twopass._scan_wide_segment(p)
    return f2, f1, twopass._reset_point(p, f2, f1)


def _segments(p: bytes):
    """The model segments of p (compress.c:148-157) as (start, f2, f1) with
    per-position flags relative to the start; a reset after the last byte
    yields one more, empty, segment start."""
    s, out = 0, []
    while True:
        f2, f1, r = _scan(p[s:])
        out.append((s, f2, f1))
        if r is None:
            return out, None
        s += r + 1
        if s >= len(p):
            return out, s          # the model resets after the packet's last byte


def dec6_leaves(p: bytes) -> bool:
    """rc_dec6.hip's own limits on a valid stream of packet p (the header's
    "off the fast path" list), from the packet's bytes: per model segment and
    bucket, a 29th order-1 visit or an 8th order-1 hit; per segment, a 5th
    order-2 hit; a third reset, or one that would start a segment at 4096."""
    if not p:
        return False
    segs, tail = _segments(p)
    starts = [s for s, _, _ in segs[1:]] + ([tail] if tail is not None else [])
    if len(starts) > DEC6_RESETS or any(s >= 4096 for s in starts):
        return True
    for k, (s, f2, f1) in enumerate(segs):
        end = segs[k + 1][0] if k + 1 < len(segs) else len(p)
        vis, hit, h2 = {}, {}, 0
        for i in range(1, end - s):
            b = p[s + i - 1]
            if i >= 2 and f2[i]:
                h2 += 1
                if h2 > DEC6_O2_HITS:
                    return True
                continue
            vis[b] = vis.get(b, 0) + 1
            if vis[b] > DEC6_O1_ELEMS:
                return True
            if f1[i]:
                hit[b] = hit.get(b, 0) + 1
                if hit[b] > DEC6_O1_HITS:
                    return True
    return False


def _big_bucket(w: bytes) -> bool:
    cnt = [0] * 256
    for i in range(1, len(w)):
        cnt[w[i - 1]] += 1
    return max(cnt) > ENC2_BUCKET


def enc2_route(p: bytes, mis: int = 0, max_len: int = 0) -> str:
    """Where rc_enc2.hip's launch codes packet p of a batch whose longest
    packet is max_len (default: p's length), p at input address mod 16 = mis:
    "narrow", "wide" or "lanes".  scan_main takes windows of 2048 - mis bytes,
    one per model segment; a window with a bucket over 64 positions sends the
    packet to the wide scan, whose windows are as long as its layout; a model
    segment longer than the window leaves the packet to the lane kernels, as
    does a packet longer than the launch's slots (max_len, at most 4096)."""
    n = len(p)
    max_len = max_len or n
    if n == 0:
        return "narrow"
    if n > min(max_len, ENC2_SLOT_MAX):
        return "lanes"

    def windows(size, narrow: bool) -> str:
        s = 0
        while True:
            w = p[s: s + size(s)]
            if narrow and _big_bucket(w):
                return "big"
            if n <= ENC2_MAX_LEN:
                return "ok"
            r = _scan(w)[2]
            if r is None:
                return "ok" if s + len(w) >= n else "lanes"
            s += r + 1
            if s >= n:
                return "ok"

    r = windows(lambda s: ENC2_WINDOW - ((mis + s) & 15), True)
    if r != "big":
        return "narrow" if r == "ok" else "lanes"
    wide_l = next(l for l in ENC2_WSCAN_LAYOUTS if min(max_len, ENC2_SLOT_MAX) <= l)
    return "wide" if windows(lambda s: wide_l, False) == "ok" else "lanes"


def _case(name: str, packet, dec_leaves=None) -> Case:
    p = bytes(packet)
    assert all(0 <= b < 256 for b in p)
    return Case(name, p, dec6_leaves(p) if dec_leaves is None else dec_leaves, twopass.scan(p) is not None)


# ------------------------------------------------- the record-light decoder's records

def o1_elements() -> List[Case]:
    """Bucket 0 with k order-1 elements, every follower new: the 16-B record
    holds 8, the 48-B record the next 20 (kTabCap = 28)."""
    return [_case(f"o1_elements/k{k}", [b for i in range(k) for b in (0, 1 + i, 100 + i)], k > DEC6_O1_ELEMS)
            for k in (DEC6_REC1_ELEMS, DEC6_REC1_ELEMS + 1, DEC6_O1_ELEMS, DEC6_O1_ELEMS + 1, DEC6_O1_ELEMS + 2)]


def o1_hits(hs=(DEC6_O1_HITS, DEC6_O1_HITS + 1, DEC6_O1_HITS + 2)) -> List[Case]:
    """Order-1 context 0 finds symbol 200 h times (its order-2 contexts
    (10 + i, 0) are all new)."""
    return [_case(f"o1_hits/h{h}", [b for i in range(h + 1) for b in (10 + i, 0, 200)], h > DEC6_O1_HITS) for h in hs]


def o2_hits() -> List[Case]:
    """Order-2 context (1, 0) finds symbol 2 m times."""
    return [_case(f"o2_hits/m{m}", [b for i in range(m + 1) for b in (1, 0, 2, 50 + 2 * i, 51 + 2 * i)],
                  m > DEC6_O2_HITS) for m in (DEC6_O2_HITS, DEC6_O2_HITS + 1, DEC6_O2_HITS + 2)]


# ------------------------------------------------------------ the encoder's scans

def bucket_positions() -> List[Case]:
    """Bucket 0 with k positions whose followers are all distinct: at 64 the
    last record's order-1 total is 5 * 63 + 2 * 63 = 441, the top entry of the
    code pass's reciprocal table (kRcpTab); 65 positions take the wide mode."""
    out = [_case(f"bucket_positions/k{k}", [b for i in range(k) for b in (0, 1 + i, 70 + i)], True)
           for k in (ENC2_BUCKET - 1, ENC2_BUCKET, ENC2_BUCKET + 1)]
    assert [c.narrow for c in out] == [True, True, False]
    return out


LONG_RUNS = ((18, 33, 1216), (18, 32, 1216), (31, 33, 2048), (62, 33, 4096))   # (runs, visits each, wide layout)


def long_runs() -> List[Case]:
    """Bucket 255 with nr runs of r visits (contexts (k, 255) for k < nr), the
    most long runs (> kWideDense visits) a packet of the layout's length can
    hold in one bucket: WScanLdsT<L>::runs has L / 64 + 2 entries.  The last
    run of [k, 255] * r is one visit short (the packet ends on its 255);
    "+1" appends a byte, so that all nr runs are long."""
    out = []
    for nr, r, layout in LONG_RUNS:
        p = bytes(b for k in range(nr) for b in [k, 255] * r)
        assert len(p) + 1 <= layout and nr <= layout // 64 + 2
        out.append(_case(f"long_runs/{nr}x{r}", p, True))
        if r > WIDE_DENSE:
            out.append(_case(f"long_runs/{nr}x{r}+1", p + bytes([nr]), True))
    return out


def one_context() -> List[Case]:
    """n zero bytes: contexts 0 and (0, 0) alone; (0, 0) rescales at its 126th
    visit (position 127) and every 63 visits after."""
    return [_case(f"one_context/n{n}", bytes(n), True) for n in (127, 128, 129, 190, 191, 192, 254, 255)]


def rescale_lane_sweep_o2() -> List[Case]:
    """Context (0, 0) sees symbol 1 k times, then zeros: its first rescale
    falls on each lane of a dense-walk round in turn (k = 0..63), the second
    63 visits later."""
    return [_case(f"rescale_sweep_o2/k{k}", bytes([0, 0, 1] * k) + bytes(300), True) for k in range(64)]


def rescale_lane_sweep_o1(m: int = 200) -> List[Case]:
    """The order-1 counterpart: context 0 sees symbol 1 k times, then symbol 2
    m times, each visit behind an order-2 context (a, 0) that lacks the
    symbol (a = 3 + j: at most one visit with 1 and one with 2)."""
    out = []
    for k in range(64):
        p = [b for j in range(k) for b in (3 + j, 0, 1)] + [b for j in range(m) for b in (3 + j, 0, 2)]
        out.append(_case(f"rescale_sweep_o1/k{k}", p, True))
    return out


def dense_edge() -> List[Case]:
    """Runs of kWideDense and kWideDense + 1 visits inside a bucket over 64
    positions: the closed form against the dense walk.  o2: context (1, 0)
    with r visits over 5 symbols, 40 more positions in bucket 0; o1: bucket 0's
    order-1 visits are exactly r (context (1, 0) finds symbol 2 39 times)."""
    out = []
    for r in (WIDE_DENSE, WIDE_DENSE + 1):
        p = [b for j in range(r) for b in (1, 0, 2 + j % 5)] + [b for j in range(40) for b in (10 + j, 0, 100 + j)]
        out.append(_case(f"dense_edge/o2_r{r}", p, True))
        p = [1, 0, 2] * 40 + [b for j in range(r - 1) for b in (10 + j, 0, 100 + j)]
        out.append(_case(f"dense_edge/o1_r{r}", p, True))
    return out


# ------------------------------------------------------------------ the model reset

def _reset_prefix(seed: int):
    """Noise and the index r of the byte after which its model resets."""
    p = noise(2200, seed)
    _, f2, f1 = twopass._scan_wide_segment(p)
    r = twopass._reset_point(p, f2, f1)
    assert r is not None and ENC2_MAX_LEN < r + 1 < ENC2_WINDOW
    return p, r


def reset_edges() -> List[Case]:
    """compress.c:148-157 at 4094 nodes: the reset after the packet's last
    byte (it changes nothing), after the byte before it, and nowhere (one
    byte short); two resets; and a first reset after byte 4095, where the
    record-light decoder's next segment would start at 4096 (can_reset6).
    (A third reset below 4096 B does not exist: a byte makes three nodes at
    most, the root's only for its first 256 symbols, so a segment is at least
    (4094 - 257) / 2 = 1918 B long and the third would end past byte 5754.)"""
    p, r = _reset_prefix(5)
    out = [_case("reset_edges/short", p[:r], False),
           _case("reset_edges/after_last", p[: r + 1], False),
           _case("reset_edges/before_last", p[: r + 2], False)]
    q, r2 = _reset_prefix(6)
    two = p[: r + 1] + q[: r2 + 1] + noise(100, 7)
    out.append(_case("reset_edges/two", two, False))
    out.append(_case("reset_edges/at_4095", reset_at_4095(), True))
    return out


def reset_at_4095() -> bytes:
    """4096 bytes whose 4094th node comes with the last byte: zeros (one node
    each at most), then 1931 bytes of noise (two or three each; the split
    found by search, checked here)."""
    p = bytes(4096 - 1931) + noise(1931, 40, 1)
    _, f2, f1 = twopass._scan_wide_segment(p)
    assert twopass._reset_point(p, f2, f1) == 4095
    return p


# --------------------------------------------------------------- the lane kernels' records

def lane3_records() -> List[Case]:
    """One order-1 context with 12 / 13 distinct symbols and one order-2
    context with 24 / 25 (rc_lane3.hip ctx_update: cap = 4 * NV, NV = 3 and 6):
    the record on its limit, and the step to the dense block; each symbol
    then looked up again."""
    out = []
    for k in (LANE3_O1_SYMS, LANE3_O1_SYMS + 1):
        out.append(_case(f"lane3_records/o1_{k}", [b for a in (30, 60) for i in range(k) for b in (a + i, 0, 100 + i)]))
    for k in (LANE3_O2_SYMS, LANE3_O2_SYMS + 1):
        out.append(_case(f"lane3_records/o2_{k}", [b for i in range(k) for b in (1, 0, 100 + i)] * 2))
    return out


# ----------------------------------------------------------------------- length edges

ENC_LENGTH_EDGES = (1216, 1408, 1919, 2048, 4095, 4096)


def length_content(n: int, kind: str, seed: int = 0) -> bytes:
    """narrow: noise (buckets of about n / 256 positions: none over 64 up to
    4097 B, which the caller checks); wide: three bytes of four zero."""
    if kind == "narrow":
        return noise(n, 100 + seed)
    z = noise(n, 200 + seed)
    v = noise(n, 300 + seed, 1)
    return bytes(v[i] if z[i] < 64 else 0 for i in range(n))


def verify_sweep():
    """Decoded lengths 2040..2052 for rc_dec6_verify's fast path (at most 512
    output dwords counted from the aligned dword of the first byte: between
    2045 and 2048 B by the output's offset mod 4).  "flat": content that the
    decoder keeps and that does not reset before 2052 B (flat_content);
    "noise": random bytes, which may reset near 2047 B."""
    out = []
    for n in range(2040, 2053):
        out.append(_case(f"verify_sweep/flat_n{n}", flat_content(n), False))
        out.append(_case(f"verify_sweep/noise_n{n}", noise(n, 400), None))
    return out


def flat_content(n: int) -> bytes:
    """A packet the record-light decoder keeps, with no model reset, at any
    length up to 4096: passes of 512 bytes x, x + 1, x + 1 + e, x + 2 + e, ...
    with an even stride e of the pass's own.  The bigram (x, x + 1) returns in
    every pass behind another byte (an order-1 hit: one node, not two), the
    bigram (y, y + e) is new, no trigram ever repeats (no order-2 hit), and a
    bucket gets two positions per pass: 16 elements and 7 hits at most."""
    out, x, k = [], 0, 0
    while len(out) < n:
        e = 2 * k + 2
        for _ in range(256):
            out += [x, (x + 1) & 255]
            x = (x + 1 + e) & 255
        k += 1
    return bytes(out[:n])


def verify_fast(n: int, out_off: int) -> bool:
    """rc_dec6_verify takes an n-byte output at offset out_off on its pipelined path."""
    lead = out_off & 3
    return (lead + n + 3) // 4 <= VERIFY_FAST_DWORDS


def all_packet_cases() -> List[Case]:
    """Every single-packet case (the length edges and the verify sweep are batches of their own)."""
    out = []
    for g in (o1_elements, o1_hits, o2_hits, bucket_positions, long_runs, one_context, rescale_lane_sweep_o2,
              rescale_lane_sweep_o1, dense_edge, reset_edges, lane3_records):
        out += g()
    assert len({c.name for c in out}) == len(out)
    return out


def filler(n: int, seed: int, length: int = 200) -> List[bytes]:
    """Random packets every fast path keeps (tests/test_limit_cases.py checks that)."""
    return [noise(length, 1000 + seed * 4096 + i) for i in range(n)]


# ---------------------------------------------------------------------------- batches

PLACEMENTS = ((0, 0), (0, 31), (0, 63), (-1, 0), (-1, 31), (-1, 63))   # (wavefront: first / last, lane)
BATCH = 256               # rc_dec6.hip kLanes6s: a workgroup of rc_decompress_dec6s decodes 256 packets


class Batch(NamedTuple):
    name: str
    packets: List[bytes]  # batch order; below 1024 packets a packet's lane is its index (rc_route.hip
                          # rc_hip_lane_launch bins by length from 1024 packets up; rc_decompress_dec6s:
                          # slot = blockIdx.x * 256 + lane, pkt = slot without an order list)
    in_mis: dict          # index -> input address mod 16 (other packets lie back to back)
    out_mod: dict         # index -> decoded output's offset mod 4
    enc_lanes: int        # packets the two-pass encoder leaves to the lane kernels (enc2_route)
    dec_lanes: int        # packets the record-light decoder leaves (dec6_leaves, the wave rule included)


def dec_lane_count(packets: List[bytes], leaves: List[bool]) -> int:
    """Leavers of the batch under rc_dec6.hip's wave rule: a wavefront (64
    consecutive packets) with 16 leavers or more leaves whole.  The rule acts
    when the 16th lane has left, so the count is exact only where the others
    are still decoding then: callers keep any 64 consecutive packets below 16
    leavers, or build the wavefront on purpose (wave_bail_batches)."""
    total = 0
    for w in range(0, len(packets), 64):
        k = sum(leaves[w: w + 64])
        total += min(64, len(packets) - w) if k >= DEC6_WAVE_BAIL else k
    return total


def make_batch(name: str, placed, n: int = BATCH, seed: int = 0, fill_len: int = 200, strict: bool = True) -> Batch:
    """placed: (index, Case or bytes, input mis or None, output mod or None);
    the rest 200-B noise packets, which every fast path keeps."""
    assert n % BATCH == 0 and n < 1024
    packets = filler(n, seed, fill_len)
    leaves = [False] * n
    in_mis, out_mod = {}, {}
    for idx, c, mis, om in placed:
        idx %= n
        assert idx not in in_mis, "one case per slot"
        packets[idx] = c.packet
        leaves[idx] = c.dec_leaves
        in_mis[idx] = mis or 0
        if om is not None:
            out_mod[idx] = om
    if strict:        # no 64 consecutive packets with 16 leavers: the wave rule cannot add any
        assert all(sum(leaves[i: i + 64]) < DEC6_WAVE_BAIL for i in range(n - 63))
    max_len = max(len(p) for p in packets)
    enc = sum(enc2_route(packets[i], m, max_len) == "lanes" for i, m in in_mis.items())
    return Batch(name, packets, in_mis, out_mod, enc, dec_lane_count(packets, leaves))


def placed_everywhere(c: Case, n: int = BATCH):
    """c at lanes 0, 31 and 63 of the batch's first and last wavefront."""
    return [((n - 64 if w else 0) + lane, c, 0, None) for w, lane in PLACEMENTS]


def case_batches(cases: List[Case], seed: int = 0) -> List[Batch]:
    """One batch per case, the case at every placement."""
    return [make_batch(c.name, placed_everywhere(c), seed=seed + i) for i, c in enumerate(cases)]


def sweep_batches(cases: List[Case], name: str, seed: int = 0) -> List[Batch]:
    """Six cases per batch, one per placement, the placements rotating from
    batch to batch (the sweeps vary what a scan wavefront sees inside one
    packet; the packet's own lane matters to the code pass and the decoder)."""
    out = []
    for b in range(0, len(cases), 6):
        grp = cases[b: b + 6]
        rot = b // 6
        placed = []
        for j, c in enumerate(grp):
            w, lane = PLACEMENTS[(j + rot) % 6]
            placed.append(((BATCH - 64 if w else 0) + lane, c, 0, None))
        out.append(make_batch(f"{name}/{b}", placed, seed=seed + b))
    return out


def wave_bail_batches() -> List[Batch]:
    """rc_dec6.hip kWaveBail6: 15 early leavers (o1_hits h = 8: off by byte 27)
    among 49 noise packets of 1200 B in the first wavefront -- nobody else
    leaves; 16 among 48 -- the 48, far from done, all follow."""
    lv = o1_hits((DEC6_O1_HITS + 1,))[0]
    assert lv.dec_leaves and len(lv.packet) == 27
    out = []
    for k in (DEC6_WAVE_BAIL - 1, DEC6_WAVE_BAIL):
        long_ones = filler(64, 77, 1200)
        placed = [(4 * j, lv, 0, None) for j in range(k)]
        taken = {i for i, _, _, _ in placed}
        placed += [(i, Case("noise1200", long_ones[i], False, True), 0, None) for i in range(64) if i not in taken]
        b = make_batch(f"wave_bail/{k}", placed, seed=50 + k, strict=False)
        assert b.dec_lanes == (k if k < DEC6_WAVE_BAIL else 64)
        out.append(b)
    return out


def length_edge_batches() -> List[Batch]:
    """The encoder's layouts and windows: a launch picks its LDS layout from
    the batch's longest packet, so each edge is a batch of its own whose
    longest packet is L, then L + 1, at input address mod 16 = 0 and 15,
    with narrow (noise) and wide (mostly zero) content."""
    out = []
    todo = [(n, kind, mis) for n in sorted({m for L in ENC_LENGTH_EDGES for m in (L, L + 1)})
            for kind in ("narrow", "wide") for mis in (0, 15)]
    # the narrow window itself (2048 - mis bytes): content that is narrow and never resets
    todo += [(n, "flat", mis) for n in (ENC2_WINDOW - 15, ENC2_WINDOW - 14, ENC2_WINDOW, ENC2_WINDOW + 1) for mis in (0, 15)]
    for j, (n, kind, mis) in enumerate(todo):
        c = _case(f"length_edge/{kind}_n{n}_mis{mis}", flat_content(n) if kind == "flat" else length_content(n, kind))
        assert c.narrow == (kind != "wide" and n <= ENC2_MAX_LEN)
        w, lane = PLACEMENTS[j % 6]
        out.append(make_batch(c.name, [((BATCH - 64 if w else 0) + lane, c, mis, None)], seed=300 + j))
    return out


def verify_batch() -> Batch:
    """verify_sweep()'s packets, each at the four output offsets mod 4."""
    placed = []
    for j, c in enumerate(verify_sweep()):
        for om in range(4):
            placed.append((len(placed) * 2 + (j & 1), c, (5 * j + om) & 15, om))
    return make_batch("verify_sweep", placed, seed=400)
