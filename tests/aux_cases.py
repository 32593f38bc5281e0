"""Edge cases for the kernels around the range coder -- TEST INFRASTRUCTURE.

rc_pack.hip (copy_bytes, the pack / unpack scans, rc_gather16, rc_slot_copy),
rc_crc32.hip, rc_dgram.hip and rc_multi_plan.hip move or checksum every byte
of a batch, and each has branches that whole-pipeline batches of ~1200-byte
packets leave alone.  The builders here are exact, not random draws: each
returns numpy arrays together with the class every case is meant to hit and a
plain reference (numpy slicing, zlib, the oracle's framing, shard_ranges).
tests/test_aux_cases.py checks on the CPU that the cases sit where they
claim; tests/test_gpu_aux_kernels.py runs them through the kernels.

No GPU and no torch.  The datagram builders need the oracle library, so they
are functions (cached), not module constants: importing this file needs
nothing built.
"""
from __future__ import annotations

import zlib
from functools import lru_cache
from typing import List, NamedTuple, Tuple

import numpy as np

SRC_CANARY = 0xA5         # fills a source buffer outside its packets
DST_CANARY = 0x5A         # fills a destination before the kernel runs
PAD = 64                  # bytes of canary before the first and after the last slot (>= one 16-B granule)


def payload(rng, n: int) -> np.ndarray:
    """n random bytes that are never one of the two canaries, so that a byte
    a kernel failed to write, or took from a gap, always shows."""
    v = rng.integers(0, 254, size=n, dtype=np.uint8)
    v += (v >= min(SRC_CANARY, DST_CANARY)).astype(np.uint8)
    v += (v >= max(SRC_CANARY, DST_CANARY)).astype(np.uint8)
    return v


# ------------------------------------------------------------- copy_bytes model

def copy_branch(src_mod4: int, dst_mod4: int, m: int):
    """The branch rc_pack.hip copy_bytes takes for m bytes from an address
    = src_mod4 (mod 4) to an address = dst_mod4 (mod 4): "empty",
    "bytes_only", or (head, tail, sh, nw).  Restates, line for line:

        if (m == 0) return;
        const uintptr_t d0 = reinterpret_cast<uintptr_t>(dst), d1 = d0 + m;
        const uintptr_t b0 = (d0 + 3) & ~static_cast<uintptr_t>(3), b1 = d1 & ~static_cast<uintptr_t>(3);
        if (b0 >= b1) {                                      // no whole dword inside
            if (lane < m) dst[lane] = src[lane];
            return;
        }
        const uint32_t head = static_cast<uint32_t>(b0 - d0), tail = static_cast<uint32_t>(d1 - b1);
        ...
        const uintptr_t s0 = reinterpret_cast<uintptr_t>(src) + head;   // source of the first whole dword
        const uint32_t sh = static_cast<uint32_t>(s0 & 3);
        ...
        const uint32_t nw = static_cast<uint32_t>((b1 - b0) >> 2);
        for (uint32_t k = lane; k < nw; k += 64) {

    head / tail: bytes stored singly before / after the whole dwords; sh: the
    alignbyte shift (0: plain dword copy); nw: whole dwords (the k loop wraps
    above 64)."""
    if m == 0:
        return "empty"
    d0 = dst_mod4 & 3
    d1 = d0 + m
    b0, b1 = (d0 + 3) & ~3, d1 & ~3
    if b0 >= b1:
        return "bytes_only"
    head, tail = b0 - d0, d1 - b1
    sh = ((src_mod4 & 3) + head) & 3
    return head, tail, sh, (b1 - b0) >> 2


# ------------------------------------------------------------------ copy layout

COPY_LENGTHS: Tuple[int, ...] = tuple(range(0, 17)) + tuple(range(250, 271)) + (1199, 1200, 1201, 4095, 4096, 4097)
COPY_GAPS = 7             # gaps 0..6 between consecutive slots


class Layout(NamedTuple):
    src: np.ndarray       # uint8: SRC_CANARY everywhere outside the packets
    off: np.ndarray       # uint64 offset of each packet's slot (the same in source and destination)
    ln: np.ndarray        # uint32
    want: np.ndarray      # uint8: the destination after a copy of every packet over DST_CANARY


def slot_offsets(ln, gap_of=lambda i: i % COPY_GAPS, pad: int = PAD):
    """Slots of exactly ln[i] bytes, gap_of(i) bytes after the previous one;
    returns (off, total) with `pad` bytes before the first and after the last."""
    off = np.zeros(len(ln), np.uint64)
    pos = pad
    for i, l in enumerate(ln):
        pos += gap_of(i)
        off[i] = pos
        pos += int(l)
    return off, pos + pad


def packet_bytes_index(off, ln) -> Tuple[np.ndarray, np.ndarray]:
    """(slot index, packed index) of every packet byte in batch order:
    packed[p] == buf[s] describes the back-to-back concatenation."""
    ln64 = np.asarray(ln, np.int64)
    total = int(ln64.sum())
    start = np.cumsum(ln64) - ln64
    p = np.arange(total, dtype=np.int64)
    s = np.repeat(np.asarray(off, np.int64) - start, ln64) + p
    return s, p


def fill_slots(off, ln, total: int, seed: int) -> Layout:
    rng = np.random.default_rng(seed)
    src = np.full(total, SRC_CANARY, np.uint8)
    s, _ = packet_bytes_index(off, ln)
    src[s] = payload(rng, len(s))
    want = np.full(total, DST_CANARY, np.uint8)
    for o, l in zip(off, ln):                       # the reference: numpy slicing
        want[int(o): int(o) + int(l)] = src[int(o): int(o) + int(l)]
    return Layout(src, np.asarray(off, np.uint64), np.asarray(ln, np.uint32), want)


def copy_lengths(n: int) -> np.ndarray:
    """COPY_LENGTHS cycled to n packets."""
    return np.array([COPY_LENGTHS[i % len(COPY_LENGTHS)] for i in range(n)], np.uint32)


@lru_cache(maxsize=1)
def copy_layout() -> Layout:
    """Every COPY_LENGTHS value seven times; the gap before packet i is
    (i + i // len(COPY_LENGTHS)) % 7, so that every length meets every gap and
    the slot addresses (and the addresses of their ends) cover every residue
    mod 4.  308 packets, ~150 KB."""
    k = len(COPY_LENGTHS)
    ln = copy_lengths(COPY_GAPS * k)
    off, total = slot_offsets(ln, lambda i: (i + i // k) % COPY_GAPS)
    return fill_slots(off, ln, total, 0xC09)


def copy_branches(lay_off, lay_ln, src_base: int = 0, dst_base: int = 0, dst_off=None) -> list:
    """copy_branch of every packet when the buffers start at the given byte
    addresses (only mod 4 counts); dst_off: the destination offsets where they
    differ from the source's (pack, unpack)."""
    d = lay_off if dst_off is None else dst_off
    return [copy_branch((src_base + int(s)) & 3, (dst_base + int(t)) & 3, int(m))
            for s, t, m in zip(lay_off, d, lay_ln)]


def pack_case(n: int, lengths=None, seed: int = 0) -> Tuple[Layout, np.ndarray]:
    """n gapped slots (COPY_LENGTHS cycled unless given) and their packed form."""
    ln = copy_lengths(n) if lengths is None else np.asarray(lengths, np.uint32)
    gaps = np.arange(n) % COPY_GAPS
    ln64 = ln.astype(np.int64)
    off = (PAD + np.cumsum(gaps + ln64) - ln64).astype(np.uint64)
    total = int(off[-1]) + int(ln[-1]) + PAD
    rng = np.random.default_rng(0x9AC0 + n + seed)
    src = np.full(total, SRC_CANARY, np.uint8)
    s, _ = packet_bytes_index(off, ln)
    packed = payload(rng, len(s))
    src[s] = packed
    want = np.full(total, DST_CANARY, np.uint8)
    want[s] = packed
    return Layout(src, off, ln, want), packed


PACK_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049)   # around the 64-packet workgroup and the 1024-packet segment
PACK_CARRY_N = 262144 + 1024 + 5                       # 258 segments: rc_pack_scan's loop runs twice, with a carry


def segment_sums(ln, per: int = 1024) -> np.ndarray:
    """What rc_pack_scan leaves in bsum: the exclusive prefix sums of the
    1024-packet segments' lengths, then the total."""
    ln64 = np.asarray(ln, np.int64)
    nb = (len(ln64) + per - 1) // per
    sums = np.add.reduceat(ln64, np.arange(0, len(ln64), per)) if len(ln64) else np.zeros(0, np.int64)
    assert len(sums) == nb
    return np.concatenate([[0], np.cumsum(sums)]).astype(np.uint64)


# --------------------------------------------------------------------- gather16

class Gather(NamedTuple):
    src: np.ndarray       # uint8, 16 B of padding at both ends
    soff: np.ndarray      # uint64
    doff: np.ndarray      # uint64
    ln: np.ndarray        # uint32
    dst_bytes: int        # size of the destination (16-B granules, one spare at the end)


def gather_case(ln, src_align: int = 0, seed: int = 0) -> Gather:
    """Source packets in gapped slots and the device offsets rc_hostmem.c
    fill_dev_offsets gives them on the gather path (zc_dev):

        const uint64_t ph = (uintptr_t) (b->in + b->in_off[i]) & 15;
        hio[i] = l ? acc + ph : acc;
        if (l) acc += (ph + l + 15) & ~(uint64_t) 15;

    and upload_direct's source offsets (0 for an empty packet):

        hso[i] = b->in_len[i] ? b->in_off[i] - p->zc_lo : 0;

    src_align: the source buffer's address mod 16 (the phase ph is taken from
    the address, not the offset)."""
    ln = np.asarray(ln, np.uint32)
    n = len(ln)
    ln64 = ln.astype(np.int64)
    gaps = np.arange(n) % COPY_GAPS
    soff = 16 + np.cumsum(gaps + ln64) - ln64
    total = int(soff[-1] + ln64[-1]) + 16
    ph = (src_align + soff) & 15
    span = np.where(ln64 > 0, (ph + ln64 + 15) & ~15, 0)
    acc = np.cumsum(span) - span
    doff = np.where(ln64 > 0, acc + ph, acc)
    rng = np.random.default_rng(0x6A7 + n + seed)
    src = payload(rng, total)                       # the gaps too: whole granules travel
    return Gather(src, np.where(ln64 > 0, soff, 0).astype(np.uint64), doff.astype(np.uint64), ln,
                  int(span.sum()) + 16)


def gather_owned(g: Gather) -> np.ndarray:
    """bool per destination byte: inside a granule owned by a non-empty packet."""
    own = np.zeros(g.dst_bytes, bool)
    for d, l in zip(g.doff, g.ln):
        if l:
            own[int(d) & ~15: (int(d) + int(l) + 15) & ~15] = True
    return own


# -------------------------------------------------------------------------- CRC

def noise_bytes(rng, n: int) -> np.ndarray:
    """n random bytes, drawn eight at a time."""
    return rng.integers(0, 1 << 64, size=(n + 7) // 8, dtype=np.uint64).view(np.uint8)[:n]


def net(v: int) -> int:
    """zlib's CRC -> enet_crc32's return value (ENET_HOST_TO_NET_32 of it)."""
    return int.from_bytes(v.to_bytes(4, "big"), "little")


CRC_SHORT = tuple(range(0, 531)) + tuple(range(1020, 1031)) + tuple(range(4090, 4101))   # one and two 256-B rounds, each +-
CRC_LONG = (8191, 8192, 8193, 65535, 65536, 65537, (1 << 20) + 5)                        # no limit in the ABI
CRC_LONG_STARTS = (0, 5, 10, 15)


class CrcBatch(NamedTuple):
    data: np.ndarray      # uint8; its address must be a multiple of 16 for `start` to hold
    off: np.ndarray       # uint64
    ln: np.ndarray        # uint32
    want: np.ndarray      # uint32, as enet_crc32 returns it


def crc_case_list() -> List[Tuple[int, int]]:
    """(start mod 16, length): CRC_SHORT at all 16 starts, CRC_LONG at four,
    shuffled with a fixed seed so that the sixteen packet groups of a
    wavefront finish in different rounds."""
    cases = [(a, l) for l in CRC_SHORT for a in range(16)] + [(a, l) for l in CRC_LONG for a in CRC_LONG_STARTS]
    order = np.random.default_rng(0xC4C).permutation(len(cases))
    return [cases[i] for i in order]


def crc_reference(data, off, ln) -> np.ndarray:
    return np.array([net(zlib.crc32(data[int(o): int(o) + int(l)].tobytes())) for o, l in zip(off, ln)], np.uint32)


@lru_cache(maxsize=1)
def crc_batch() -> CrcBatch:
    """The case list laid out in one buffer (~8 MB): each packet at the next
    offset with its start residue, 16..31 B of padding after the last (the
    kernel reads whole aligned 16-B granules)."""
    cases = crc_case_list()
    off = np.zeros(len(cases), np.uint64)
    pos = 16
    for i, (a, l) in enumerate(cases):
        pos += (a - pos) % 16
        off[i] = pos
        pos += l
    total = ((pos + 15) & ~15) + 16
    data = noise_bytes(np.random.default_rng(0xC4C32), total)
    ln = np.array([l for _, l in cases], np.uint32)
    return CrcBatch(data, off, ln, crc_reference(data, off, ln))


def crc_restart_batch(n: int, seed: int = 0x4E5) -> CrcBatch:
    """n packets of lengths 0..600 at random alignment (gaps 0..15)."""
    rng = np.random.default_rng(seed)
    ln = rng.integers(0, 601, size=n).astype(np.int64)
    gaps = rng.integers(0, 16, size=n)
    off = 16 + np.cumsum(gaps + ln) - ln
    total = ((int(off[-1] + ln[-1]) + 15) & ~15) + 16
    data = noise_bytes(rng, total)
    return CrcBatch(data, off.astype(np.uint64), ln.astype(np.uint32), crc_reference(data, off, ln))


# -------------------------------------------------------------------- datagrams

MTU = 4096
HEADER_SIZES = (2, 4, 6, 8)      # SENT_TIME x checksum
C_CLASSES = ("c==L-1", "c==L", "c==0,needs L+1", "c==0,wide")
PER_CLASS = 2


def _port():
    from oracle.pyoracle import Coder
    return Coder("port")


def classify_c(port, cmds: bytes):
    """The class of protocol.c:1696's decision for these commands: c is the
    coder's result under outLimit = L, r what the stream needs."""
    L = len(cmds)
    c, _ = port.compress(cmds, out_limit=L, in_limit=L)
    r, _ = port.compress(cmds, out_limit=2 * L + 64, in_limit=L)
    if c == L - 1 and c > 0:
        return "c==L-1"
    if c == L:
        return "c==L"
    if c == 0 and r == L + 1:
        return "c==0,needs L+1"
    if c == 0 and r >= L + 8:
        return "c==0,wide"
    return None


@lru_cache(maxsize=1)
def edge_payloads() -> dict:
    """PER_CLASS command payloads for each class of C_CLASSES, the first found
    among random payloads of a fixed seed (length 1..299, alphabet size from
    {2, 3, 4, 8, 16, 32, 64, 128, 256})."""
    port = _port()
    rng = np.random.default_rng(1696)
    found = {k: [] for k in C_CLASSES}
    for _ in range(20000):
        if all(len(v) >= PER_CLASS for v in found.values()):
            break
        size = int(rng.integers(1, 300))
        alpha = int(rng.choice([2, 3, 4, 8, 16, 32, 64, 128, 256]))
        cmds = rng.integers(0, alpha, size=size, dtype=np.uint8).tobytes()
        k = classify_c(port, cmds)
        if k is not None and len(found[k]) < PER_CLASS and (k != "c==0,wide" or size >= 64):
            found[k].append(cmds)
    assert all(len(v) >= PER_CLASS for v in found.values()), {k: len(v) for k, v in found.items()}
    return found


class Dgram(NamedTuple):
    name: str
    cls: str              # what the case is meant to hit
    hs: int
    checksum: bool
    seed: int
    data: bytes           # assembled datagram (encode) or wire datagram (decode)
    want: bytes           # the oracle's output (b"" where protocol.c drops it)


def _head(sent: bool, k: int, compressed: bool = False) -> bytes:
    word = (0x123 + 17 * k) & 0xFFF | ((k & 3) << 12) | (0x8000 if sent else 0) | (0x4000 if compressed else 0)
    return word.to_bytes(2, "big") + (((0xBEEF + k) & 0xFFFF).to_bytes(2, "big") if sent else b"")


def _three(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 3, size=n, dtype=np.uint8).tobytes()


def _noise(n: int, seed: int) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8).tobytes()


def _assembled(hs: int, total: int, body: str, k: int) -> bytes:
    """An assembled datagram of `total` bytes for header size hs (cut short
    where total < hs); its checksum field holds junk, as before the send."""
    sent, ck = hs in (4, 8), hs in (6, 8)
    head = _head(sent, k) + (b"\xde\xad\xbe\xef" if ck else b"")
    if total <= hs:
        return head[:total]
    return head + (_three if body == "three" else _noise)(total - hs, 1000 * hs + total)


@lru_cache(maxsize=1)
def datagram_encode_cases() -> List[Dgram]:
    from oracle.pyoracle import datagram_encode
    port = _port()
    out = []
    for hs in HEADER_SIZES:
        sent, ck = hs in (4, 8), hs in (6, 8)
        seed = 0x9E3779B9 ^ (hs * 0x01010101)
        raw = []
        for total in (0, 1, hs - 1, hs, hs + 1):
            raw.append((f"len{total}", "short" if total < max(hs, 2) else "tiny", _assembled(hs, total, "noise", total)))
        for total in (4095, 4096):
            raw.append((f"len{total}/noise", "mtu_kept", _assembled(hs, total, "noise", total)))
            raw.append((f"len{total}/three", "mtu_kept", _assembled(hs, total, "three", total)))
        raw.append(("len4097", "mtu_over", _assembled(hs, 4097, "three", 4097)))
        for cls, pays in edge_payloads().items():
            for j, cmds in enumerate(pays):
                raw.append((f"{cls}/{j}", cls, _assembled(hs, hs, "noise", j) + cmds))
        # the COMPRESSED bit on the way in is ignored (protocol.c:1698 clears it)
        for cls in ("c==L-1", "c==0,wide"):
            d = bytearray(_assembled(hs, hs, "noise", 9) + edge_payloads()[cls][0])
            d[0] |= 0x40
            raw.append((f"compressed_bit_in/{cls}", "compressed_bit_in", bytes(d)))
        for name, cls, d in raw:
            out.append(Dgram(f"hs{hs}/{name}", cls, hs, ck, seed, d, datagram_encode(d, ck, seed, port)))
    return out


def _wire_by_hand(hs: int, cmds: bytes, seed: int, port) -> bytes:
    """header | checksum | range-coded cmds with COMPRESSED set, whatever the
    length of cmds: what a sender without the MTU limit would emit (the
    checksum is right, so that only the size can be the reason for a drop)."""
    sent, ck = hs in (4, 8), hs in (6, 8)
    head = _head(sent, 5, compressed=True)
    r, stream = port.compress(cmds, out_limit=len(cmds), in_limit=len(cmds))
    assert 0 < r < len(cmds)
    if ck:
        crc = net(zlib.crc32(head + seed.to_bytes(4, "little") + cmds))
        head += crc.to_bytes(4, "little")
    return head + stream


@lru_cache(maxsize=1)
def datagram_decode_cases() -> List[Dgram]:
    from oracle.pyoracle import datagram_decode
    port = _port()
    raw = []
    for e in datagram_encode_cases():
        if e.want:
            raw.append((e.name + "/wire", "valid", e.hs, e.checksum, e.seed, e.want))
        else:
            raw.append((e.name + "/raw", e.cls, e.hs, e.checksum, e.seed, e.data))
    for hs in HEADER_SIZES:
        ck = hs in (6, 8)
        seed = 0x51ED270B ^ hs
        fit = _wire_by_hand(hs, _three(MTU - hs, 40 + hs), seed, port)
        over = _wire_by_hand(hs, _three(MTU - hs + 1, 50 + hs), seed, port)
        raw.append((f"hs{hs}/decodes_to_mtu", "mtu_fit", hs, ck, seed, fit))
        raw.append((f"hs{hs}/decodes_to_mtu+1", "mtu_over", hs, ck, seed, over))
        # an uncompressed wire of 4097 bytes (protocol.c never receives one; the ABI bounds it)
        raw.append((f"hs{hs}/plain_4097", "mtu_over", hs, ck, seed, _assembled(hs, 4097, "noise", 3)))
        good = next(e for e in datagram_encode_cases() if e.hs == hs and e.cls == "c==L-1")
        plain = next(e for e in datagram_encode_cases() if e.hs == hs and e.cls == "c==L")
        raw.append((f"hs{hs}/wrong_seed", "wrong_seed", hs, ck, good.seed ^ 0x00010000, good.want))
        raw.append((f"hs{hs}/wrong_seed_plain", "wrong_seed", hs, ck, plain.seed ^ 1, plain.want))
        if ck:
            for nm, w in (("compressed", good.want), ("plain", plain.want)):
                b = bytearray(w)
                b[hs - 2] ^= 0x10
                raw.append((f"hs{hs}/checksum_bit/{nm}", "checksum_bit", hs, ck, good.seed, bytes(b)))
        for nm, w in (("short", good.want), ("long", fit)):
            b = bytearray(w)
            b[hs + (len(w) - hs) // 2] ^= 0x04
            raw.append((f"hs{hs}/stream_bit/{nm}", "stream_bit", hs, ck, good.seed if nm == "short" else seed, bytes(b)))
    return [Dgram(n, c, hs, ck, sd, w, datagram_decode(w, ck, sd, port)) for n, c, hs, ck, sd, w in raw]


def datagram_slots(sizes, aligned: bool, step: int = 5, pad: int = PAD):
    """Offsets of slots of the given sizes with canary room between and after
    them: every offset a multiple of 16 (at least 16 B apart), or gaps 0..15
    that put slot i at residue (step i + 1) mod 16 (step odd: every residue)."""
    off = np.zeros(len(sizes), np.uint64)
    pos = pad
    for i, s in enumerate(sizes):
        pos = (pos + 16 + 15) & ~15 if aligned else pos + (step * i + 1 - pos) % 16
        off[i] = pos
        pos += int(s)
    return off, pos + pad


# -------------------------------------------------------------------- plan ties

class PlanCase(NamedTuple):
    name: str
    ln: np.ndarray        # uint32
    ioff: np.ndarray      # uint64
    ooff: np.ndarray      # uint64
    cap: np.ndarray       # uint32
    parts: int
    ties: int             # split points k (0 < k < parts) where a prefix sum equals k / parts of the total exactly


def plan_ties(ln, parts: int) -> int:
    cum = np.concatenate([[0], np.cumsum(np.asarray(ln, np.int64))])
    total = int(cum[-1])
    return sum(1 for k in range(1, parts) if (total * k) % parts == 0 and (total * k) // parts in cum)


def _plan_case(name, ln, parts):
    ln = np.asarray(ln, np.uint32)
    n = len(ln)
    ln64 = ln.astype(np.uint64)
    ioff = (np.cumsum(ln64 + np.uint64(3)) - ln64).astype(np.uint64)            # slots 3 B apart, from 3
    cap = (2 * ln + 64).astype(np.uint32)
    ooff = (np.cumsum(cap.astype(np.uint64)) - cap.astype(np.uint64) + np.uint64(128)).astype(np.uint64)
    return PlanCase(name, ln, ioff, ooff, cap, parts, plan_ties(ln, parts))


def plan_tie_cases() -> List[PlanCase]:
    """Uniform lengths: every split point is an exact tie.  n = 2048, parts = 2
    ties on packet 1023, the last of segment 0; the /zeros variants empty
    packets 1020..1030 (across the segment edge); n = 2051 with those zeros
    ties at 1020, followed by the eleven empty packets."""
    def uniform(n, zeros=False):
        ln = np.full(n, 100, np.uint32)
        if zeros:
            ln[1020:1031] = 0
        return ln
    out = []
    for zeros in (False, True):
        tag = "/zeros" if zeros else ""
        for parts in (2, 3, 4, 8, 64):
            out.append(_plan_case(f"n4096/p{parts}{tag}", uniform(4096, zeros), parts))
        out.append(_plan_case(f"n2048/p2{tag}", uniform(2048, zeros), 2))
    out.append(_plan_case("n2051/p2/zeros", uniform(2051, True), 2))
    out.append(_plan_case("n64/p64", uniform(64), 64))
    return out


def plan_reference(c: PlanCase) -> List[int]:
    """shard.shard_ranges and each part's extents in numpy (as _plan_numpy of
    tests/test_multi.py, with the split from Python instead of the C split)."""
    from enet_amd import shard
    ranges = shard.shard_ranges(c.ln, c.parts)
    first = [a for a, _ in ranges] + [len(c.ln)]
    ext = []
    ln64, cap64 = c.ln.astype(np.uint64), c.cap.astype(np.uint64)
    for a, b in ranges:
        if a == b:
            ext += [2 ** 64 - 1, 0, 2 ** 64 - 1, 0]
        else:
            ext += [int(c.ioff[a:b].min()), int((c.ioff[a:b] + ln64[a:b]).max()),
                    int(c.ooff[a:b].min()), int((c.ooff[a:b] + cap64[a:b]).max())]
    return first + ext
