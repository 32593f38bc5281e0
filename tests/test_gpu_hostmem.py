"""Host-pointer batches and the caller's memory (rc_hostmem.c), against the
oracle:

- the GPU gather of a gapped compressed input over the caller's mapped,
  page-locked range (rc_gather16 over a buffer the caller page-locked) when
  the CPU rewrites that buffer between calls, and when the buffer is freed
  and a new one takes its place -- the round-5 review's candidate (b) for the
  r5a wrong decode (stale lines of mapped pages); the same batches from
  pageable memory take the pinned staging (the library never page-locks
  caller memory);
- back-to-back output slots that some packets do not fill (corrupt streams):
  the caller's bytes past each out_len stay as they were, as compress.c
  writes only what it decodes (round-5 ADVICE: the one-DMA result path);
- every input and result route, and a split batch, over memory the caller
  page-locked (enet_rc_last_host_paths).
"""
import ctypes as C

import numpy as np
import pytest

from enet_amd import synth

pytestmark = pytest.mark.gpu

P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def rc():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from enet_amd import RangeCoder
    c = RangeCoder()
    yield c
    c.close()


def _pinned(nbytes, fill=None):
    import torch
    a = torch.empty(nbytes, dtype=torch.uint8).pin_memory().numpy()
    if fill is not None:
        a[:] = fill
    return a


def _oracle_streams(d, o, l):
    from oracle.pyoracle import compress_batch
    out, oo, cap, ol = compress_batch(d, o, l, "port")
    return [out[int(oo[i]): int(oo[i]) + int(ol[i])] for i in range(len(l))]


@pytest.mark.parametrize("mem", ["pinned", "pageable"])
def test_zero_copy_input_rewritten_between_calls(rc, mem):
    n = 30000
    a = synth.mixed_batch(n, seed=0x5A31)
    b = synth.mixed_batch(n, seed=0x5A32)
    sa, sb = _oracle_streams(*a), _oracle_streams(*b)
    # gapped slots, not at a uniform pitch: the GPU gather over the mapped caller range
    cap = np.array([max(len(x), len(y)) + 16 + (i % 7) for i, (x, y) in enumerate(zip(sa, sb))], np.uint64)
    coff = np.zeros(n, np.uint64)
    coff[1:] = np.cumsum(cap[:-1])
    total = int(coff[-1] + cap[-1])

    def fill(buf, which):
        lens = np.zeros(n, np.uint32)
        for i in range(n):
            s = (sa if which[i] == 0 else sb)[i]
            buf[int(coff[i]): int(coff[i]) + len(s)] = s
            lens[i] = len(s)
        return lens

    def check(buf, lens, which):
        dout = np.zeros(int(a[2].sum()) + int(b[2].sum()) + 64, np.uint8)
        ln = np.where(which == 0, a[2], b[2]).astype(np.uint32)
        oo = np.zeros(n, np.uint64)
        oo[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
        got = np.zeros(n, np.uint32)
        assert rc.lib.enet_rc_decompress_batch_host(rc.ctx, P(buf), P(coff), P(lens), n, P(dout), P(oo), P(ln),
                                                    P(got)) == 0
        # the GPU gather over the caller's mapped range, or the pinned staging
        assert rc.lib.enet_rc_last_host_paths(rc.ctx) & 0xF == (4 if mem == "pinned" else 1)
        assert np.array_equal(got, ln), (np.nonzero(got != ln)[0][:8], rc.last_lane_count())
        bad = []
        for i in range(n):
            src = a if which[i] == 0 else b
            want = src[0][int(src[1][i]): int(src[1][i]) + int(src[2][i])]
            if not np.array_equal(dout[int(oo[i]): int(oo[i]) + int(ln[i])], want):
                bad.append(i)
        assert not bad, bad[:8]

    buf = _pinned(total, 0xEE) if mem == "pinned" else np.full(total, 0xEE, np.uint8)
    which = np.zeros(n, np.int8)
    check(buf, fill(buf, which), which)
    which = np.ones(n, np.int8)                   # every stream rewritten by the CPU in place
    check(buf, fill(buf, which), which)
    which = (np.arange(n) % 2).astype(np.int8)    # half of them back
    check(buf, fill(buf, which), which)
    del buf                                        # a new buffer, likely on the same pages
    buf = _pinned(total, 0x11) if mem == "pinned" else np.full(total, 0x11, np.uint8)
    which = np.zeros(n, np.int8)
    check(buf, fill(buf, which), which)


@pytest.mark.parametrize("mem", ["pinned", "pageable"])
def test_back_to_back_slots_keep_bytes_past_out_len(rc, mem):
    from oracle.pyoracle import compress_batch, decompress_batch
    n, size = 4000, 1200
    d, o, l = synth.random_batch(n, size, seed=0x5A33)
    out, oo, ocap, ol = compress_batch(d, o, l, "port")
    rng = np.random.default_rng(5)
    bad = rng.choice(n, n // 8, replace=False)
    for i in bad:                                   # corrupt streams: short or failed decodes
        at = int(oo[i]) + int(rng.integers(2, max(int(ol[i]) - 1, 3)))
        out[at] ^= np.uint8(1 + rng.integers(0, 255))
    want, wo, wl = decompress_batch(out, oo, ol, l)
    assert (wl != l).sum() > 0                     # some slots are not filled
    for trial in ("corrupt", "clean"):
        if trial == "clean":
            out, oo, ocap, ol = compress_batch(d, o, l, "port")
            want, wo, wl = decompress_batch(out, oo, ol, l)
        dout = _pinned(n * size + 64, 0x3C) if mem == "pinned" else np.full(n * size + 64, 0x3C, np.uint8)
        got = np.zeros(n, np.uint32)
        l32 = l.astype(np.uint32)
        assert rc.lib.enet_rc_decompress_batch_host(rc.ctx, P(out), P(oo), P(ol), n, P(dout), P(o), P(l32),
                                                    P(got)) == 0
        assert np.array_equal(got, wl)
        paths = rc.lib.enet_rc_last_host_paths(rc.ctx) >> 4
        # one DMA of the span into a page-locked buffer only when every slot is full
        assert (paths == 2) == (trial == "clean" and mem == "pinned"), paths
        for i in range(n):
            s = int(o[i])
            assert np.array_equal(dout[s: s + int(got[i])], want[int(wo[i]): int(wo[i]) + int(wl[i])]), i
            assert (dout[s + int(got[i]): s + size] == 0x3C).all(), i


@pytest.fixture(scope="module")
def route_batch():
    """32768 random 1200-B packets and their oracle streams (read-only): the
    route cases take the first 14336 (17.2 MB, just over the 16 MiB threshold
    of the gather and slot-copy routes), the split case all of them."""
    from oracle.pyoracle import compress_batch
    d, o, l = synth.random_batch(32768, 1200, seed=0x5A35)
    out, oo, cap, ol = compress_batch(d, o, l, "port")
    for a in (d, o, l, out, oo, cap, ol):
        a.setflags(write=False)
    return d, o, l, out, oo, cap, ol


def _gapped(cap, n):
    """Slots of cap[i] bytes with non-uniform gaps (0..6 bytes) between them."""
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(cap[:n - 1].astype(np.uint64) + (np.arange(n - 1, dtype=np.uint64) % np.uint64(7)))
    return off, int(off[-1]) + int(cap[n - 1]) + 16


def _slot_mismatches(buf, boff, want, woff, wlen):
    return [i for i in range(len(wlen))
            if not np.array_equal(buf[int(boff[i]): int(boff[i]) + int(wlen[i])],
                                  want[int(woff[i]): int(woff[i]) + int(wlen[i])])][:8]


@pytest.mark.parametrize("case,mem,n,layout,paths", [
    ("compress", "pinned", 14336, "packed", (2, 3)),       # one DMA of the caller's range in, GPU slot copy out
    ("compress", "pinned", 14336, "pitch", (3, 3)),        # strided DMA of slots at pitch 1216 in
    ("decompress", "pinned", 14336, "gapped", (4, 2)),     # GPU gather in, one DMA of the span out
    ("compress", "pageable", 14336, "packed", (1, 4)),     # staging in, device pack + host scatter out
    ("compress", "pinned", 64, "packed", (1, 1)),          # below the 1 MiB floor: staging in, small copy out
])
def test_host_routes(rc, route_batch, case, mem, n, layout, paths):
    """The input and result routes of a host batch (rc_hostmem.c), each asserted
    by both nibbles of enet_rc_last_host_paths and bit-exact against the oracle."""
    d, o, l, want, wo, wcap, wl = route_batch
    buf = _pinned if mem == "pinned" else (lambda nbytes, fill: np.full(nbytes, fill, np.uint8))
    ln, cl = np.ascontiguousarray(l[:n]), np.ascontiguousarray(wl[:n])
    got = np.zeros(n, np.uint32)
    if case == "compress":
        pitch = 1200 if layout == "packed" else 1216
        ioff = np.arange(n, dtype=np.uint64) * np.uint64(pitch)
        din = buf(n * pitch, 0x77)
        din.reshape(n, pitch)[:, :1200] = d[: n * 1200].reshape(n, 1200)
        cap = np.ascontiguousarray(wcap[:n])
        coff, total = _gapped(cap, n)
        cout = buf(total, 0xC3)
        assert rc.lib.enet_rc_compress_batch_host(rc.ctx, P(din), P(ioff), P(ln), n, P(cout), P(coff), P(cap),
                                                  P(got)) == 0
        p = rc.lib.enet_rc_last_host_paths(rc.ctx)
        assert (p & 0xF, p >> 4) == paths, hex(p)
        assert np.array_equal(got, cl)
        assert not _slot_mismatches(cout, coff, want, wo, cl)
    else:
        assert int(cl.sum(dtype=np.uint64)) >= 16 << 20     # else the gather route is not the one under test
        coff, total = _gapped(cl, n)
        cin = buf(total, 0xC3)
        for i in range(n):
            cin[int(coff[i]): int(coff[i]) + int(cl[i])] = want[int(wo[i]): int(wo[i]) + int(cl[i])]
        dout = buf(n * 1200 + 16, 0x3C)
        doff = np.ascontiguousarray(o[:n])
        assert rc.lib.enet_rc_decompress_batch_host(rc.ctx, P(cin), P(coff), P(cl), n, P(dout), P(doff), P(ln),
                                                    P(got)) == 0
        p = rc.lib.enet_rc_last_host_paths(rc.ctx)
        assert (p & 0xF, p >> 4) == paths, hex(p)
        assert np.array_equal(got, ln)
        assert np.array_equal(dout[: n * 1200], d[: n * 1200])


def test_host_split_over_pinned_memory(rc, route_batch):
    """A split batch (default ENET_RC_HOST_SPLIT) whose buffers the caller
    page-locked: 32768 x 1200 B compressed into gapped slots, then decompressed
    into back-to-back slots; bit-exact against the oracle both ways."""
    import os
    d, o, l, want, wo, wcap, wl = route_batch
    n = len(l)
    pieces = min(3, max(int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) - 1, 1))
    din = _pinned(d.size)
    din[:] = d
    coff, total = _gapped(wcap, n)
    cout = _pinned(total, 0xC3)
    clen = np.zeros(n, np.uint32)
    assert rc.lib.enet_rc_compress_batch_host(rc.ctx, P(din), P(o), P(l), n, P(cout), P(coff), P(wcap), P(clen)) == 0
    assert rc.lib.enet_rc_last_split(rc.ctx) == pieces
    assert np.array_equal(clen, wl)
    assert not _slot_mismatches(cout, coff, want, wo, wl)
    dout = _pinned(d.size + 16, 0x3C)
    dlen = np.zeros(n, np.uint32)
    assert rc.lib.enet_rc_decompress_batch_host(rc.ctx, P(cout), P(coff), P(clen), n, P(dout), P(o), P(l), P(dlen)) == 0
    assert rc.lib.enet_rc_last_split(rc.ctx) == pieces
    assert np.array_equal(dlen, l)
    assert np.array_equal(dout[: d.size], d)


def test_slot_handoff_many_packets_per_lane(rc):
    """The record-light decoder's input hand-off on the hardware across packet
    boundaries: 4 x 65536 short random packets, so every decoding lane takes
    several packets in turn (new generations, the helper's new-packet path,
    rc_slot.h), decoded through the device entry against the oracle; the
    hand-off's check sums (rc_dec6_verify) must never disagree
    (enet_rc_debug_counter 7 counts the packets they sent to the lane kernels)."""
    import torch
    from oracle.pyoracle import compress_batch, fnv_digest
    n = 4 * 65536
    d, o, l = synth.mixed_batch(n, lo=24, hi=300, seed=0x5A34)
    want, wo, wcap, wl = compress_batch(d, o, l, "port")
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a)).to(t).cuda()  # noqa: E731
    din, doff, dlen = dev(d, torch.uint8), dev(o, torch.int64), dev(l, torch.int32)
    cap = (2 * dlen.to(torch.int64) + 64).to(torch.int32)
    coff = torch.zeros(n, dtype=torch.int64, device="cuda")
    coff[1:] = torch.cumsum(cap[:-1].to(torch.int64), 0)
    cout = torch.zeros(int(coff[-1] + cap[-1]), dtype=torch.uint8, device="cuda")
    clen = torch.zeros(n, dtype=torch.int32, device="cuda")
    rc.compress_batch(din, doff, dlen, cout, coff, cap, clen, max_len=int(l.max()))
    torch.cuda.synchronize()
    cl = clen.cpu().numpy().astype(np.uint32)
    assert np.array_equal(cl, wl)
    assert fnv_digest(cout.cpu().numpy(), coff.cpu().numpy().astype(np.uint64), cl) == fnv_digest(want, wo, wl)
    for _ in range(3):
        dout = torch.zeros_like(din)
        dl = torch.zeros(n, dtype=torch.int32, device="cuda")
        rc.decompress_batch(cout, coff, clen, dout, doff, dlen, dl, max_len=int(cl.max()))
        torch.cuda.synchronize()
        assert torch.equal(dl, dlen) and torch.equal(dout, din)
        assert rc.lib.enet_rc_debug_counter(rc.ctx, 7) == 0          # no hand-off sum mismatch
        assert rc.last_lane_count() == 0
