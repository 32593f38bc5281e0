"""The kernels around the range coder at their edges (tests/aux_cases.py):
rc_pack.hip's copies and scans, rc_crc32.hip, rc_dgram.hip through the
device entries, and rc_multi_plan.hip on exact ties.

Each kernel is called directly through the C ABI -- the public entries, and
the launchers rc_hip_slot_copy, rc_hip_gather16 and rc_hip_unpack that the
library exports -- on buffers filled with a canary, and compared byte for
byte with a plain reference: numpy slicing, zlib, the oracle's framing,
shard_ranges.  Every comparison is exact.  Every offset and length stays
inside its buffer, the 16-byte granule reads of rc_crc32.hip and rc_gather16
included (tests/test_aux_cases.py checks the padding).
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from tests import aux_cases as ac

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def coder():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from enet_amd import RangeCoder
    c = RangeCoder()
    yield c
    c.close()


@pytest.fixture(scope="module")
def launch(coder):
    """The internal launchers of rc_pack.hip (plain extern "C" symbols of the library)."""
    lib = coder.lib
    vp, u32 = C.c_void_p, C.c_uint32
    # int rc_hip_slot_copy(src, off, len, n, dst, max_wgs, stream)
    lib.rc_hip_slot_copy.restype = C.c_int
    lib.rc_hip_slot_copy.argtypes = [vp, vp, vp, u32, vp, u32, vp]
    # int rc_hip_gather16(src, soff, dst, doff, len, n, stream)
    lib.rc_hip_gather16.restype = C.c_int
    lib.rc_hip_gather16.argtypes = [vp, vp, vp, vp, vp, u32, vp]
    # int rc_hip_unpack(packed, out, out_off, out_len, n, bsum, stream)
    lib.rc_hip_unpack.restype = C.c_int
    lib.rc_hip_unpack.argtypes = [vp, vp, vp, vp, u32, vp, vp]
    return lib


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a if dtype is None else a.astype(dtype))).cuda()


def _dev_bytes(a, shift=0, align=256):
    """a on the device at an address = shift (mod align): a view into a
    buffer a little larger (allocations are 256-B aligned)."""
    buf = torch.empty(len(a) + shift, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % align == 0
    view = buf[shift:]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.data_ptr() % align == shift and view.is_contiguous()
    return view


def _host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


# -------------------------------------------------------------------- slot_copy

@pytest.mark.parametrize("max_wgs", [0, 1, 3])
def test_slot_copy_every_alignment(launch, max_wgs):
    """rc_slot_copy over the copy layout (308 packets; every head, tail and
    shift of copy_bytes, its byte-only branch, empty packets, 63..67 whole
    dwords) at all 4 x 4 alignments of the two buffers.  max_wgs 1 and 3: 4
    and 12 wavefronts take the packets in turn (77 and 26 each) -- the
    grid-stride loop; 0: the launcher's own cap, one wavefront per packet."""
    lay = ac.copy_layout()
    off, ln = _dev(lay.off, np.int64), _dev(lay.ln, np.int32)
    blank = np.full(len(lay.src), ac.DST_CANARY, np.uint8)
    for sb, db in itertools.product(range(4), range(4)):
        src, dst = _dev_bytes(lay.src, sb), _dev_bytes(blank, db)
        rc = launch.rc_hip_slot_copy(src.data_ptr(), off.data_ptr(), ln.data_ptr(), len(lay.ln), dst.data_ptr(),
                                     max_wgs, _stream())
        assert rc == 0
        got = _host(dst)
        bad = np.flatnonzero(got != lay.want)
        assert bad.size == 0, (sb, db, max_wgs, bad[:8], _where(lay, bad[0]))
        assert np.array_equal(_host(src), lay.src)


def _where(lay, pos):
    """(packet, its offset and length) around byte pos of a layout, for a failure message."""
    i = int(np.searchsorted(lay.off, pos, side="right")) - 1
    return i, int(lay.off[max(i, 0)]), int(lay.ln[max(i, 0)])


# ---------------------------------------------------------------- pack / unpack

def _pack_unpack(coder, launch, lay, packed_want):
    n, total = len(lay.ln), len(packed_want)
    off, ln = _dev(lay.off, np.int64), _dev(lay.ln, np.int32)
    src = _dev_bytes(lay.src)
    pbuf = _dev_bytes(np.full(total + 2 * ac.PAD, ac.DST_CANARY, np.uint8))
    coder.pack_batch(src, off, ln, pbuf[ac.PAD:])
    got = _host(pbuf)
    assert np.array_equal(got[ac.PAD: ac.PAD + total], packed_want)           # the numpy concatenation
    assert np.all(got[:ac.PAD] == ac.DST_CANARY) and np.all(got[ac.PAD + total:] == ac.DST_CANARY)
    # back into a second canaried slot buffer, with a bsum of the test's own
    nb = (n + 1023) // 1024
    bsum = torch.full((nb + 1,), -1, dtype=torch.int64, device="cuda")
    dst = _dev_bytes(np.full(len(lay.src), ac.DST_CANARY, np.uint8))
    rc = launch.rc_hip_unpack(pbuf[ac.PAD:].data_ptr(), dst.data_ptr(), off.data_ptr(), ln.data_ptr(), n,
                              bsum.data_ptr(), _stream())
    assert rc == 0
    back = _host(dst)
    bad = np.flatnonzero(back != lay.want)
    assert bad.size == 0, (n, bad[:8], _where(lay, bad[0]))
    sums = _host(bsum).view(np.uint64)
    assert int(sums[nb]) == total                                              # the packed total
    assert np.array_equal(sums, ac.segment_sums(lay.ln))
    assert np.array_equal(_host(pbuf), got) and np.array_equal(_host(src), lay.src)


@pytest.mark.parametrize("n", ac.PACK_SIZES)
def test_pack_unpack_small(coder, launch, n):
    """enet_rc_pack_batch_device, then rc_hip_unpack: around the 64-packet
    workgroup and the 1024-packet segment, the copy layout's lengths cycled."""
    _pack_unpack(coder, launch, *ac.pack_case(n))


def test_pack_unpack_carry_across_256_segments(coder, launch):
    """n = 262144 + 1024 + 5 packets of 0..7 bytes (~0.9 MB): 258 segments, so
    rc_pack_scan's loop runs twice and the second pass adds the carry."""
    n = ac.PACK_CARRY_N
    assert (n + 1023) // 1024 > 256
    _pack_unpack(coder, launch, *ac.pack_case(n, (np.arange(n) % 8).astype(np.uint32)))


# --------------------------------------------------------------------- gather16

def _gather(launch, ln, shift):
    g = ac.gather_case(ln, shift)
    src = _dev_bytes(g.src, shift, align=16)
    dst = _dev_bytes(np.full(g.dst_bytes, ac.DST_CANARY, np.uint8), 0, align=16)
    soff, doff, dl = _dev(g.soff, np.int64), _dev(g.doff, np.int64), _dev(g.ln, np.int32)
    rc = launch.rc_hip_gather16(src.data_ptr(), soff.data_ptr(), dst.data_ptr(), doff.data_ptr(), dl.data_ptr(),
                                len(g.ln), _stream())
    assert rc == 0
    got = _host(dst)
    s, _ = ac.packet_bytes_index(g.soff, g.ln)
    d, _ = ac.packet_bytes_index(g.doff, g.ln)
    bad = np.flatnonzero(got[d] != g.src[s])
    assert bad.size == 0, (len(ln), shift, bad[:8])
    # no granule but those of the non-empty packets changed
    assert np.all(got[~ac.gather_owned(g)] == ac.DST_CANARY)
    # each packet's first granule keeps the source's phase: whole granules were copied
    live = g.ln > 0
    assert np.array_equal((g.doff[live] & np.uint64(15)), ((g.soff[live] + np.uint64(shift)) & np.uint64(15)))


@pytest.mark.parametrize("shift", [0, 5])
def test_gather16_grid_stride(launch, shift):
    """n = 128 CUs + 1000 packets of 0..40 bytes: more than the launcher's cap
    of 8 CUs workgroups x 16 packets, so its loop is re-entered (a workgroup's
    second packets are those past 128 CUs)."""
    cus = _cus()
    n = 128 * cus + 1000
    assert n > 8 * cus * 16
    _gather(launch, (np.arange(n) % 41).astype(np.uint32), shift)


@pytest.mark.parametrize("shift", [0, 5])
def test_gather16_copy_lengths(launch, shift):
    _gather(launch, ac.copy_lengths(100), shift)


# -------------------------------------------------------------------------- CRC

def _crc(coder, b):
    data = _dev_bytes(b.data, 0, align=16)                  # the cases' start residues are address residues
    got = coder.crc32_batch(data, _dev(b.off, np.int64), _dev(b.ln, np.int32))
    return _host(got).view(np.uint32)


def test_crc_case_list(coder):
    """Every length 0..530 and around 1024, 4096 at all 16 start residues;
    8192, 65536 and 2^20 + 5 at four -- against zlib."""
    b = ac.crc_batch()
    got = _crc(coder, b)
    bad = np.flatnonzero(got != b.want)
    assert bad.size == 0, [(int(b.off[i]) & 15, int(b.ln[i]), hex(got[i]), hex(b.want[i])) for i in bad[:8]]


def test_crc_persistent_restart(coder):
    """n = 512 CUs + 3000 packets: more than the launcher's 2 CUs workgroups x
    256 packets, so every group of four lanes takes a second packet (and
    re-initialises rr, acc, start, end, rounds and mis)."""
    cus = _cus()
    n = 512 * cus + 3000
    assert n > 2 * cus * 256 + 256
    b = ac.crc_restart_batch(n)
    got = _crc(coder, b)
    bad = np.flatnonzero(got != b.want)
    assert bad.size == 0, (bad.size, [(int(i), int(b.ln[i]), hex(got[i]), hex(b.want[i])) for i in bad[:8]])


# -------------------------------------------------------------------- datagrams

def _run_dgrams(coder, decode, cases, aligned, step):
    """One batch through the device entry: inputs in slots of exactly their
    length, outputs in slots of in_len (encode) or 4096 bytes (decode), canary
    between and after the slots on both sides."""
    ck = cases[0].checksum
    assert all(c.checksum == ck for c in cases)
    n = len(cases)
    in_len = np.array([len(c.data) for c in cases], np.uint32)
    in_off, in_total = ac.datagram_slots(in_len, aligned, step)
    out_size = np.full(n, 4096, np.uint32) if decode else in_len
    out_off, out_total = ac.datagram_slots(out_size, aligned, step + 2)
    if aligned:
        assert not (in_off % 16).any() and not (out_off % 16).any()
    blob = np.full(in_total, ac.SRC_CANARY, np.uint8)
    for c, o in zip(cases, in_off):
        blob[int(o): int(o) + len(c.data)] = np.frombuffer(c.data, np.uint8)
    din = _dev_bytes(blob, 0, align=16)
    dout = _dev_bytes(np.full(out_total, ac.DST_CANARY, np.uint8), 0, align=16)
    out_len = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    seed = _dev(np.array([c.seed for c in cases], np.uint32).view(np.int32))
    fn = coder.datagram_decode_batch if decode else coder.datagram_encode_batch
    fn(din, _dev(in_off, np.int64), _dev(in_len, np.int32), dout, _dev(out_off, np.int64), out_len,
       checksum=ck, seed=seed)
    got, gl = _host(dout), _host(out_len)
    outside = np.ones(out_total, bool)
    for i, c in enumerate(cases):
        o = int(out_off[i])
        assert int(gl[i]) == len(c.want), (c.name, int(gl[i]), len(c.want))
        assert got[o: o + len(c.want)].tobytes() == c.want, c.name
        outside[o: o + int(out_size[i])] = False
    assert np.all(got[outside] == ac.DST_CANARY)
    assert np.array_equal(_host(din), blob)


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("decode", [False, True])
def test_datagrams_device_entries(coder, decode, aligned):
    """enet_rc_datagram_{encode,decode}_batch_device against the oracle's
    framing: every header size, the 4096-byte limits from both sides, each
    side of protocol.c:1696, corrupt wires; 16-byte-aligned slots (wave_copy's
    vector path and its tail) and slots at every residue (its byte path).  A
    second, smaller batch of other content on the same context follows each:
    nothing left in the workspace may help it."""
    cases = ac.datagram_decode_cases() if decode else ac.datagram_encode_cases()
    for ck in (False, True):
        sel = [c for c in cases if c.checksum == ck]
        assert len(sel) >= 40
        _run_dgrams(coder, decode, sel, aligned, 5)
        _run_dgrams(coder, decode, sel[::-3], aligned, 7)


# -------------------------------------------------------------------- plan ties

@pytest.mark.parametrize("case", ac.plan_tie_cases(), ids=lambda c: c.name)
def test_plan_device_on_exact_ties(coder, case):
    """rc_plan_first's `<` / `>=` pair where the prefix sum meets k / parts of
    the total exactly: the device plan, the host plan and numpy agree."""
    from enet_amd import multi_plan
    c = case
    want = ac.plan_reference(c)
    assert [int(x) for x in multi_plan(c.ln, c.ioff, c.ooff, c.cap, c.parts)] == want
    dev = [_dev(a, t) for a, t in ((c.ln, np.int32), (c.ioff, np.int64), (c.ooff, np.int64), (c.cap, np.int32))]
    # first a plan whose split points all lie elsewhere (every byte in packet
    # 0), so that a split point the kernel failed to write cannot be right by
    # being left over in reused memory
    other = np.zeros_like(c.ln)
    other[0] = 1000
    got = multi_plan(_dev(other, np.int32), *dev[1:], c.parts, device=True)
    assert [int(x) for x in got[:c.parts + 1]] == [0] + [1] * (c.parts - 1) + [len(c.ln)]
    got = multi_plan(*dev, c.parts, device=True)
    assert [int(x) for x in got] == want, c.name
