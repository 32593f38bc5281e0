"""Every fast-path limit crossed from both sides, on the GPU.

The packets of tests/limit_cases.py -- each sits on a hard-coded limit of the
two-pass encoder (rc_enc2.hip), of the record-light decoder and its check
(rc_dec6.hip) or of the lane kernels' records (rc_lane3.hip), or one past it;
tests/test_limit_cases.py holds the host models to the same claims -- go
through the C ABI in batches of 256 (a workgroup of rc_decompress_dec6s),
the case at lanes 0, 31 and 63 of the batch's first and last wavefront, the
rest 200-B noise packets every fast path keeps.  Below 1024 packets nothing
reorders a batch (rc_route.hip rc_hip_lane_launch bins by length from 1024
up; rc_decompress_dec6s takes packet blockIdx.x * 256 + lane without an
order list), so a packet's lane is its index.

Per batch: compress equals the oracle (return value and bytes) at outLimit
2N + 64 and N; decompress of the oracle's streams equals the oracle at
capacity N and 4096; nothing takes the exact path; and the packets the fast
kernels hand to the lane kernels are exactly as many as the host models say
leave -- 0 for a batch on its limit, k for one with k packets past it.  The
counts come from the models (lc.dec6_leaves, lc.enc2_route), never from a
GPU run.  Bit-exact or wrong: nothing here has a tolerance.
"""
import numpy as np
import pytest

from tests import limit_cases as lc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from tests.test_gpu_parity import VARIANTS  # noqa: E402
from tests.test_gpu_wide import _coder  # noqa: E402


GROUPS = {
    # rc_dec6_rare.h kTabCap = 28 (and the 16-B -> 48-B record step at 8 / 9); rc_dec6.hip: 7 order-1 hits
    # per bucket, 4 order-2 hits
    "dec_records": lambda: lc.case_batches(lc.o1_elements() + lc.o1_hits() + lc.o2_hits()),
    # rc_enc2.hip kE2Bucket = 64 / kRcpTab's top entry 441; WScanLdsT::runs; rescales every 127 / 63 visits;
    # kWideDense = 32
    "scan_buckets": lambda: lc.case_batches(lc.bucket_positions() + lc.long_runs() + lc.one_context() +
                                            lc.dense_edge(), seed=20),
    # the dense walk's rounds: the rescaling visit at every lane, at order 2 and at order 1
    "rescale_sweep": lambda: lc.sweep_batches(lc.rescale_lane_sweep_o2(), "rescale_sweep_o2", 40) +
                             lc.sweep_batches(lc.rescale_lane_sweep_o1(), "rescale_sweep_o1", 60),
    # compress.c:148-157 at the packet's end, twice, and at byte 4095 (rc_dec6.hip can_reset6);
    # rc_lane3.hip ctx_update: 12 / 24 symbols per record
    "resets_records": lambda: lc.case_batches(lc.reset_edges() + lc.lane3_records(), seed=80),
    # rc_enc2.hip's layouts (1216, 1408, 2048, 4096) and windows (2048 - input address mod 16)
    "length_edges": lc.length_edge_batches,
    # rc_dec6_verify's pipelined path: 512 dwords from the aligned dword of the first output byte
    "verify_sweep": lambda: [lc.verify_batch()],
    # rc_dec6.hip kWaveBail6 = 16
    "wave_bail": lc.wave_bail_batches,
}
LEAVERS = ("dec_records", "wave_bail")

_cache = {}


def _batches(group):
    if group not in _cache:
        _cache[group] = GROUPS[group]()
    return _cache[group]


def _port():
    if "port" not in _cache:
        from oracle.pyoracle import Coder
        _cache["port"] = Coder("port")
    return _cache["port"]


def _oracle(p, lim):
    """The oracle's compress of p at lim, computed once per (packet, limit)."""
    key = (p, lim)
    if key not in _cache:
        _cache[key] = _port().compress(p, out_limit=lim)
    return _cache[key]


def _place(sizes, mods, modulus):
    """Offsets of back-to-back regions; region i of mods at the next offset = mods[i] (mod modulus)."""
    off, cur = np.zeros(len(sizes), np.int64), 0
    for i, s in enumerate(sizes):
        if i in mods:
            cur += (mods[i] - cur) % modulus
        off[i] = cur
        cur += s
    return off, cur


def _launch(coder, decompress, blobs, in_mods, caps, out_mods):
    """One batch call; returns [(return value, bytes)] per packet."""
    n = len(blobs)
    in_off, total = _place([len(b) for b in blobs], in_mods, 16)
    data = np.zeros(total + 16, np.uint8)
    for b, o in zip(blobs, in_off):
        data[o: o + len(b)] = np.frombuffer(b, np.uint8)
    out_off, out_total = _place(caps, out_mods, 4)
    din = torch.from_numpy(data).cuda()
    assert din.data_ptr() % 16 == 0                    # (offsets mod 16 are addresses mod 16)
    out = torch.zeros(out_total + 16, dtype=torch.uint8, device="cuda")
    out_len = torch.zeros(n, dtype=torch.int32, device="cuda")
    args = (din, torch.from_numpy(in_off).cuda(), torch.tensor([len(b) for b in blobs], dtype=torch.int32).cuda(),
            out, torch.from_numpy(out_off).cuda(), torch.tensor(caps, dtype=torch.int32).cuda(), out_len)
    ml = max(len(b) for b in blobs)
    if decompress:
        coder.decompress_batch(*args, max_len=ml)
    else:
        coder.compress_batch(*args, max_len=ml)
    torch.cuda.synchronize()
    ol = out_len.cpu().numpy().astype(np.int64)
    ob = out.cpu().numpy()
    return [(int(ol[i]), ob[out_off[i]: out_off[i] + ol[i]].tobytes()) for i in range(n)]


def _same(got, want, what):
    bad = [(i, g[0], w[0]) for i, (g, w) in enumerate(zip(got, want)) if g[0] != w[0] or (w[0] and g[1] != w[1])]
    assert not bad, (what, bad[:8])


def _check(coder, b, routed, compress=True, decompress=True):
    """routed: the fast kernels are on -- their hand-over counts are asserted."""
    n = len(b.packets)
    if compress:
        for lim in (lambda k: 2 * k + 64, lambda k: k):
            want = [_oracle(p, lim(len(p))) for p in b.packets]
            got = _launch(coder, False, b.packets, b.in_mis, [lim(len(p)) for p in b.packets], {})
            _same(got, want, (b.name, "compress", lim(100)))
            assert coder.last_exact_count() == 0, b.name
            if routed:
                assert coder.last_lane_count() == b.enc_lanes, (b.name, "packets the encoder left")
    if decompress:
        streams = [_oracle(p, 2 * len(p) + 64)[1] for p in b.packets]
        for cap in (lambda k: k, lambda k: 4096):
            caps = [cap(len(p)) for p in b.packets]
            want = [(len(p), p) if c >= len(p) else _port().decompress(s, c) for p, s, c in zip(b.packets, streams, caps)]
            got = _launch(coder, True, streams, {}, caps, b.out_mod)
            _same(got, want, (b.name, "decompress", cap(100)))
            assert coder.last_exact_count() == 0, b.name
            if routed:
                assert coder.last_lane_count() == b.dec_lanes, (b.name, "packets the decoder left")
    assert n % lc.BATCH == 0 and n < 1024


@pytest.fixture(scope="module")
def fast():
    c = _coder()
    yield c
    c.close()


@pytest.fixture(scope="module")
def slow():
    c = _coder(ENET_RC_ENC2_SLOW="1")
    yield c
    c.close()


@pytest.fixture(scope="module")
def lanes_only():
    # tests/test_gpu_parity.py's lane3-only: no two-pass encoder, no fast decoder (rc_host.c reads
    # ENET_RC_DEC=0 and, as here, its older name ENET_RC_DEC4=0)
    c = _coder(**VARIANTS["lane3-only"])
    yield c
    c.close()


@pytest.fixture(scope="module")
def small():
    # the default routing of small batches (no ENET_RC_SMALL_BATCH): the fast kernels, then the wave
    # kernel on what the decoder leaves (rc_kernels.hip small_route)
    import os
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from enet_amd import RangeCoder
    old = {k: os.environ.pop(k, None) for k in ("ENET_RC_KERNEL", "ENET_RC_SMALL_BATCH")}
    os.environ["ENET_RC_KERNEL"] = "lane3"
    try:
        c = RangeCoder()
    finally:
        os.environ.pop("ENET_RC_KERNEL", None)
        os.environ.update({k: v for k, v in old.items() if v is not None})
    yield c
    c.close()


@pytest.mark.parametrize("group", list(GROUPS))
def test_limits_routed_and_exact(fast, group):
    for b in _batches(group):
        _check(fast, b, routed=True)


@pytest.mark.parametrize("group", list(GROUPS))
def test_limits_scan_slow_paths(slow, group):
    """ENET_RC_ENC2_SLOW=1: the scans without the lane-order shortcut."""
    for b in _batches(group):
        _check(slow, b, routed=True, decompress=False)


@pytest.mark.parametrize("group", list(GROUPS))
def test_limits_lane_kernels_alone(lanes_only, group):
    for b in _batches(group):
        _check(lanes_only, b, routed=False)


@pytest.mark.parametrize("group", LEAVERS)
def test_leavers_default_small_batch_routing(small, group):
    """The wave kernel takes what rc_decompress_dec6s leaves."""
    for b in _batches(group):
        _check(small, b, routed=True)
