"""The case builders of tests/aux_cases.py against their own claims, on the CPU:
every branch of copy_bytes, every alignment pair of the CRC kernel, each side
of protocol.c:1696 and of the 4096-byte limits, and every tie of the split
have to be in the cases before tests/test_gpu_aux_kernels.py can claim to
have run them.  A claim that does not hold here is a wrong builder.  No case
is skipped and every comparison is exact."""
import itertools
import zlib

import numpy as np
import pytest

from enet_amd import multi_plan
from tests import aux_cases as ac


def test_payload_never_equals_a_canary():
    v = ac.payload(np.random.default_rng(1), 1 << 16)
    assert len(np.unique(v)) == 254 and ac.SRC_CANARY not in v and ac.DST_CANARY not in v


def test_copy_branch_model_by_hand():
    assert ac.copy_branch(0, 0, 0) == "empty"
    assert ac.copy_branch(0, 1, 6) == "bytes_only"          # 1..7 holds no whole dword
    assert ac.copy_branch(0, 0, 3) == "bytes_only"
    assert ac.copy_branch(0, 0, 4) == (0, 0, 0, 1)
    assert ac.copy_branch(0, 1, 7) == (3, 0, 3, 1)
    assert ac.copy_branch(2, 3, 262) == (1, 1, 3, 65)
    # by brute force: head + 4 nw + tail = m, and the branch is bytes_only iff no aligned dword fits
    for s, d, m in itertools.product(range(4), range(4), range(1, 300)):
        b = ac.copy_branch(s, d, m)
        fits = any(a % 4 == 0 and a >= d and a + 4 <= d + m for a in range(d, d + m))
        assert (b != "bytes_only") == fits
        if fits:
            head, tail, sh, nw = b
            assert head + 4 * nw + tail == m and (d + head) % 4 == 0 and sh == (s + head) % 4


def _all_classes(branches):
    triples = {b[:3] for b in branches if isinstance(b, tuple)}
    nws = {b[3] for b in branches if isinstance(b, tuple)}
    return triples, nws, {b for b in branches if isinstance(b, str)}


def test_copy_layout_reaches_every_branch():
    lay = ac.copy_layout()
    assert sorted(set(int(x) for x in lay.ln)) == sorted(ac.COPY_LENGTHS)
    ends = lay.off + lay.ln
    gap = lay.off[1:].astype(np.int64) - ends[:-1].astype(np.int64)
    assert set(int(g) for g in gap) == set(range(ac.COPY_GAPS))
    # the slot addresses cover every residue mod 4; with the 0..3-byte shifts of
    # the buffers every length meets every residue
    assert {int(o) & 3 for o in lay.off} == set(range(4))
    # rc_slot_copy over the 4 x 4 buffer alignments the GPU test uses
    branches = []
    for sb, db in itertools.product(range(4), range(4)):
        branches += ac.copy_branches(lay.off, lay.ln, sb, db)
    triples, nws, names = _all_classes(branches)
    assert triples == set(itertools.product(range(4), repeat=3))
    assert {1, 63, 64, 65} <= nws
    assert names == {"empty", "bytes_only"}
    # one alignment alone already has every head and tail, and both other classes
    triples, nws, names = _all_classes(ac.copy_branches(lay.off, lay.ln))
    assert {t[:2] for t in triples} == set(itertools.product(range(4), repeat=2))
    assert {1, 63, 64, 65} <= nws and names == {"empty", "bytes_only"}
    # the reference image: packets by slicing, canary elsewhere
    inside = np.zeros(len(lay.src), bool)
    for o, l in zip(lay.off, lay.ln):
        inside[int(o): int(o) + int(l)] = True
    assert np.all(lay.src[~inside] == ac.SRC_CANARY) and np.all(lay.want[~inside] == ac.DST_CANARY)
    assert np.array_equal(lay.want[inside], lay.src[inside])
    assert not inside[:ac.PAD].any() and not inside[-ac.PAD:].any()


def test_pack_cases_reach_every_branch_in_both_directions():
    """pack: slot -> packed address (the running sum); unpack: the reverse.
    The largest of the small cases has every (head, tail, sh) both ways."""
    lay, packed = ac.pack_case(max(ac.PACK_SIZES))
    ln64 = lay.ln.astype(np.int64)
    poff = np.cumsum(ln64) - ln64
    assert np.array_equal(packed, np.concatenate([lay.src[int(o): int(o) + int(l)] for o, l in zip(lay.off, lay.ln)]))
    for branches in (ac.copy_branches(lay.off, lay.ln, dst_off=poff),            # pack
                     ac.copy_branches(poff, lay.ln, dst_off=lay.off)):           # unpack
        triples, nws, names = _all_classes(branches)
        assert triples == set(itertools.product(range(4), repeat=3))
        assert {1, 63, 64, 65} <= nws and names == {"empty", "bytes_only"}
    # the carry case: more than 256 segments, every length 0..7, offsets by hand for the first few
    ln = (np.arange(ac.PACK_CARRY_N) % 8).astype(np.uint32)
    lay, packed = ac.pack_case(ac.PACK_CARRY_N, ln)
    sums = ac.segment_sums(ln)
    assert len(sums) == 258 + 1 and int(sums[-1]) == int(ln.sum()) == len(packed)
    assert [int(x) for x in sums[:3]] == [0, 128 * 28, 256 * 28] and int(sums[257]) == 257 * 128 * 28
    assert [int(x) for x in lay.off[:4]] == [ac.PAD, ac.PAD + 1, ac.PAD + 4, ac.PAD + 9]
    assert int(lay.off[-1]) + int(lay.ln[-1]) + ac.PAD == len(lay.src)


def test_gather_case_restates_fill_dev_offsets():
    for align in (0, 5):
        g = ac.gather_case(np.array([0, 1, 15, 16, 17, 0, 40, 33], np.uint32), align)
        acc = 0
        for so, do, l in zip(g.soff, g.doff, g.ln):         # the C loop, as written
            ph = (align + int(so)) & 15
            assert int(do) == (acc + ph if l else acc)
            if l:
                acc += (ph + int(l) + 15) & ~15
            assert l or int(so) == 0
        assert g.dst_bytes == acc + 16
        own = ac.gather_owned(g)
        assert own.sum() == acc and not own[-16:].any()
    g = ac.gather_case(ac.copy_lengths(100))
    assert {(int(g.soff[i]) & 15) for i in range(100) if g.ln[i]} == set(range(16))
    # granule reads stay inside the source: 16 B of padding at both ends
    live = g.ln > 0
    assert (g.soff[live] >= 16).all() and ((g.soff[live] + g.ln[live] + 15) // 16 * 16 <= len(g.src)).all()


def test_crc_cases_reach_every_alignment_pair():
    cases = ac.crc_case_list()
    assert len(cases) == 16 * len(ac.CRC_SHORT) + 4 * len(ac.CRC_LONG)
    assert cases != sorted(cases)
    lens = {l for _, l in cases}
    assert set(range(0, 531)) | set(range(1020, 1031)) | set(range(4090, 4101)) | \
        {8191, 8192, 8193, 65535, 65536, 65537, (1 << 20) + 5} == lens
    b = ac.crc_batch()
    assert [(int(o) & 15, int(l)) for o, l in zip(b.off, b.ln)] == cases
    assert {(int(o) & 15, int(o + l) & 15) for o, l in zip(b.off, b.ln) if l >= 4} == \
        set(itertools.product(range(16), repeat=2))
    assert {(int(o) & 15, int(l)) for o, l in zip(b.off, b.ln) if l < 4} == set(itertools.product(range(16), range(4)))
    # no overlap, 16 B of padding at both ends, a few tens of MB at the most
    ends = b.off + b.ln
    assert (b.off[1:] >= ends[:-1]).all() and int(b.off[0]) >= 16
    assert ((int(ends[-1]) + 15) & ~15) + 16 <= len(b.data) < 32 << 20
    # sixteen consecutive packets (one wavefront) finish in different rounds
    rounds = (b.ln.astype(np.int64) + 255) // 256
    assert np.mean([len(set(rounds[i: i + 16])) > 1 for i in range(0, len(rounds) - 16, 16)]) > 0.5
    assert int(b.want[0]) == ac.net(zlib.crc32(b.data[int(b.off[0]): int(ends[0])].tobytes()))
    assert ac.net(0xCBF43926) == 0x2639F4CB
    from oracle.pyoracle import crc32_batch
    assert np.array_equal(crc32_batch(b.data, b.off, b.ln, "port"), b.want)


def test_crc_restart_batch_is_ragged_and_padded():
    b = ac.crc_restart_batch(5000)
    assert set(range(601)) == set(int(x) for x in b.ln)
    assert {int(o) & 15 for o in b.off} == set(range(16))
    assert int(b.off[-1] + b.ln[-1]) + 16 <= len(b.data)


def test_edge_payloads_sit_on_each_side_of_the_decision():
    from oracle.pyoracle import Coder
    port = Coder("port")
    for cls, pays in ac.edge_payloads().items():
        assert len(pays) == ac.PER_CLASS
        for cmds in pays:
            L = len(cmds)
            c, _ = port.compress(cmds, out_limit=L, in_limit=L)
            r, s = port.compress(cmds, out_limit=L + 1, in_limit=L)
            assert port.decompress(s, L) == (L, cmds) if r else True
            if cls == "c==L-1":
                assert c == L - 1
            elif cls == "c==L":
                assert c == L == r
            elif cls == "c==0,needs L+1":
                assert c == 0 and r == L + 1
            else:
                assert c == 0 and r == 0 and L >= 64


@pytest.mark.parametrize("hs", ac.HEADER_SIZES)
def test_datagram_cases_sit_where_planned(hs):
    enc = [c for c in ac.datagram_encode_cases() if c.hs == hs]
    ck = hs in (6, 8)
    assert all(c.checksum == ck and (c.data[0] & 0x80 != 0) == (hs in (4, 8)) for c in enc if c.data)
    assert {len(c.data) for c in enc} >= {0, 1, hs - 1, hs, hs + 1, 4095, 4096, 4097}
    by = {c.name.split("/", 1)[1]: c for c in enc}
    for total in (0, 1, hs - 1, 4097):
        assert by[f"len{total}"].want == b""
    assert by[f"len{hs}"].want[:hs - (4 if ck else 0)] == by[f"len{hs}"].data[:hs - (4 if ck else 0)]
    assert len(by["len4096/noise"].want) == 4096 and not by["len4096/noise"].want[0] & 0x40
    assert len(by["len4096/three"].want) < 1200 and by["len4096/three"].want[0] & 0x40
    # all four classes of the c against L decision, with what protocol.c:1696 makes of them
    for cls in ac.C_CLASSES:
        for j in range(ac.PER_CLASS):
            c = by[f"{cls}/{j}"]
            L = len(c.data) - hs
            if cls == "c==L-1":
                assert len(c.want) == hs + L - 1 and c.want[0] & 0x40
            else:
                assert len(c.want) == hs + L and not c.want[0] & 0x40 and c.want[hs:] == c.data[hs:]
    for c in enc:
        if c.cls == "compressed_bit_in":
            assert c.data[0] & 0x40
            clean = bytes([c.data[0] & ~0x40]) + c.data[1:]
            from oracle.pyoracle import Coder, datagram_encode
            assert c.want == datagram_encode(clean, ck, c.seed, Coder("port")) and c.want
    assert any(c.cls == "compressed_bit_in" and not c.want[0] & 0x40 for c in enc)     # in, and cleared on the way out

    dec = [c for c in ac.datagram_decode_cases() if c.hs == hs]
    by = {c.name.split("/", 1)[1]: c for c in dec}
    # the two wires at the 4096 edge: commands of exactly 4096 - hs bytes are taken, one more is dropped
    fit, over = by["decodes_to_mtu"], by["decodes_to_mtu+1"]
    assert fit.data[0] & 0x40 and over.data[0] & 0x40 and len(fit.data) < 1200 and len(over.data) < 1200
    assert len(fit.want) == 4096 and over.want == b""
    from oracle.pyoracle import Coder
    port = Coder("port")
    assert port.decompress(over.data[hs:], 4096 - hs + 1)[0] == 4096 - hs + 1       # dropped for its size alone
    assert port.decompress(over.data[hs:], 4096 - hs)[0] == 0
    assert by["plain_4097"].want == b"" and len(by["plain_4097"].data) == 4097
    # every valid wire decodes to what was assembled (checksum field = seed)
    valid = [c for c in dec if c.cls == "valid"]
    assert len(valid) >= 4 * ac.PER_CLASS + 6 and all(c.want for c in valid)
    assert any(c.data[0] & 0x40 for c in valid) and any(not c.data[0] & 0x40 for c in valid)
    assert {len(c.data) for c in valid} >= {hs, hs + 1, 4095, 4096}
    if ck:
        assert by["wrong_seed"].want == b"" and by["wrong_seed_plain"].want == b""
        assert by["checksum_bit/compressed"].want == b"" and by["checksum_bit/plain"].want == b""
        assert by["stream_bit/short"].want == b"" and by["stream_bit/long"].want == b""
    else:
        assert by["wrong_seed"].want and by["wrong_seed_plain"].want           # no checksum: the seed is not looked at
    assert {"stream_bit/short", "stream_bit/long"} <= set(by)


def test_datagram_slots_layouts():
    sizes = [0, 1, 16, 17, 4096, 5, 4097]
    off, total = ac.datagram_slots(sizes, aligned=True)
    assert all(int(o) % 16 == 0 for o in off)
    off2, total2 = ac.datagram_slots(list(range(40)), aligned=False)
    assert {int(o) & 15 for o in off2} == set(range(16))
    for o, s, t in ((off, sizes, total), (off2, list(range(40)), total2)):
        ends = o + np.array(s, np.uint64)
        assert (o[1:] >= ends[:-1]).all() and int(o[0]) >= ac.PAD and int(ends[-1]) + ac.PAD == t
    assert (off[1:] >= (off + np.array(sizes, np.uint64))[:-1] + 16).all()


def test_plan_tie_cases_are_ties_and_the_host_plan_agrees():
    cases = ac.plan_tie_cases()
    by = {c.name: c for c in cases}
    for parts in (2, 3, 4, 8, 64):
        c = by[f"n4096/p{parts}"]
        want_ties = sum(1 for k in range(1, parts) if (4096 * k) % parts == 0)
        assert c.ties == want_ties and (parts == 3 or c.ties == parts - 1)
    assert by["n2048/p2"].ties == 1 and by["n2051/p2/zeros"].ties == 1 and by["n64/p64"].ties == 63
    assert ac.plan_reference(by["n2048/p2"])[:3] == [0, 1024, 2048]             # packet 1023: a segment's last
    assert ac.plan_reference(by["n2051/p2/zeros"])[:3] == [0, 1020, 2051]       # the tie, then the empty packets
    assert ac.plan_reference(by["n64/p64"])[:65] == list(range(65))
    assert {f"n4096/p{p}/zeros" for p in (2, 3, 4, 8, 64)} | {"n2048/p2/zeros"} <= set(by)
    for c in cases:
        assert (c.ln[1020:1031] == 0).all() == c.name.endswith("/zeros") or len(c.ln) < 1031
        got = [int(x) for x in multi_plan(c.ln, c.ioff, c.ooff, c.cap, c.parts)]
        assert got == ac.plan_reference(c), c.name
