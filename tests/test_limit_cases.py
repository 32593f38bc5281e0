"""The limit-case generators (tests/limit_cases.py) against the host models, on
the CPU: every packet that claims to sit on a fast-path limit, or one past
it, is round-tripped by the oracle, routed and coded by the Python model of
the two-pass encoder (tests/proto/twopass.py) and decoded by the host build
of the per-lane code (tests/proto/lane_host.cpp: the record-light decoder
with and without its LDS slot, and the lane kernels alone) -- each of which
has to keep or leave it as the case claims, bit-exactly.  A claim that does
not hold here is a wrong generator.  tests/test_gpu_limits.py then holds the
kernels to the same claims."""
import pytest

from tests import limit_cases as lc
from tests.proto import twopass
from tests.test_lane_host import lane  # noqa: F401  (the host builds v3, v6, v6s: a fixture, reused)


@pytest.fixture(scope="module")
def port():
    from oracle.pyoracle import Coder
    return Coder("port")


@pytest.fixture(scope="module")
def batches():
    return {"length": lc.length_edge_batches(), "verify": [lc.verify_batch()], "bail": lc.wave_bail_batches()}


@pytest.fixture(scope="module")
def cases(batches):
    """Every distinct packet of the generators with its claims, and the fillers."""
    out = {c.name: c for c in lc.all_packet_cases() + lc.verify_sweep()}
    for b in batches["length"]:
        (i, _), = b.in_mis.items()
        out[b.name] = lc.Case(b.name, b.packets[i], b.dec_lanes == 1, twopass.scan(b.packets[i]) is not None)
    for j, p in enumerate(lc.filler(24, 0) + lc.filler(8, 77, 1200)):
        out[f"filler/{j}"] = lc.Case(f"filler/{j}", p, False, True)
    return list(out.values())


@pytest.fixture(scope="module")
def streams(cases, port):
    """The oracle's stream of every case, computed once; the oracle round-trips each."""
    out = {}
    for c in cases:
        n = len(c.packet)
        r, s = port.compress(c.packet, 2 * n + 64)
        assert r > 0 and port.decompress(s, n) == (n, c.packet), c.name
        assert port.decompress(s, 4096 if n <= 4096 else n + 64) == (n, c.packet), c.name
        out[c.name] = (r, s)
    return out


def test_table_claims_are_the_stated_constants(cases):
    """The claims the generators state outright, by name: each side of every
    limit of the record-light decoder and of the narrow scan."""
    by = {c.name: c for c in cases}
    kept = ["o1_elements/k8", "o1_elements/k9", "o1_elements/k28", "o1_hits/h7", "o2_hits/m4",
            "reset_edges/short", "reset_edges/after_last", "reset_edges/before_last", "reset_edges/two"]
    left = ["o1_elements/k29", "o1_elements/k30", "o1_hits/h8", "o1_hits/h9", "o2_hits/m5", "o2_hits/m6",
            "reset_edges/at_4095"]
    assert [by[k].dec_leaves for k in kept] == [False] * len(kept)
    assert [by[k].dec_leaves for k in left] == [True] * len(left)
    assert [by[f"bucket_positions/k{k}"].narrow for k in (63, 64, 65)] == [True, True, False]
    # the generators' own model of the decoder's limits agrees with what they state
    assert [lc.dec6_leaves(by[k].packet) for k in kept + left] == [False] * len(kept) + [True] * len(left)
    for c in cases:
        if c.name.startswith("length_edge/"):
            assert c.dec_leaves == ("/wide_" in c.name), c.name
        if c.name.startswith(("verify_sweep/", "filler/")):
            assert not c.dec_leaves, c.name


def test_narrow_scan_reaches_the_top_of_its_reciprocal_table(cases):
    """bucket_positions/k64: the last position of bucket 0 has 63 earlier
    visits, all distinct, at order 1: total 5 * 63 + 2 * 63 = 441 = kRcpTab - 1
    (rc_enc2.hip); k63 stops one entry short."""
    by = {c.name: c for c in cases}

    def top(p):
        prim, ext = twopass.scan(p)
        tot = 0
        for h, e in zip(prim, ext):
            t, d = (h >> 3) & 63, (h >> 9) & 63
            tot = max(tot, 5 * d + 2 * t)
            if h & 7 in (4, 5):
                tot = max(tot, 5 * ((e >> 6) & 63) + 2 * (e & 63))
        return tot
    assert top(by["bucket_positions/k64"].packet) == lc.ENC2_RCP_TOP
    assert top(by["bucket_positions/k63"].packet) == lc.ENC2_RCP_TOP - 7


def test_reset_edges_reset_where_they_claim(cases):
    by = {c.name: c for c in cases}

    def resets(name):
        return [i for i, r in enumerate(twopass.scan_wide(by[name].packet, 4096)) if r[3]]
    n = len(by["reset_edges/after_last"].packet)
    assert resets("reset_edges/short") == [] and resets("reset_edges/after_last") == []
    assert resets("reset_edges/before_last") == [n - 1]
    assert len(resets("reset_edges/two")) == 2
    assert resets("reset_edges/at_4095") == []                    # (after the last byte: nothing left to code)
    segs, tail = lc._segments(by["reset_edges/at_4095"].packet)
    assert len(segs) == 1 and tail == 4096
    segs, tail = lc._segments(by["reset_edges/after_last"].packet)
    assert len(segs) == 1 and tail == n
    # the verify sweep's flat content never resets, its noise does before 2040
    for c in cases:
        if c.name.startswith("verify_sweep/flat"):
            assert not any(r[3] for r in twopass.scan_wide(c.packet, 4096)), c.name
    assert any(r[3] for r in twopass.scan_wide(by["verify_sweep/noise_n2040"].packet, 4096))


def test_long_runs_fill_the_run_list(cases):
    """long_runs: nr runs of more than kWideDense visits in one bucket, within
    wide_runs_max<L>() = L / 64 + 2 of the layout the packet's length selects."""
    by = {c.name: c for c in cases}
    for nr, r, layout in lc.LONG_RUNS:
        p = by[f"long_runs/{nr}x{r}"].packet
        runs = {}
        for i in range(2, len(p)):
            if p[i - 1] == 255:
                runs[p[i - 2]] = runs.get(p[i - 2], 0) + 1
        long_runs = sum(v > lc.WIDE_DENSE for v in runs.values())
        assert sorted(runs.values()) == [r - 1] + [r] * (nr - 1)
        assert long_runs == (nr - 1 if r > lc.WIDE_DENSE else 0)   # (runs of 32: the closed form, by one visit)
        assert layout == next(l for l in lc.ENC2_WSCAN_LAYOUTS if len(p) <= l)
        if r > lc.WIDE_DENSE:                                      # one more byte: every run is long
            p = by[f"long_runs/{nr}x{r}+1"].packet
            assert sum(p[i - 1] == 255 for i in range(2, len(p))) == nr * r
            assert nr <= layout // 66 + 1 <= layout // 64 + 2      # (the bound rc_enc2.hip proves, and the array)
            assert layout == next(l for l in lc.ENC2_WSCAN_LAYOUTS if len(p) <= l)


def test_twopass_models_route_and_code_as_claimed(cases, streams, port):
    for c in cases:
        p, n = c.packet, len(c.packet)
        narrow = twopass.scan(p)
        wide = twopass.scan_wide(p, 4096)
        assert (narrow is not None) == c.narrow, c.name
        assert (wide is not None) == (n <= 4096), c.name
        for lim in (2 * n + 64, n):
            ref = streams[c.name] if lim != n else port.compress(p, out_limit=lim)
            if narrow is not None:
                assert twopass.code(p, narrow[0], narrow[1], lim) == ref, (c.name, lim)
            if wide is not None:
                assert twopass.code_wide(p, wide, lim) == ref, (c.name, lim)


def test_encoder_route_model(cases, batches):
    """lc.enc2_route, the model of rc_enc2.hip's windows (nothing compiles the
    scans for the host): the answers that follow from the code by hand."""
    for c in cases:
        if c.name.startswith("length_edge/"):
            continue
        n = len(c.packet)
        want = "narrow" if c.narrow else "wide"
        if n > lc.ENC2_MAX_LEN and c.name.startswith(("verify_sweep/", "reset_edges/")) and c.name != "reset_edges/at_4095":
            # noise: every model segment ends within a window; flat: narrow with no reset, one segment
            want = "lanes" if c.name.startswith("verify_sweep/flat") and n > lc.ENC2_WINDOW else "narrow"
        assert lc.enc2_route(c.packet) == want, c.name
    flat = {(2033, 0): 0, (2033, 15): 0, (2034, 0): 0, (2034, 15): 1, (2048, 0): 0, (2048, 15): 1,
            (2049, 0): 1, (2049, 15): 1}
    for b in batches["length"]:
        (i, mis), = b.in_mis.items()
        n = len(b.packets[i])
        if "/flat_" in b.name:
            assert b.enc_lanes == flat[(n, mis)], b.name
        else:
            assert b.enc_lanes == (1 if n > lc.ENC2_SLOT_MAX else 0), b.name
    vb = batches["verify"][0]
    # the flat packets longer than their window (2048 - input address mod 16): one segment, no reset
    over = sum(1 for i, mis in vb.in_mis.items()
               if vb.packets[i] == lc.flat_content(len(vb.packets[i])) and len(vb.packets[i]) > lc.ENC2_WINDOW - mis)
    assert vb.enc_lanes == over >= 4 * 4 and vb.dec_lanes == 0


def test_host_lane_code_keeps_or_leaves_as_claimed(lane, cases, streams):  # noqa: F811
    for c in cases:
        p, n = c.packet, len(c.packet)
        r, s = streams[c.name]
        if lane.version == "v3":
            assert lane(0, p, 2 * n + 64, max_len=n) == (r, s), c.name
            assert lane(1, s, n, max_len=max(r, 16)) == (n, p), c.name
            continue
        for cap in (n, max(n, 4096)):
            lane.left = 0
            assert lane(1, s, cap, max_len=4096) == (n, p), (c.name, cap)
            assert lane.left == int(c.dec_leaves), (c.name, cap)


def test_verify_fast_path_edge():
    """rc_dec6_verify's pipelined path holds 512 dwords from the aligned dword
    of the first output byte: the sweep's lengths straddle it at every offset."""
    for om, last in ((0, 2048), (1, 2047), (2, 2046), (3, 2045)):
        assert lc.verify_fast(last, om) and not lc.verify_fast(last + 1, om)
        assert 2040 <= last < last + 1 <= 2052


def test_batches_hold_their_cases(batches):
    for b in lc.case_batches(lc.o1_hits()) + batches["bail"]:
        assert len(b.packets) == lc.BATCH
    on, past = lc.case_batches(lc.o1_hits())[0], lc.case_batches(lc.o1_hits())[1]
    assert (on.dec_lanes, past.dec_lanes) == (0, 6) and on.enc_lanes == past.enc_lanes == 0
    assert sorted(past.in_mis) == [0, 31, 63, 192, 223, 255]
    assert [b.dec_lanes for b in batches["bail"]] == [lc.DEC6_WAVE_BAIL - 1, 64]
    sw = lc.sweep_batches(lc.rescale_lane_sweep_o2(), "o2")
    assert sum(len(b.in_mis) for b in sw) == 64 and all(b.dec_lanes == len(b.in_mis) for b in sw)
    with pytest.raises(AssertionError):          # 16 leavers in 64 consecutive packets: refused
        lc.make_batch("x", [(i, lc.o1_hits()[1], 0, None) for i in range(40, 56)])
