"""bench.py's plain run, --full and --dump-outputs.

CPU: a plain run switches every side measurement off and --full leaves them
on; dump_outputs on host tensors writes the packets' own bytes (never the
unwritten room between output slots), every byte counts in the sums, and the
arrays are float32 / float64 within the size limit.  GPU: one small plain run
with --dump-outputs, its arrays checked against the oracle's compression of
the same seeded batch."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from enet_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEGS = ("no_cpu", "no_pcie", "no_crc", "no_rccl", "no_dgram", "no_configs", "no_multi")
NAMES = {"packets", "compressed_len", "decompressed_len", "compressed_sum", "decompressed_sum",
         "sample_packets", "compressed_sample", "decompressed_sample"}


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_has_no_side_measurements(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert all(getattr(a, k) for k in LEGS) and not a.full and a.dump_outputs is None and a.steps == 7


def test_full_keeps_the_side_measurements(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and not any(getattr(a, k) for k in LEGS)
    a = _parse(monkeypatch, "--full", "--no-cpu", "--dump-outputs", "x")
    assert a.no_cpu and not a.no_crc and a.dump_outputs == "x"


def _weighted(b):
    return float((b.astype(np.int64) * (np.arange(b.size) + 1)).sum())


def _load(path):
    assert {f[:-4] for f in os.listdir(path)} == NAMES
    out = {k: np.load(os.path.join(path, k + ".npy")) for k in NAMES}
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    assert sum(a.nbytes for a in out.values()) <= 64e6
    return out


def test_dump_outputs_on_host_tensors(tmp_path, monkeypatch):
    torch = pytest.importorskip("torch")
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 100000)     # a byte sample smaller than this small batch
    n = 700
    d, o, l = synth.mixed_batch(n)
    o = o.astype(np.int64)
    rng = np.random.default_rng(1)
    cap = 2 * l.astype(np.int64) + 64
    coff = np.zeros(n, np.int64)
    coff[1:] = np.cumsum(cap[:-1])
    clen = rng.integers(0, cap + 1).astype(np.int32)     # any lengths within the slots, empty and full ones too
    clen[:2] = (0, cap[1])
    written = np.zeros(int(cap.sum()), bool)
    for i in range(n):
        written[coff[i]: coff[i] + clen[i]] = True
    cout = rng.integers(0, 256, written.size).astype(np.uint8)

    def dump(name, cout, dl=l):
        t = torch.from_numpy
        bench.dump_outputs(str(tmp_path / name), dict(
            cout=t(cout), coff=t(coff), clen=t(clen), dout=t(d), doff=t(o), dl=t(dl.astype(np.int32)),
            dlen=t(l.astype(np.int32))))
        return _load(str(tmp_path / name))

    a = dump("a", cout)
    pk, sp = a["packets"].astype(np.int64), a["sample_packets"].astype(np.int64)
    assert np.array_equal(pk, np.arange(n))
    assert 0 < sp.size < n and np.all(np.diff(sp) > 0)
    assert np.array_equal(a["compressed_len"], clen.astype(np.float32))
    assert np.array_equal(a["decompressed_len"], l.astype(np.float32))
    assert a["compressed_sum"].tolist() == [_weighted(cout[coff[i]: coff[i] + clen[i]]) for i in range(n)]
    assert a["decompressed_sum"].tolist() == [_weighted(d[o[i]: o[i] + l[i]]) for i in range(n)]
    assert np.array_equal(a["compressed_sample"],
                          np.concatenate([cout[coff[i]: coff[i] + clen[i]] for i in sp]).astype(np.float32))
    assert np.array_equal(a["decompressed_sample"],
                          np.concatenate([d[o[i]: o[i] + l[i]] for i in sp]).astype(np.float32))
    # the room between the packets is no output: other bytes there, the same arrays
    other = np.where(written, cout, cout ^ 0x5A).astype(np.uint8)
    b = dump("b", other)
    assert all(np.array_equal(a[k], b[k]) for k in NAMES)
    # one bit of one packet outside the byte sample shows in that packet's sum alone
    i = int(np.setdiff1d(np.flatnonzero(clen > 0), sp)[0])
    flipped = cout.copy()
    flipped[coff[i] + clen[i] - 1] ^= 1
    c = dump("c", flipped)
    assert np.flatnonzero(c["compressed_sum"] != a["compressed_sum"]).tolist() == [i]
    # lengths beyond a packet's slot are written as they came, and nothing is read outside the slot
    bad = l.copy()
    bad[3] += 5000
    e = dump("e", cout, bad)
    assert e["decompressed_len"][3] == float(bad[3]) and e["decompressed_sum"][3] == a["decompressed_sum"][3]


@pytest.mark.gpu
def test_plain_run_dumps_what_it_computed(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from oracle.pyoracle import Coder
    n = 300
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--workload", "c4", "--packets", str(n), "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["bit_exact_roundtrip"]
    assert not {"configs", "crc32", "pcie_inclusive", "datagram_path", "multi_device_c_abi", "cpu_baseline"} & set(line)
    a = _load(str(tmp_path / "out"))
    d, o, l = bench.make_batch("c4", n, 1200, 0)
    port = Coder("port")
    comp = [port.compress(d[int(o[i]): int(o[i]) + int(l[i])].tobytes()) for i in range(n)]
    comp = [np.frombuffer(c, np.uint8)[:k] for k, c in comp]
    sp = a["sample_packets"].astype(np.int64)
    assert np.array_equal(a["packets"], np.arange(n)) and np.array_equal(sp, np.arange(n))
    assert np.array_equal(a["compressed_len"], np.array([c.size for c in comp], np.float32))
    assert np.array_equal(a["decompressed_len"], l.astype(np.float32))
    assert a["compressed_sum"].tolist() == [_weighted(c) for c in comp]
    assert np.array_equal(a["compressed_sample"], np.concatenate(comp).astype(np.float32))
    assert np.array_equal(a["decompressed_sample"], d.astype(np.float32))
