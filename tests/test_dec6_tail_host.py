"""Host (CPU) build of the record-light decoder (rc_dec6.hip through
tests/proto/lane_host.cpp, variants v6 and v6s) with -DDEC6_TAIL=0..3: every
setting compiles from the one source and decodes tests/dec6_tail_cases.py's
packets and 64 random 1200-B packets as the oracle does, itself (nothing left
to the lane kernels).  One lane, so a stall ends the block at once: this is
the path of a block that requested nothing, and the tail steps of a lane that
does not stall; tests/test_gpu_dec6_tail.py runs the wavefront.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import dec6_tail_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAILS = (0, 1, 2, 3)
VARIANTS = {"v6": ["-DDEC6"], "v6s": ["-DDEC6", "-DDEC6S"]}


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """The eight builds, compiled side by side."""
    out = tmp_path_factory.mktemp("dec6_tail")
    csrc = os.path.join(ROOT, "enet_amd", "csrc")
    procs = {}
    for v, flags in VARIANTS.items():
        for k in TAILS:
            so = str(out / f"liblanehost_{v}_t{k}.so")
            procs[v, k] = (so, subprocess.Popen(
                ["g++", "-O2", "-std=c++17", "-fPIC", "-shared"] + flags + [f"-DDEC6_TAIL={k}", "-I", csrc, "-I",
                 os.path.join(ROOT, "tests", "proto"), "-o", so, os.path.join(ROOT, "tests", "proto", "lane_host.cpp")]))
    res = {}
    for key, (so, pr) in procs.items():
        assert pr.wait() == 0, key
        lib = C.CDLL(so)
        lib.lane_host_run.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32,
                                      C.POINTER(C.c_uint32)]
        res[key] = lib
    return res


@pytest.fixture(scope="module")
def work():
    """(name, packet, the oracle's stream), computed once."""
    from oracle.pyoracle import Coder
    port = Coder("port")
    rng = np.random.default_rng(29)
    packets = [(c.name, c.packet) for c in tc.all_cases()]
    packets += [(f"random1200/{i}", rng.integers(0, 256, size=1200, dtype=np.uint8).tobytes()) for i in range(64)]
    return [(n, p, port.compress(p, 2 * len(p) + 64)[1]) for n, p in packets]


def _decode(lib, stream, cap):
    a = np.frombuffer(bytes(stream) + b"\0" * 16, dtype=np.uint8).copy()
    out = np.zeros(cap + 16, np.uint8)
    ol = C.c_uint32()
    rc = lib.lane_host_run(1, a.ctypes.data, len(stream), out.ctypes.data, cap, max(len(stream), 16), C.byref(ol))
    return rc, ol.value, out[: ol.value].tobytes()


def test_cases_sit_where_planned():
    for c in tc.all_cases():
        assert tc.repeats(c.packet)[0] == tc.planned_first_repeat(c), c.name
    for b in tc.whole_wave_batches():
        assert b.dec_lanes == 0 and len(set(b.packets[:64])) == 1, b.name


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_tail_builds_decode_as_the_oracle(libs, work, variant, tail):
    lib = libs[variant, tail]
    for name, p, stream in work:
        for cap in (len(p), 4096):
            rc, n, got = _decode(lib, stream, cap)
            assert rc == 0, (name, cap, "left to the lane kernels" if rc == 2 else "exact path")
            assert (n, got) == (len(p), p), (name, cap)
