"""The host shim's copy threads (enet_amd/csrc/rc_hostcopy.c: the pool,
rc_par_memcpy / rc_par_scatter / rc_par_gather) on the CPU: the stand-alone
program tests/proto/hostcopy_main.c checks them against serial loops, built
once with AddressSanitizer + UBSan and once with ThreadSanitizer."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "enet_amd", "csrc")


@pytest.mark.parametrize("sanitize", ["address,undefined", "thread"])
def test_hostcopy_sanitized(tmp_path, sanitize):
    exe = str(tmp_path / "hostcopy")
    subprocess.check_call(["gcc", "-O1", "-g", "-pthread", "-std=c11", f"-fsanitize={sanitize}",
                           "-fno-sanitize-recover=undefined", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           os.path.join(HERE, "proto", "hostcopy_main.c"), os.path.join(CSRC, "rc_hostcopy.c"),
                           "-o", exe])
    env = {k: v for k, v in os.environ.items() if not k.startswith("ENET_RC_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "hostcopy ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-2000:]
