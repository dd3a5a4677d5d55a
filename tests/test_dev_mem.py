"""The engine's buffer owner (wiser_amd/csrc/dev_mem.h) on CPU, over a fake
memory policy that tracks live blocks and can fail an allocation: growth only
above capacity and to exactly the asked capacity, a failed regrowth leaves the
buffer (or the whole group) empty and reusable, moves and destruction free
every block once (tests/cpp/dev_mem_check.cc)."""
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "dev_mem_check")


def test_dev_mem_check():
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["ok reserve", "ok failed_alloc", "ok group", "ok move", "ok destruct"]
