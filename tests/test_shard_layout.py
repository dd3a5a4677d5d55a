"""The doc-range shard exchange's region layout (wiser_amd/csrc/shard_layout.h) on
CPU: its sizes against the formula, every meta pair and slot inside the buffer
and apart from the others, and the sender's emission view against the owner's
replay job through an all-to-all, for a batch's own buffers and a step group's
(tests/cpp/shard_layout_check.cc)."""
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "shard_layout_check")


def test_shard_layout_check():
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == [
        "ok sizes", "ok ranges", "ok sender_owner_agree", "ok wide_arithmetic"]


def test_region_events_matches_the_library(built):
    """shard.py's region size (the host exchange's) is the header's."""
    import ctypes as C

    from wiser_amd import _capi
    from wiser_amd.shard import region_events
    n = C.c_uint64()
    for qpr, slot in ((1, 1), (2, 5), (3, 1), (8, 5), (1024, 0xFFFFFFFF)):
        _capi.check(_capi.lib.wsr_shard_step_regions(qpr, slot, C.byref(n)))
        assert n.value == 16 * region_events(qpr, slot)
