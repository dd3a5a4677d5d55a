"""The host's plan of a batch upload (wiser_amd/csrc/batch_plan.cc) on CPU, over
a hand-made image directory: the instance flags, the class rule it shares with
the device plan at its boundaries, the grids, the event and item workspaces,
long and disjunctive queries, the error codes and messages, and which
persistent kernels a run launches (tests/cpp/batch_plan_check.cc)."""
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "batch_plan_check")


def test_batch_plan_check():
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == [
        "ok instance_flags", "ok class_rule", "ok grids", "ok invalid_queries", "ok workspace",
        "ok long_queries", "ok or_queries", "ok errors", "ok launches_of", "ok reuse"]
