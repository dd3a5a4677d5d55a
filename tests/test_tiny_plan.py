"""The tiny class in the host's plan of a batch upload (batch_plan.cc) on CPU,
over a hand-made image directory: the batch's tiny count equals the rule of
engine_types.h applied query by query, the general grid that is left, and
which runs have the class (tests/cpp/tiny_plan_check.cc)."""
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "tiny_plan_check")


def test_tiny_plan_check():
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["ok rule", "ok count", "ok grids", "ok launches_of"]
