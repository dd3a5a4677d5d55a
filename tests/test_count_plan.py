"""wsr_count_bool on the host: the header declares both entry points, the
library exports them and a null call is refused with a message; the plan of a
call (plan_count in wiser_amd/csrc/bool_plan.cc) on CPU over a hand-made image
directory -- k ignored, the settled queries, the items against plan_bool's for
the same queries, every error code with its message
(tests/cpp/count_plan_check.cc).  CPU only."""
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "count_plan_check")


def test_header_declares_and_library_exports(built):
    import wiser_amd as w
    from wiser_amd import _capi
    for name in ("wsr_count_bool", "wsr_count_bool_ex"):
        assert name in _capi.header_symbols()
        assert hasattr(_capi.lib, name)
    assert _capi.lib.wsr_count_bool(None, None, 0, None) == _capi.E_INVALID
    assert b"null argument" in _capi.lib.wsr_last_error()
    assert _capi.lib.wsr_count_bool_ex(None, None, 1, None, 0, None) == _capi.E_INVALID
    assert b"null argument" in _capi.lib.wsr_last_error()
    assert hasattr(w.VacuumEngine, "count_bool") and hasattr(w.VacuumEngine, "count")


def test_count_plan_check(built):
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["ok k_ignored", "ok settled", "ok items", "ok errors"]
