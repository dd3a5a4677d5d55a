"""wsr_search_bool on the host: the header declares the entry points and the
query struct, the library exports them and the ctypes mirror agrees with the
header's layout; the plan of a call (wiser_amd/csrc/bool_plan.cc) on CPU over a
hand-made image directory -- the slot masks, lead and need_should, the queries
settled on the host, the MaxScore sums without MUST_NOT slots, item ranges and
event-slot caps, and every error code with its message
(tests/cpp/bool_plan_check.cc).  CPU only."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "bool_plan_check")


def test_header_declares_and_library_exports(built):
    import wiser_amd as w
    from wiser_amd import _capi
    for name in ("wsr_search_bool", "wsr_check_bool_query", "wsr_search_bool_ex"):
        assert name in _capi.header_symbols()
        assert hasattr(_capi.lib, name)
    text = open(_capi.HEADER).read()
    assert "typedef struct wsr_bool_query" in text and "} wsr_bool_query;" in text
    assert "enum { WSR_ROLE_SHOULD = 0, WSR_ROLE_MUST = 1, WSR_ROLE_MUST_NOT = 2 };" in text
    assert (_capi.ROLE_SHOULD, _capi.ROLE_MUST, _capi.ROLE_MUST_NOT) == (0, 1, 2)
    assert _capi.lib.wsr_search_bool(None, None, 0, 0, None, None) == _capi.E_INVALID
    assert b"null argument" in _capi.lib.wsr_last_error()
    assert _capi.lib.wsr_check_bool_query(None, None) == _capi.E_INVALID
    assert w.BoolQuery([("a", "must")]).n_results == 10 and w.BoolQuery([]).min_should == 0
    assert hasattr(w.VacuumEngine, "search_bool")


def test_bool_query_layout(built, tmp_path):
    """the ctypes mirror agrees with wsr_bool_query as compiled by gcc (the header is C)"""
    from wiser_amd import _capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wiser_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(wsr_bool_query),'
                   ' offsetof(wsr_bool_query, n_terms), offsetof(wsr_bool_query, k),'
                   ' offsetof(wsr_bool_query, list_ids), offsetof(wsr_bool_query, role),'
                   ' offsetof(wsr_bool_query, min_should)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    B = _capi.BoolQuery
    assert got == [C.sizeof(B), B.n_terms.offset, B.k.offset, B.list_ids.offset, B.role.offset,
                   B.min_should.offset] == [92, 0, 4, 8, 72, 88]


def test_bool_plan_check(built):
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["ok roles", "ok settled", "ok items", "ok errors"]
