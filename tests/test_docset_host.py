"""Doc sets on the host (include/wiser_hip.h, wsr_docset; wiser_amd/csrc/
docset.cc): the header declares the seven entry points, the library exports
them, null calls are refused with a message, both mirrors carry the surface
and docset_cli builds.  CPU only."""
import inspect
import os

from conftest import ROOT

ENTRY_POINTS = ("wsr_docset_from_ids", "wsr_docset_from_bool", "wsr_docset_count", "wsr_docset_ids",
                "wsr_docset_destroy", "wsr_search_bool_filtered", "wsr_count_bool_filtered")


def test_header_declares_and_library_exports(built):
    from wiser_amd import _capi
    for name in ENTRY_POINTS:
        assert name in _capi.header_symbols(), name
        assert hasattr(_capi.lib, name), name


def test_null_calls_are_refused(built):
    import ctypes as C
    from wiser_amd import _capi
    lib = _capi.lib
    out, n = C.c_void_p(), C.c_int64(-7)
    one = (_capi.BoolQuery * 1)()
    hits, nh, counts = (_capi.Hit * 1)(), (C.c_int32 * 1)(-7), (C.c_int64 * 1)(-7)
    calls = [lambda: lib.wsr_docset_from_ids(None, None, 0, C.byref(out)),
             lambda: lib.wsr_docset_from_bool(None, one, None, 0, C.byref(out)),
             lambda: lib.wsr_docset_count(None, None, C.byref(n)),
             lambda: lib.wsr_docset_ids(None, None, None, 0, C.byref(n)),
             lambda: lib.wsr_search_bool_filtered(None, one, 1, None, 1, hits, nh, 0, None),
             lambda: lib.wsr_count_bool_filtered(None, one, 1, None, counts, 0, None)]
    for call in calls:
        lib.wsr_search_bool(None, None, -1, 0, None, None)   # (another message in the slot)
        assert call() == _capi.E_INVALID
        assert b"null argument" in lib.wsr_last_error()
    assert out.value is None and n.value == -7 and nh[0] == -7 and counts[0] == -7
    lib.wsr_docset_destroy(None, None)   # (ignored)


def test_mirrors_and_cli(built):
    import wiser_amd as w
    for name in ("docset", "docset_from_bool"):
        assert hasattr(w.VacuumEngine, name)
    for name in ("count", "ids", "close", "__enter__", "__exit__"):
        assert hasattr(w.DocSet, name)
    for fn in (w.VacuumEngine.search_bool, w.VacuumEngine.count_bool):
        assert inspect.signature(fn).parameters["filters"].default is None
    assert inspect.signature(w.VacuumEngine.docset_from_bool).parameters["within"].default is None
    with open(os.path.join(ROOT, "include", "wiser_hip_engine.hpp")) as f:
        hpp = f.read()
    for word in ("class DocSet", "MakeDocSet(const std::vector<int32_t>& ids)", "MakeDocSet(const BoolQuery& q",
                 "wsr_search_bool_filtered", "wsr_count_bool_filtered"):
        assert word in hpp, word
    cli = os.path.join(ROOT, "wiser_amd", "_lib", "docset_cli")
    assert os.path.isfile(cli) and os.access(cli, os.X_OK)
