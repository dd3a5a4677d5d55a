"""wsr_score_docs on the host: the header declares the entry point and its
answer struct, the library exports it and the ctypes mirror agrees with the
header's layout; the plan of a call (wiser_amd/csrc/score_plan.cc) on CPU over
a hand-made image directory -- the sort is the stable one, every item holds at
most 64 candidates, every candidate that needs the device lands in exactly one
item, the index array is a permutation, and the error codes
(tests/cpp/score_plan_check.cc).  CPU only."""
import ctypes as C
import os
import subprocess

from conftest import ROOT

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "score_plan_check")


def test_header_declares_and_library_exports(built):
    from wiser_amd import _capi
    assert "wsr_score_docs" in _capi.header_symbols()
    assert hasattr(_capi.lib, "wsr_score_docs")
    text = open(_capi.HEADER).read()
    assert "typedef struct wsr_doc_score" in text and "} wsr_doc_score;" in text
    assert _capi.lib.wsr_score_docs(None, None, 0, None, None, None) == _capi.E_INVALID
    assert b"null argument" in _capi.lib.wsr_last_error()


def test_doc_score_layout(built, tmp_path):
    """the ctypes mirror agrees with wsr_doc_score as compiled by gcc"""
    from wiser_amd import _capi
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "wiser_hip.h"\n'
                   'int main(void){printf("%zu %zu %zu\\n", sizeof(wsr_doc_score),'
                   ' offsetof(wsr_doc_score, score), offsetof(wsr_doc_score, mask)); return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(_capi.DocScore), _capi.DocScore.score.offset, _capi.DocScore.mask.offset] == [16, 0, 8]


def test_score_plan_check(built):
    out = subprocess.run([CHECK], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert out.stdout.splitlines() == ["ok sort_and_items", "ok shard_range", "ok empty", "ok errors"]
