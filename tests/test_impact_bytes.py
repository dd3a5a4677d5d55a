"""The impact byte of a posting (IndexArgs::impact, built at load next to
bmax): the lean pipeline prunes on it instead of the posting's tf and length
code, so the value a byte is read as must never fall below the exact
tf / (tf + cache_[c4]) it stands for, whatever the tf (the 1-byte tf escape
included: the loader uses the real tf) and whatever the length code.

wsr_impact_byte answers with the loader's own function (engine_types.h
impact_byte), no engine needed.  The exact value is computed here, in IEEE
double with the reference's operation order (heapmodel.norm).
"""
import ctypes as C

import pytest

from heapmodel import norm

TFS = list(range(1, 301)) + [1000, 65535, 1 << 20, (1 << 31) - 1]
STEP = 1.0 / 255.0


@pytest.mark.parametrize("avg", [1.0, 3.25, 37.5, 412.0, 6500.125])
def test_impact_byte_conservative_and_monotone(built, avg):
    from wiser_amd._capi import check, lib
    b, v = C.c_uint32(), C.c_double()
    value_of = {}
    for c in range(256):
        nrm = norm(c, avg)
        assert nrm > 0.0
        prev_b, prev_v = 0, 0.0
        for tf in TFS:
            check(lib.wsr_impact_byte(avg, tf, c, C.byref(b), C.byref(v)))
            exact = tf / (tf + nrm)
            assert 0 <= b.value <= 255
            assert v.value >= exact, (avg, c, tf, b.value, v.value, exact)
            # one quantisation step at most above it (the step, 1/255, plus the
            # scale's and the product's f32 rounding, below 1e-6 of the value)
            assert v.value - exact <= STEP * (1 + 1e-6) + 1e-6, (avg, c, tf, b.value, v.value, exact)
            # monotone in tf for a fixed code, bytes and values
            assert b.value >= prev_b and v.value >= prev_v, (avg, c, tf)
            prev_b, prev_v = b.value, v.value
            # the value is a function of the byte alone (what the kernel reads)
            assert value_of.setdefault(b.value, v.value) == v.value
    assert value_of[255] >= 1.0
    assert all(value_of[q] < value_of[r] for q, r in zip(sorted(value_of), sorted(value_of)[1:]))


def test_impact_byte_rejects_bad_arguments(built):
    from wiser_amd._capi import lib
    b, v = C.c_uint32(), C.c_double()
    assert lib.wsr_impact_byte(10.0, 1, 256, C.byref(b), C.byref(v)) != 0
    assert lib.wsr_impact_byte(0.0, 1, 3, C.byref(b), C.byref(v)) != 0
    assert lib.wsr_impact_byte(10.0, 1, 3, None, C.byref(v)) != 0


def test_image_info_counts_impact_bytes(synth_small):
    """One impact byte per posting slot, as plen, counted inside dir_bytes."""
    import wiser_amd as w
    d, _ = synth_small
    info = w.image_size(d, threads=4)
    assert info["impact_bytes"] == info["plen_bytes"] > 0
    assert info["dir_bytes"] > info["impact_bytes"]
