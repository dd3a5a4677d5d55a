"""The bloom filters of doc-range shard images on the host (no GPU):
build_image places a list's bloom box b at the image's row b - r0, r0 the
list's first skip row in the image, which is above 0 only in a shard.
tests/cpp/bloom_image_check.cc builds the whole image and the shard images of
the tampered tie corpus (3-way split and the hand-made 4-way tiling) and of the
tampered skewed corpus of seed 1 (3-way split and the cut through the widest
gap of x127 / x128 / x129) and compares every shard block's filters with the
whole image's block of the same list and last doc id; the blanked boxes
(bloom_tamper.py) make a misplaced box visible as an empty block where a filled
one belongs, or the reverse."""
import os
import subprocess

import pytest

from bloom_tamper import tampered_copy
from conftest import BLOOM_ENTRIES, BLOOM_RATIO, ROOT
from test_gpu_shard_instances import HAND4, widest_gap_cut

CHECK = os.path.join(ROOT, "wiser_amd", "_lib", "bloom_image_check")


@pytest.mark.parametrize("corpus", ["tiespos", "rand1"])
def test_shard_image_filters_equal_whole_image(built, tmp_path, corpus):
    from edge_corpora import build_skewed_index, build_tie_index
    from oracle.oracle import OracleVacuum
    from wiser_amd.shard import shard_range
    bloom = (BLOOM_RATIO, BLOOM_ENTRIES)
    src = (build_tie_index(tmp_path, positions=True, bloom=bloom) if corpus == "tiespos"
           else build_skewed_index(tmp_path, 1, bloom=bloom)[0])
    d = str(tmp_path / "tampered")
    blanked = tampered_copy(src, d, corpus)
    orc = OracleVacuum(d)
    try:
        n = orc.n_docs()
        ranges = [tuple(shard_range(n, r, 3)) for r in range(3)]
        if corpus == "tiespos":
            assert n == HAND4[-1][1]
            ranges += HAND4
        else:
            ranges += widest_gap_cut(orc, n)[1]
    finally:
        orc.close()
    args = [CHECK, d]
    for lo, hi in ranges:
        args += ["range", str(lo), str(hi)]
    for t, bs in blanked.items():
        args += ["blank", t, ",".join(map(str, bs))]
    out = subprocess.run(args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr + out.stdout
    got = dict(zip(out.stdout.split()[0::2], map(int, out.stdout.split()[1::2])))
    assert got["ranges"] == len(ranges) and got["blanked"] > 0 and got["filled"] > 0 and got["late_starts"] > 0, got
