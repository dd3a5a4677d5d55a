"""Static VALU / SALU counts of the two-term lean kernel's block loop per stage
and per decode helper (DESIGN.md 5.0000's table, finer): kernels.hip is
compiled for gfx950 to assembly with line tables, with one copy of the
pipeline in lean_kernel<false, true, false> (the bucket copy compiled out; the
16-bit doc id copy or the unpack copy, by argument), and every instruction of
that kernel is attributed to the source line of its .loc.  A line belongs to
the helper or the stage lambda whose text holds it (an inlined helper's
instructions carry the helper's lines, so pair_words, pair_values, pair_shift
and the DPP scan are apart from the stage that calls them).

Counted: the instructions between the first and the last one attributed to C,
H, D or the loop body, i.e. the loop of two blocks with the scoring of a chunk
inside; W's prologue copy in front of the loop is not in it.  v_* are VALU, s_*
SALU (waits, nops and branches included), the rest (loads, stores, LDS) other.

usage: stage_insts.py [KERNELS_HIP] [unpack|doc16]   -> one JSON object"""
import json
import os
import re
import subprocess
import sys
import tempfile

src = sys.argv[1] if len(sys.argv) > 1 else "wiser_amd/csrc/kernels.hip"
copy = sys.argv[2] if len(sys.argv) > 2 else "unpack"
text = open(src).read()
# one copy of the pipeline: no bucket copy; the 16-bit copy for every item or for none
text = text.replace("uni(static_cast<uint32_t>(Q.o_bm >> kProbeShiftBit))", "false")
text = text.replace("uni(Q.a_d16) != kNoDoc16", "true" if copy == "doc16" else "false")
lines = text.splitlines()


def at(pat, start=0):
    return next(i for i in range(start, len(lines)) if re.search(pat, lines[i])) + 1   # 1-based


seg = at(r"^__device__ __forceinline__ void lean_segment\(")
marks = [("flush", at(r"auto flush = ", seg)), ("score", at(r"auto score_chunk = ", seg)),
         ("regs", at(r"struct Regs", seg)), ("pair_shift", at(r"auto pair_shift = ", seg)),
         ("W", at(r"auto issue_words = ", seg)), ("C", at(r"auto stage_C = ", seg)),
         ("H", at(r"auto stage_H = ", seg)), ("D", at(r"auto stage_D = ", seg)),
         ("body", at(r"auto body = ", seg)), ("end", at(r"^// -+ single-term segment", seg))]
ranges = [(n, a, b) for (n, a), (_, b) in zip(marks, marks[1:])]
ranges.append(("setup", seg, marks[0][1]))
pw, pv = at(r"void pair_words\("), at(r"void pair_values\(")
ranges += [("pair_words", pw, at(r"^}", pw) + 1), ("pair_values", pv, at(r"^}", pv) + 1),
           ("dpp_scan", at(r"^template <int CTRL"), at(r"uint32_t wave_incl_scan\(") + 1)]
d0, d1 = marks[7][1], marks[8][1]
adds = {i + 1 for i in range(d0, d1) if re.match(r"\s*(uint32_t )?a[01] = (prev|a0) ", lines[i])}


def bucket(line):
    if line in adds:
        return "D_adds"
    for n, a, b in ranges:
        if a <= line < b:
            return n
    return "other"


with tempfile.TemporaryDirectory() as tmp:
    hip = os.path.join(tmp, "kernels.hip")
    open(hip, "w").write(text)
    asm = os.path.join(tmp, "k.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                    "-ffp-contract=off", "--offload-device-only", "-gline-tables-only", "-S",
                    "-I", os.path.dirname(os.path.abspath(src)), hip, "-o", asm],
                   check=True, stderr=subprocess.DEVNULL)
    out = open(asm).read().splitlines()

start = next(i for i, l in enumerate(out) if l.startswith("_ZN5wiser11lean_kernelILb0ELb1ELb0E"))
end = next(i for i in range(start, len(out)) if out[i].startswith("\t.end_amdhsa_kernel") or ".Lfunc_end" in out[i])
main_file = None
insts, cur = [], None   # (bucket, kind)
for l in out[start:end]:
    s = l.strip()
    m = re.match(r"\.loc\s+(\d+)\s+(\d+)", s)
    if m:
        cur = (m.group(1), int(m.group(2)))
        continue
    if not s or s.startswith((".", ";", "//")) or s.endswith(":"):
        continue
    op = s.split()[0]
    kind = "valu" if op.startswith("v_") else "salu" if op.startswith("s_") else "other"
    insts.append((cur, kind))
# the file number of kernels.hip: the one most instructions carry
files = {}
for c, _ in insts:
    if c:
        files[c[0]] = files.get(c[0], 0) + 1
main_file = max(files, key=files.get)
tagged = [(bucket(c[1]) if c and c[0] == main_file else "other", k) for c, k in insts]
loop = [i for i, (b, _) in enumerate(tagged) if b in ("C", "H", "D", "D_adds", "body")]
table = {}
for b, k in tagged[loop[0]:loop[-1] + 1]:
    table.setdefault(b, {"valu": 0, "salu": 0, "other": 0})[k] += 1
print(json.dumps({"kernel": "lean_kernel<false, true, false>", "copy": copy, "loop_of_blocks": 2,
                  "code_bytes_note": "one copy of the pipeline compiled in",
                  "per_bucket": dict(sorted(table.items()))}, indent=1))
