"""Builder of the staged ("stair") corpus that pins the MaxScore window
skipping of the windowed traversal, next to edge_corpora.py.
Deterministic: the same call gives the same index.

73,728 docs = 36 aligned windows of 2,048, the last four past doc 65,535.  The
terms lie in idf tiers, so that a query over them sheds its slots one tier at
a time as its threshold rises:

  hi    48 postings in three groups of 16: G1 in window 0 (hi alone, tf 4-6,
        the doc as long as its tf: above twice lo's bound, below lo's + mid's),
        G2 in window 17 and G3 in window 33 (hi with mid, lo or lo2: above
        lo's + mid's bound)
  mid   about 560 postings (five blocks): clusters in windows 0, 3, 6, 9, 20,
        28 and 34, inside the hi groups, and single postings at window edges
        (doc % 2048 in {0, 1, 2047}) in windows 5, 6, 9 and 24
  lo    115 postings in every window but the two empty ones (31 blocks), tf
        1-3, doc lengths 2, 3, 4 and 6
  lo2   94 postings per window (25 blocks), as lo
  ban   a MUST_NOT list: some docs of each hi group, 30 lo docs in each of
        windows 1, 8 and 35, and a few docs of its own
  z     filler: the docs with no term are six tokens long, which keeps the
        average length near 6 and the short hi docs close to their bound

Windows 12 and 30 hold no term at all; more than twenty hold lo / lo2 alone."""
import os
import random

from edge_corpora import TOKEN_ONLY_HEADER

WINDOW = 2048
N_WINDOWS = 36
N_DOCS = N_WINDOWS * WINDOW
EMPTY_WINDOWS = (12, 30)
HI_WINDOWS = (0, 17, 33)
# window -> (first doc % 2048, postings) of a mid cluster (every second doc from there)
MID_CLUSTERS = {0: (900, 70), 3: (40, 80), 6: (1000, 80), 9: (1500, 80), 20: (300, 80), 28: (1200, 80), 34: (64, 60)}
# single mid postings at window edges: (window, doc % 2048)
MID_EDGES = ((5, 0), (5, 1), (5, 2047), (6, 0), (9, 2047), (24, 0), (24, 1), (24, 2047))
G1 = [0 * WINDOW + 300 + 5 * j for j in range(16)]
G2 = [17 * WINDOW + 700 + 3 * j for j in range(16)]
G3 = [33 * WINDOW + 100 + 7 * j for j in range(16)]
SHARD_CUTS = (G2[7], 18 * WINDOW)   # inside the second hi group; the window-aligned 36,864
LO_PER_WINDOW, LO2_PER_WINDOW = 115, 94


def stair_docs():
    """-> the token list of every doc"""
    rng = random.Random(0x57A1)
    docs = [None] * N_DOCS
    # the hi groups
    for j, d in enumerate(G1):
        docs[d] = ["hi"] * (4 + j % 3) if j not in (0, 5, 9) else ["hi"] * 3 + ["mid"] * 2
        if j in (5, 11):
            docs[d] = docs[d] + ["ban"]
    for j, d in enumerate(G2):
        docs[d] = ["hi"] * 4 + ["mid"] * 2 if j < 14 else ["hi"] * 3 + ["lo"] * 2
        if j in (2, 3, 15):
            docs[d] = docs[d] + ["ban"]
    for j, d in enumerate(G3):
        docs[d] = (["hi"] * (3 + j % 4) + ["mid"] * 2 if j < 8 else ["hi"] * 4 + ["lo2"] * 2 if j < 12
                   else ["hi"] * (3 + j % 4))
        if j in (1, 9, 13):
            docs[d] = docs[d] + ["ban"]
    # mid: clusters (half of their docs hold lo as well) and edge postings
    for w, (r0, n) in MID_CLUSTERS.items():
        for j in range(n):
            toks = ["mid"] * rng.choice([1, 2, 2, 3])
            if j % 2:
                toks += ["lo"] * rng.choice([1, 2, 3])
            elif j % 4 == 0:
                toks += ["z"] * rng.choice([1, 2])
            docs[w * WINDOW + r0 + 2 * j] = toks
    for w, r in MID_EDGES:
        docs[w * WINDOW + r] = ["mid"] * 2 + ["z"]
    # lo and lo2 in every window but the empty ones, tf 1-3, lengths 2, 3, 4 and 6
    for w in range(N_WINDOWS):
        if w in EMPTY_WINDOWS:
            continue
        free = [d for d in range(w * WINDOW, (w + 1) * WINDOW) if docs[d] is None]
        have = sum(1 for d in range(w * WINDOW, (w + 1) * WINDOW) if docs[d] and "lo" in docs[d])
        have2 = sum(1 for d in range(w * WINDOW, (w + 1) * WINDOW) if docs[d] and "lo2" in docs[d])
        picked = rng.sample(free, (LO_PER_WINDOW - have) + (LO2_PER_WINDOW - have2) + 6)
        n_lo, n_lo2 = LO_PER_WINDOW - have, LO2_PER_WINDOW - have2
        for i, d in enumerate(picked):
            if i < n_lo:
                toks = ["lo"] * rng.choice([1, 2, 3])
                if i % 5 == 0 and n_lo2 > 0:   # (a doc of both lists)
                    toks += ["lo2"]
                    n_lo2 -= 1
            elif i < n_lo + n_lo2:
                toks = ["lo2"] * rng.choice([1, 2, 3])
            else:
                break
            if w in (1, 8, 35) and i < 30:
                toks += ["ban"]
            toks += ["z"] * max(0, rng.choice([2, 3, 4, 6]) - len(toks))
            docs[d] = toks
        for d in picked[-6:]:
            if docs[d] is None and w in (1, 8, 20, 35):
                docs[d] = ["ban", "z"]   # ban alone
    for d in range(N_DOCS):
        if docs[d] is None:
            docs[d] = ["z"] * 6
    return docs


def build_stair_index(root):
    """stair_docs() as a TOKEN_ONLY index -> index dir"""
    import wiser_amd as w
    root = str(root)
    path = os.path.join(root, "stair.linedoc")
    with open(path, "w") as f:
        f.write(TOKEN_ONLY_HEADER)
        for toks in stair_docs():
            line = " ".join(toks)
            f.write(f"t\t{line}\t{line}\n")
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(path, d, "TOKEN_ONLY")
    return d
