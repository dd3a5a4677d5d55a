"""Builders of the small edge-case corpora the GPU parity tests share (next to
bucket_corpus.py): the tie corpus of test_gpu_prune.py, the random skewed
corpora of test_gpu_random.py and the large-tf corpus of
test_large_tf_dense_escape.  Every builder is deterministic: the same
arguments give the same index."""
import os
import random

TOKEN_ONLY_HEADER = "FIELDS_HEADER_INDICATOR###\tdoctitle\tbody\ttokenized\n"
POSITIONS_HEADER = "FIELDS_HEADER_INDICATOR###\tdoctitle\tbody\ttokenized\toffsets\tpositions\n"


def positions_row(seq):
    """One WITH_POSITIONS linedoc row of the token sequence seq."""
    occ, offs, at = {}, {}, 0
    for p, w in enumerate(seq):
        occ.setdefault(w, []).append(p)
        offs.setdefault(w, []).append((at, at + len(w)))
        at += len(w) + 1
    toks = list(occ)
    off_col = "".join("".join(f"{s},{e};" for s, e in offs[w]) + "." for w in toks)
    pos_col = "".join("".join(f"{p};" for p in occ[w]) + "." for w in toks)
    return f"t\t{' '.join(seq)}\t{' '.join(toks)}\t{off_col}\t{pos_col}\n"


def build_tie_index(root, positions=False, bloom=None):
    """20,000 docs built for score ties: doc lengths from four values and tfs
    1..3 of "a" (every doc), "b" (0.8), "c" (0.5) and "d" (0.3), shuffled among
    filler words; doc 7777 holds 300 more "c" (above the 1-byte tf escape).
    positions: the same docs written WITH_POSITIONS (for phrase queries)
    instead of TOKEN_ONLY; bloom = (ratio, entries): also with the two-way phrase
    bloom filters (build_from_linedoc; None: the index as it always was).
    -> index dir"""
    import wiser_amd as w
    root = str(root)
    path = os.path.join(root, "ties.linedoc")
    rng = random.Random(5)
    with open(path, "w") as f:
        f.write(POSITIONS_HEADER if positions else TOKEN_ONLY_HEADER)
        for i in range(20000):
            toks = ["a"] * rng.choice([1, 1, 1, 2, 3])
            if rng.random() < 0.8:
                toks += ["b"] * rng.choice([1, 1, 2])
            if rng.random() < 0.5:
                toks += ["c"] * rng.choice([1, 2, 3])
            if rng.random() < 0.3:
                toks += ["d"]
            if i == 7777:
                toks += ["c"] * 300   # above the tf8 escape: c's tf bound is 303
            n = rng.choice([8, 16, 24, 64])
            toks += [f"f{j}" for j in range(max(0, n - len(toks)))]
            rng.shuffle(toks)
            f.write(positions_row(toks) if positions else f"t\t{' '.join(toks)}\t{' '.join(toks)}\n")
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(path, d, "WITH_POSITIONS" if positions else "TOKEN_ONLY", bloom=bloom)
    return d


SKEWED_FIXED_DF = (1, 2, 127, 128, 129, 255, 256, 300)   # the lists "x<df>" of a skewed corpus


def write_skewed_linedoc(path, seed):
    """WITH_POSITIONS linedoc of a small random corpus with skewed shapes: lists
    of exactly 1 / 2 / 127 / 128 / 129 / 255 / 256 / 300 postings ("x<df>",
    capped by the doc count), a Zipf vocabulary "v<i>", "heavy" with tf 300 in
    every 97th doc, "lonely" in otherwise empty docs; returns the vocabulary."""
    rng = random.Random(seed)
    vocab = [f"v{i}" for i in range(rng.choice([5, 30, 300]))]
    fixed = {f"x{n}": n for n in SKEWED_FIXED_DF}   # term -> df
    n_docs = rng.choice([300, 700, 1500])
    docs = [[] for _ in range(n_docs)]
    for t, df in fixed.items():
        for d in rng.sample(range(n_docs), min(df, n_docs)):
            docs[d].append(t)
    weights = [1.0 / (i + 1) for i in range(len(vocab))]
    for d in range(n_docs):
        docs[d] += rng.choices(vocab, weights, k=rng.choice([0, 1, 3, 20, 80]))
        if d % 97 == 0:
            docs[d] += ["heavy"] * 300          # tf >= 255
        rng.shuffle(docs[d])
        if not docs[d]:
            docs[d] = ["lonely"]
    with open(path, "w") as f:
        f.write(POSITIONS_HEADER)
        for seq in docs:
            f.write(positions_row(seq))
    return vocab + list(fixed) + ["heavy", "lonely", "absent-term"]


def build_skewed_index(root, seed, bloom=None):
    """write_skewed_linedoc(seed) as a WITH_POSITIONS index, with bloom =
    (ratio, entries) also holding the two-way phrase bloom filters
    -> (index dir, vocabulary)"""
    import wiser_amd as w
    root = str(root)
    ld = os.path.join(root, "c.linedoc")
    terms = write_skewed_linedoc(ld, seed)
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(ld, d, "WITH_POSITIONS", bloom=bloom)
    return d, terms


def build_large_tf_index(root):
    """300 docs, TOKEN_ONLY: "x" with tf 1 / 2 / 254 / 255 / 256 / 600 in every
    doc, "y" (tf 1..3) in every other doc, "z" with tf 300 in every 7th and a
    one-posting "w<i>" per doc: tfs around and above the 1-byte escape.
    -> index dir"""
    import wiser_amd as w
    root = str(root)
    ld = os.path.join(root, "big_tf.linedoc")
    rng = random.Random(5)
    with open(ld, "w") as f:
        f.write(TOKEN_ONLY_HEADER)
        for i in range(300):
            toks = ["x"] * rng.choice([1, 2, 254, 255, 256, 600])
            if i % 2 == 0:
                toks += ["y"] * rng.randint(1, 3)
            if i % 7 == 0:
                toks += ["z"] * 300
            toks += [f"w{i}"]
            f.write(f"t\t{' '.join(toks)}\t{' '.join(toks)}\n")
    d = os.path.join(root, "idx")
    os.makedirs(d)
    w.build_from_linedoc(ld, d, "TOKEN_ONLY")
    return d
