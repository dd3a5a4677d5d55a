"""Python mirror of the reference operator surface for the Vacuum engine.

Same names, argument meaning and error behaviour as the reference's
``SearchEngineServiceNew`` implemented by ``VacuumEngine``
(src/qq_mem/src/engine_services.h:14-27, vacuum_engine.h:119-258) and its
``SearchQuery`` / ``SearchResult`` types (types.h:205-346); every call goes
through the C ABI of libwiser_hip.so into the HIP kernels.

    engine = CreateSearchEngine("vacuum:vacuum_dump:/path/to/index")
    engine.Load()
    result = engine.Search(SearchQuery(["hello", "world"], n_results=10))

Behaviour kept from the reference:
  * ``n_results == 0`` -> empty result (vacuum_engine.h:206-208);
  * any term missing from the dictionary -> empty result, ``doc_freqs`` left
    empty (vacuum_engine.h:210-215);
  * entries ordered as the reference heap pops them (SortHeap), f64 scores;
  * ``is_phrase`` with two or more terms ranks only docs holding the terms at
    consecutive positions (QueryProcessor, query_processing.h:854-912); the
    engine must be loaded with ``positions=True`` (the default).
Beyond the reference: ``match_any`` makes a query disjunctive (WSR_QUERY_OR) --
a doc matches when it holds at least one of the terms, a term missing from the
dictionary contributes nothing (``doc_freqs`` has a 0 for it), and the score is
the sum of the BM25 terms of the lists that hold the doc.  Not with
``is_phrase`` or ``return_snippets`` (WSR_E_INVALID).
Snippets (SearchQuery.return_snippets): a host stage after the GPU top-k, as
in the reference (vacuum_engine.h:243-253): offsets from the index, text from the
doc store (my.fdx / my.fdt), SimpleHighlighter -- wsr_snippet in the C ABI.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

from . import _capi
from ._capi import check, lib


@dataclass
class SearchQuery:
    """types.h:205-256"""
    terms: List[str]
    n_results: int = 5
    return_snippets: bool = False
    n_snippet_passages: int = 3
    is_phrase: bool = False
    match_any: bool = False     # disjunctive (OR): rank the docs that hold any of the terms


@dataclass
class BoolQuery:
    """A boolean query (beyond the reference, wsr_search_bool): terms is
    [(term, role)] in query order, role one of "must", "should", "must_not".
    A doc matches when it holds every must term, no must_not term and at least
    max(min_should, 1 if there is no must term else 0) of the should terms (a
    term given twice counts twice); its score is the sum of the BM25 terms of
    the must and should terms it holds, in query order."""
    terms: List[Tuple[str, str]]
    n_results: int = 10
    min_should: int = 0


@dataclass
class SearchResultEntry:
    """types.h:259-274 (snippet filled when the query asks for snippets)"""
    doc_id: int
    doc_score: float
    snippet: str = ""


@dataclass
class SearchResult:
    """types.h:297-346"""
    entries: List[SearchResultEntry] = field(default_factory=list)
    doc_freqs: List[int] = field(default_factory=list)

    def Size(self) -> int:
        return len(self.entries)

    def __getitem__(self, i):
        return self.entries[i]


class DocSet:
    """A set of doc ids of the whole index, resident on the device (wsr_docset;
    VacuumEngine.docset / docset_from_bool): the filter of search_bool and
    count_bool.  Immutable; close() it (or use it as a context manager) before
    its engine is closed."""

    def __init__(self, engine: "VacuumEngine", handle):
        self._engine = engine
        self._s = handle

    def count(self) -> int:
        n = C.c_int64()
        check(lib.wsr_docset_count(self._engine._h, self._s, C.byref(n)))
        return n.value

    def ids(self):
        """The set's doc ids, ascending: a numpy int32 array."""
        import numpy as np
        out = np.empty(self.count(), dtype=np.int32)
        n = C.c_int64()
        check(lib.wsr_docset_ids(self._engine._h, self._s, out.ctypes.data_as(C.POINTER(C.c_int32)), out.size,
                                 C.byref(n)))
        return out[: n.value]

    def close(self) -> None:
        if self._s is not None and self._engine._h is not None:
            lib.wsr_docset_destroy(self._engine._h, self._s)
        self._s = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ParseUrl(url: str):
    """engine_factory.h:21-31: ``vacuum:<source_type>:<path>``."""
    parts = url.split(":", 2)
    if len(parts) != 3 or parts[0] != "vacuum":
        raise ValueError(f"not a vacuum url: {url}")
    return parts[1], parts[2]


def CreateSearchEngine(url: str, bloom_factor: int = 1, device: int = 0) -> "VacuumEngine":
    """engine_factory.h:33-50 (only ``vacuum:vacuum_dump:<dir>`` is served here)."""
    source, path = ParseUrl(url)
    if source != "vacuum_dump":
        raise ValueError(f"unsupported vacuum source type: {source}")
    return VacuumEngine(path, bloom_factor=bloom_factor, device=device)


class VacuumEngine:
    """SearchEngineServiceNew over the HIP engine (vacuum_engine.h:119-258)."""

    def __init__(self, engine_dir_path: str, bloom_factor: int = 1, device: int = 0,
                 doc_range: Optional[Sequence[int]] = None, threads: int = 0,
                 positions: bool = True):
        self.engine_dir_path = engine_dir_path
        self.positions = positions
        self.bloom_factor = bloom_factor
        self.device = device
        self.doc_range = doc_range
        self.threads = threads
        self.snippet_threads = 0     # host threads of the snippet stage (0 = all cores)
        self._h = None

    # ---- SearchEngineServiceNew -------------------------------------
    def Load(self) -> None:
        if self._h is not None:
            raise RuntimeError("Engine is already loaded.")  # vacuum_engine.h:145
        opts = _capi.OpenOpts()
        opts.device = self.device
        opts.doc_lo, opts.doc_hi = (self.doc_range if self.doc_range else (0, 0))
        opts.threads = self.threads
        opts.positions = 1 if self.positions else 0
        opts.bloom_factor = int(self.bloom_factor)
        h = C.c_void_p()
        check(lib.wsr_open(self.engine_dir_path.encode(), C.byref(opts), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if self._h is not None:
            lib.wsr_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def image_info(self) -> Dict[str, int]:
        """HBM bytes of this engine's image per buffer (wsr_image_info_get)."""
        i = _capi.ImageInfo()
        check(lib.wsr_image_info_get(self._h, C.byref(i)))
        return {f: getattr(i, f) for f, _ in _capi.ImageInfo._fields_}

    def TermCount(self) -> int:
        n = C.c_int32()
        check(lib.wsr_term_count(self._h, C.byref(n)))
        return n.value

    def NumDocs(self) -> int:
        n = C.c_int32()
        check(lib.wsr_n_docs(self._h, C.byref(n)))
        return n.value

    def PostinglistSizes(self, terms: Sequence[str]) -> Dict[str, int]:
        out = {}
        for t in terms:
            lid, df = self.lookup(t)
            if lid >= 0:
                out[t] = df
        return out

    def Search(self, query: SearchQuery) -> SearchResult:
        return self.SearchBatch([query])[0]

    # ---- batched extension -----------------------------------------
    def lookup(self, term: str):
        lid, df = C.c_int32(), C.c_int32()
        check(lib.wsr_lookup(self._h, term.encode(), C.byref(lid), C.byref(df)))
        return lid.value, df.value

    def resolve(self, query: SearchQuery):
        """-> (wsr_query, doc_freqs or None) with the reference's empty-result rules.
        A query of more than MAX_TERMS terms carries the rest in more_ids (ctypes
        keeps the array alive with the Query and with every array it is copied into)."""
        if len(query.terms) > _capi.MAX_QUERY_TERMS:
            raise NotImplementedError(f"more than {_capi.MAX_QUERY_TERMS} terms per query")
        if query.n_results > _capi.MAX_K:
            raise NotImplementedError(f"n_results above {_capi.MAX_K}")
        if query.match_any and (query.is_phrase or query.return_snippets):
            raise _capi.WiserError(_capi.E_INVALID, "match_any goes with neither is_phrase nor return_snippets")
        q = _capi.Query()
        q.k = max(0, int(query.n_results))
        q.flags = _capi.QUERY_PHRASE if (query.is_phrase and len(query.terms) > 1) else 0
        ids, dfs = [], []
        for t in query.terms:
            lid, df = self.lookup(t)
            ids.append(lid)
            dfs.append(df)
        missing = any(i < 0 for i in ids) or not ids
        if query.match_any:
            # a missing term contributes nothing (its doc_freq is 0); the engine
            # checks the term limit (WSR_MAX_OR_TERMS)
            q.flags = _capi.QUERY_OR
            missing = not ids
            if len(ids) > _capi.MAX_OR_TERMS:   # (loud whatever k is: k = 0 never reaches the engine's check)
                raise _capi.WiserError(_capi.E_LIMIT, f"more than {_capi.MAX_OR_TERMS} terms in a match_any query")
        q.n_terms = 0 if (missing or q.k == 0) else len(ids)
        for i, lid in enumerate(ids[:_capi.MAX_TERMS]):
            q.list_ids[i] = lid
        if len(ids) > _capi.MAX_TERMS:
            more = (C.c_int32 * (len(ids) - _capi.MAX_TERMS))(*ids[_capi.MAX_TERMS:])
            q.more_ids = C.cast(more, C.POINTER(C.c_int32))
        freqs = None if (missing or q.k == 0) else dfs
        return q, freqs

    def SearchBatch(self, queries: Sequence[SearchQuery]) -> List[SearchResult]:
        if not queries:
            return []
        arr = (_capi.Query * len(queries))()
        freqs = []
        stride = 1
        for i, sq in enumerate(queries):
            q, f = self.resolve(sq)
            arr[i] = q
            freqs.append(f)
            stride = max(stride, q.k)
        hits = (_capi.Hit * (len(queries) * stride))()
        nh = (C.c_int32 * len(queries))()
        check(lib.wsr_search_batch(self._h, arr, len(queries), stride, hits, nh))
        out = []
        for i in range(len(queries)):
            r = SearchResult()
            if freqs[i] is not None:
                r.doc_freqs = list(freqs[i])
                for j in range(nh[i]):
                    h = hits[i * stride + j]
                    r.entries.append(SearchResultEntry(h.doc_id, h.score))
            out.append(r)
        # vacuum_engine.h:248-252: the snippet stage, all entries of the batch at
        # once on the host's threads (grouped by n_snippet_passages)
        groups: Dict[int, List[int]] = {}
        for i, sq in enumerate(queries):
            if sq.return_snippets and freqs[i] is not None and nh[i] > 0:
                groups.setdefault(int(sq.n_snippet_passages), []).append(i)
        for n_passages, idx in groups.items():
            sub_q = (_capi.Query * len(idx))(*[arr[i] for i in idx])
            sub_h = (_capi.Hit * (len(idx) * stride))()
            sub_n = (C.c_int32 * len(idx))(*[nh[i] for i in idx])
            for a, i in enumerate(idx):
                C.memmove(C.byref(sub_h, a * stride * C.sizeof(_capi.Hit)),
                          C.byref(hits, i * stride * C.sizeof(_capi.Hit)), stride * C.sizeof(_capi.Hit))
            snips = _capi.snippets_batch(self._h, sub_q, sub_h, sub_n, stride, n_passages,
                                         self.snippet_threads)
            for a, i in enumerate(idx):
                for e, sn in zip(out[i].entries, snips[a]):
                    e.snippet = sn
        return out

    # ---- boolean queries ------------------------------------------------
    def resolve_bool(self, query: BoolQuery):
        """-> (wsr_bool_query, doc_freqs or None): every term looked up (-1: not
        in the index, its doc_freq 0); doc_freqs None as for match_any (no terms
        or n_results <= 0).  The engine checks the limits."""
        if len(query.terms) > _capi.MAX_OR_TERMS:
            raise _capi.WiserError(_capi.E_LIMIT, f"more than {_capi.MAX_OR_TERMS} terms in a boolean query")
        q = _capi.BoolQuery()
        q.n_terms = len(query.terms)
        q.k = max(0, int(query.n_results))
        q.min_should = int(query.min_should)
        dfs = []
        for i, (t, role) in enumerate(query.terms):
            if role not in _capi.ROLES:
                raise ValueError(f"role {role!r}: one of {sorted(_capi.ROLES)}")
            lid, df = self.lookup(t)
            q.list_ids[i] = lid
            q.role[i] = _capi.ROLES[role]
            dfs.append(df)
        return q, (None if (not dfs or q.k == 0) else dfs)

    # ---- doc sets -------------------------------------------------------
    def docset(self, ids) -> DocSet:
        """wsr_docset_from_ids: the set of the given doc ids of the whole index
        (any order, duplicates allowed; an id outside [0, NumDocs()) is refused)."""
        import numpy as np
        a = np.ascontiguousarray(np.asarray(list(ids) if not hasattr(ids, "dtype") else ids, dtype=np.int64))
        if a.size and (a.min() < -2**31 or a.max() >= 2**31):
            raise _capi.WiserError(_capi.E_INVALID, "a doc id outside int32")
        a = a.astype(np.int32)
        s = C.c_void_p()
        check(lib.wsr_docset_from_ids(self._h, a.ctypes.data_as(C.POINTER(C.c_int32)), a.size, C.byref(s)))
        return DocSet(self, s)

    def docset_from_bool(self, query: BoolQuery, within: Optional[DocSet] = None) -> DocSet:
        """wsr_docset_from_bool: the docs that match the query under search_bool's
        match rule (n_results is ignored), intersected with `within` when given."""
        q = self.resolve_bool(query)[0]
        s = C.c_void_p()
        check(lib.wsr_docset_from_bool(self._h, C.byref(q), within._s if within is not None else None, 0,
                                       C.byref(s)))
        return DocSet(self, s)

    @staticmethod
    def _filter_array(filters, n):
        """filters (one DocSet or None per query) as the C ABI's array"""
        if len(filters) != n:
            raise ValueError("one filter (or None) per query")
        return (C.c_void_p * n)(*[f._s if f is not None else None for f in filters])

    def search_bool(self, queries: Sequence[BoolQuery],
                    filters: Optional[Sequence[Optional[DocSet]]] = None) -> List[SearchResult]:
        """wsr_search_bool: one SearchResult per query, entries ordered as every
        query's, doc_freqs as for Search with match_any (0 for a missing term).
        filters (wsr_search_bool_filtered): one DocSet or None per query; a
        query ranks only the docs of its set."""
        if not queries:
            return []
        n = len(queries)
        arr = (_capi.BoolQuery * n)()
        freqs = []
        stride = 1
        for i, bq in enumerate(queries):
            arr[i], f = self.resolve_bool(bq)
            freqs.append(f)
            stride = max(stride, arr[i].k)
        hits = (_capi.Hit * (n * stride))()
        nh = (C.c_int32 * n)()
        if filters is None:
            check(lib.wsr_search_bool(self._h, arr, n, stride, hits, nh))
        else:
            check(lib.wsr_search_bool_filtered(self._h, arr, n, self._filter_array(filters, n), stride, hits, nh,
                                               0, None))
        out = []
        for i in range(n):
            r = SearchResult()
            if freqs[i] is not None:
                r.doc_freqs = list(freqs[i])
                r.entries = [SearchResultEntry(hits[i * stride + j].doc_id, hits[i * stride + j].score)
                             for j in range(nh[i])]
            out.append(r)
        return out

    # ---- exact match counts ---------------------------------------------
    def count_bool(self, queries: Sequence[BoolQuery],
                   filters: Optional[Sequence[Optional[DocSet]]] = None) -> List[int]:
        """wsr_count_bool: how many docs match each query under search_bool's
        match rule (n_results is ignored; on a doc-range shard engine, the
        matches in the shard's doc range -- the shards of a partition add up).
        filters (wsr_count_bool_filtered): one DocSet or None per query; a
        query counts only the docs of its set."""
        if not queries:
            return []
        n = len(queries)
        arr = (_capi.BoolQuery * n)(*[self.resolve_bool(bq)[0] for bq in queries])
        counts = (C.c_int64 * n)()
        if filters is None:
            check(lib.wsr_count_bool(self._h, arr, n, counts))
        else:
            check(lib.wsr_count_bool_filtered(self._h, arr, n, self._filter_array(filters, n), counts, 0, None))
        return list(counts)

    def count(self, query: SearchQuery) -> int:
        """How many docs a Search of the query would rank from: the docs that
        hold every term, or any term with match_any.  Phrase queries and more
        than MAX_OR_TERMS terms are refused."""
        if query.is_phrase and len(query.terms) > 1:
            raise _capi.WiserError(_capi.E_INVALID, "count takes no phrase query")
        if len(query.terms) > _capi.MAX_OR_TERMS:
            raise _capi.WiserError(_capi.E_LIMIT, f"more than {_capi.MAX_OR_TERMS} terms in a count query")
        role = "should" if query.match_any else "must"
        return self.count_bool([BoolQuery([(t, role) for t in query.terms])])[0]

    # ---- given (query, doc) pairs -------------------------------------
    def resolve_terms(self, query: SearchQuery):
        """-> wsr_query for wsr_score_docs: every term looked up (-1: not in the
        index, it sets no mask bit), none of Search's empty-result rules; k is
        ignored there.  The engine checks the term limit and the flags."""
        q = _capi.Query()
        q.n_terms = len(query.terms)
        q.flags = ((_capi.QUERY_PHRASE if (query.is_phrase and len(query.terms) > 1) else 0) |
                   (_capi.QUERY_OR if query.match_any else 0))
        for i, t in enumerate(query.terms[:_capi.MAX_TERMS]):
            q.list_ids[i] = self.lookup(t)[0]
        return q

    def score_docs_batch(self, queries: Sequence[SearchQuery],
                         doc_id_lists: Sequence[Sequence[int]]) -> List[List[Tuple[float, int]]]:
        """wsr_score_docs: per query, (score, mask) of each of its doc ids, in the
        caller's order.  mask bit t: term t is in the index and its list holds
        the doc; score: the sum of those terms' BM25, in query order from 0.0
        (a full mask: the conjunctive score; any mask: the match_any score)."""
        if len(queries) != len(doc_id_lists):
            raise ValueError("one doc id list per query")
        n = len(queries)
        arr = (_capi.Query * max(n, 1))(*[self.resolve_terms(sq) for sq in queries])
        off = (C.c_int64 * (n + 1))()
        for i, d in enumerate(doc_id_lists):
            off[i + 1] = off[i] + len(d)
        total = off[n]
        docs = (C.c_int32 * max(total, 1))(*[int(x) for d in doc_id_lists for x in d])
        out = (_capi.DocScore * max(total, 1))()
        check(lib.wsr_score_docs(self._h, arr, n, off, docs, out))
        return [[(out[j].score, out[j].mask) for j in range(off[i], off[i + 1])] for i in range(n)]

    def score_docs(self, query: SearchQuery, doc_ids: Sequence[int]) -> List[Tuple[float, int]]:
        """What `query` gives each of doc_ids: [(score, mask)] (score_docs_batch)."""
        return self.score_docs_batch([query], [doc_ids])[0]

    def snippet(self, q, doc_id: int, n_passages: int) -> str:
        """VacuumEngine::GenerateSnippet for result entry doc_id of resolved query q."""
        # (a 1-term phrase query is a plain query in the reference's dispatch)
        return _capi.text_call(lib.wsr_snippet, self._h, C.byref(q), doc_id, n_passages)

    def GetDocument(self, doc_id: int) -> str:
        """The doc store's body text (ChunkedDocStoreReader::Get)."""
        return _capi.text_call(lib.wsr_doc_get, self._h, doc_id)

    def decode_block(self, list_id: int, block: int, which: int = 0):
        """Device decode of one block (test hook) -> list of values."""
        buf = (C.c_uint32 * 128)()
        cnt = C.c_int32()
        check(lib.wsr_debug_decode_block(self._h, list_id, block, which, buf, C.byref(cnt)))
        return list(buf[: cnt.value])


class DocsHost:
    """The snippet stage alone, without a device: the index dictionary and the doc
    store of a Vacuum dump (wsr_docs_*).  Same snippets as VacuumEngine's."""

    def __init__(self, engine_dir_path: str):
        h = C.c_void_p()
        check(lib.wsr_docs_open(engine_dir_path.encode(), C.byref(h)))
        self._h = h

    def close(self) -> None:
        if self._h is not None:
            lib.wsr_docs_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def query(self, terms: Sequence[str], is_phrase: bool = False, match_any: bool = False):
        q = _capi.Query()
        q.n_terms = len(terms)
        q.k = 1
        q.flags = _capi.QUERY_PHRASE if (is_phrase and len(terms) > 1) else 0
        if match_any:   # (a disjunctive query has no snippets: wsr_docs_snippet refuses it)
            q.flags |= _capi.QUERY_OR
        for i, t in enumerate(terms):
            lid, df = C.c_int32(), C.c_int32()
            check(lib.wsr_docs_lookup(self._h, t.encode(), C.byref(lid), C.byref(df)))
            q.list_ids[i] = lid.value
        return q

    def snippet(self, terms: Sequence[str], doc_id: int, n_passages: int = 3,
                is_phrase: bool = False) -> str:
        q = self.query(terms, is_phrase)
        return _capi.text_call(lib.wsr_docs_snippet, self._h, C.byref(q), doc_id, n_passages)

    def GetDocument(self, doc_id: int) -> str:
        return _capi.text_call(lib.wsr_docs_get, self._h, doc_id)


class ResidentBatch:
    """A query batch kept in HBM (wsr_batch_*): upload once, run many times."""

    def __init__(self, engine: VacuumEngine, max_queries: int, hit_stride: int):
        self.engine = engine
        self.stride = hit_stride
        b = C.c_void_p()
        check(lib.wsr_batch_create(engine._h, max_queries, hit_stride, C.byref(b)))
        self._b = b
        self.nq = 0
        # page-locked result arrays, reused by every fetch
        ph, pn = C.c_void_p(), C.c_void_p()
        check(lib.wsr_pinned_alloc(C.sizeof(_capi.Hit) * max(max_queries, 1) * hit_stride, C.byref(ph)))
        check(lib.wsr_pinned_alloc(4 * max(max_queries, 1), C.byref(pn)))
        self._pin = (ph, pn)
        self._hits = C.cast(ph, C.POINTER(_capi.Hit * (max(max_queries, 1) * hit_stride))).contents
        self._nh = C.cast(pn, C.POINTER(C.c_int32 * max(max_queries, 1))).contents

    def upload(self, queries) -> None:
        """queries: ctypes array of _capi.Query."""
        check(lib.wsr_batch_upload(self.engine._h, self._b, queries, len(queries)))
        self.nq = len(queries)

    def run(self) -> None:
        check(lib.wsr_batch_run(self.engine._h, self._b))

    def fetch(self):
        """-> (hits, n_hits): views of the batch's page-locked arrays, valid until
        the next fetch"""
        check(lib.wsr_batch_fetch(self.engine._h, self._b, self._hits, self._nh))
        return self._hits, self._nh

    def ready(self) -> bool:
        """True once the batch's last run has finished on the device."""
        rc = lib.wsr_batch_ready(self.engine._h, self._b)
        if rc < 0:
            check(rc)
        return rc == 1

    def wait_ready(self) -> None:
        """Spin until the batch's last run has finished (a host-side throttle)."""
        while not self.ready():
            pass

    def stats(self) -> _capi.BatchStats:
        st = _capi.BatchStats()
        check(lib.wsr_batch_stats_get(self.engine._h, self._b, C.byref(st)))
        return st

    def or_stats(self) -> _capi.OrStats:
        """Counters of the last run's disjunctive queries (wsr_batch_or_stats_get)."""
        st = _capi.OrStats()
        check(lib.wsr_batch_or_stats_get(self.engine._h, self._b, C.byref(st)))
        return st

    def launch_class(self) -> Dict[str, bool]:
        """wsr_debug_batch_class: the class flags of the last upload (they pick
        the kernel instances a run launches) and ran_conj / ran_gen of the last
        run, by name (_capi.CLASS_BITS).  Host state only."""
        f = C.c_uint32()
        check(lib.wsr_debug_batch_class(self.engine._h, self._b, C.byref(f)))
        return {name: bool(f.value & bit) for name, bit in _capi.CLASS_BITS.items()}

    def set_item_blocks(self, blocks: int) -> None:
        """wsr_batch_set_item_blocks (disjunctive queries: before the upload)."""
        check(lib.wsr_batch_set_item_blocks(self.engine._h, self._b, blocks))

    def close(self) -> None:
        if self._b is not None:
            lib.wsr_batch_destroy(self.engine._h, self._b)
            self._b = None
            for p in self._pin:
                lib.wsr_pinned_free(p)
            self._pin = ()


class Server:
    """Micro-batching front end (wsr_server_*): Search() may be called from many
    threads at once; concurrent calls are coalesced into GPU batches.  The
    analogue of the reference's gRPC workers sharing one engine
    (grpc_server_impl.h:260-263,382-389)."""

    def __init__(self, engine: VacuumEngine, max_batch: int = 4096, window_us: int = 200):
        self.engine = engine
        s = C.c_void_p()
        check(lib.wsr_server_open(engine._h, max_batch, window_us, C.byref(s)))
        self._s = s

    def Search(self, query: SearchQuery) -> SearchResult:
        q, freqs = self.engine.resolve(query)
        hits = (_capi.Hit * max(1, q.k))()
        n = C.c_int32()
        check(lib.wsr_server_search(self._s, C.byref(q), hits, C.byref(n)))
        r = SearchResult()
        if freqs is not None:
            r.doc_freqs = list(freqs)
            r.entries = [SearchResultEntry(hits[j].doc_id, hits[j].score) for j in range(n.value)]
        return r

    def bench(self, queries, n_clients: int = 16, depth: int = 256,
              seconds: float = 3.0) -> _capi.ServeStats:
        """closed-loop load: queries = ctypes array of _capi.Query"""
        st = _capi.ServeStats()
        check(lib.wsr_server_bench(self._s, queries, len(queries), n_clients, depth, seconds,
                                   C.byref(st)))
        return st

    def close(self) -> None:
        if self._s is not None:
            lib.wsr_server_close(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def image_size(index_dir: str, doc_range=None, positions: bool = False, bloom_factor: int = 0,
               threads: int = 0) -> Dict[str, int]:
    """HBM bytes per buffer of the image wsr_open would build for index_dir (or
    its doc range [lo, hi)), computed on the host without a device
    (wsr_image_size)."""
    lo, hi = doc_range or (0, 0)
    i = _capi.ImageInfo()
    check(lib.wsr_image_size(index_dir.encode(), lo, hi, 1 if positions else 0, bloom_factor, threads,
                             C.byref(i)))
    return {f: getattr(i, f) for f, _ in _capi.ImageInfo._fields_}


def sync(engine: VacuumEngine) -> None:
    check(lib.wsr_sync(engine._h))


# ---- index building (host only) -------------------------------------------
def build_from_linedoc(linedoc: str, out_dir: str, fmt: str = "WITH_POSITIONS",
                       n_rows: int = -1, bloom: Optional[Sequence] = None) -> _capi.BuildStats:
    """bloom = (ratio, expected_entries), e.g. (0.0009, 5): also write the
    two-way phrase bloom filters (flash_engine_dumper.h:412-525)."""
    st = _capi.BuildStats()
    if bloom:
        check(lib.wsr_build_from_linedoc_bloom(linedoc.encode(), n_rows, fmt.encode(),
                                               out_dir.encode(), float(bloom[0]), int(bloom[1]),
                                               C.byref(st)))
    else:
        check(lib.wsr_build_from_linedoc(linedoc.encode(), n_rows, fmt.encode(), out_dir.encode(),
                                         C.byref(st)))
    return st


def build_synthetic(out_dir: str, n_docs: int = 1_000_000, vocab: int = 500_000,
                    zipf_s: float = 1.07, seed: int = 0x5EED2026, with_positions: bool = True,
                    threads: int = 0) -> _capi.BuildStats:
    st = _capi.BuildStats()
    check(lib.wsr_build_synthetic(out_dir.encode(), n_docs, vocab, zipf_s, seed,
                                  1 if with_positions else 0, threads, C.byref(st)))
    return st


def build_wiki_standin(out_dir: str, n_docs: int = 5_500_000, term_scale: float = 1.0,
                       seed: int = 0x3C3C2026, threads: int = 0, topics: int = 0,
                       topics_per_term: int = 2, affinity: float = 0.6) -> _capi.BuildStats:
    """BASELINE configs[2] stand-in: df histogram of the reference's en-Wikipedia
    index (tools/gen_synthetic_log.py:8-16) x term_scale over n_docs docs.
    topics > 0: the topic-clustered variant (doc ids in `topics` contiguous
    ranges, every term under N/16 postings draws `affinity` of its docs from
    its topics_per_term home topics; the df histogram is unchanged)."""
    st = _capi.BuildStats()
    if topics > 0:
        check(lib.wsr_build_wiki_standin_topics(out_dir.encode(), n_docs, term_scale, seed, threads, topics,
                                                topics_per_term, affinity, C.byref(st)))
    else:
        check(lib.wsr_build_wiki_standin(out_dir.encode(), n_docs, term_scale, seed, threads,
                                         C.byref(st)))
    return st


def gen_two_term_log(index_dir: str, out_path: str, n_queries: int = 100_000, seed: int = 7) -> int:
    n = C.c_int64()
    check(lib.wsr_gen_two_term_log(index_dir.encode(), n_queries, seed, out_path.encode(),
                                   C.byref(n)))
    return n.value


def gen_mixed_log(index_dir: str, out_path: str, n_queries: int = 20_000, seed: int = 7) -> int:
    """1-5 term AND queries with the AOL term-count shares."""
    n = C.c_int64()
    check(lib.wsr_gen_mixed_log(index_dir.encode(), n_queries, seed, out_path.encode(),
                                C.byref(n)))
    return n.value


def gen_single_term_log(index_dir: str, out_path: str, high: bool, n_queries: int = 20_000, seed: int = 7) -> int:
    """Single-term queries of one df group (tools/gen_synthetic_log.py:171-189;
    run_exp.py:116-117's type_single.docfreq_high / _low)."""
    n = C.c_int64()
    check(lib.wsr_gen_single_term_log(index_dir.encode(), 1 if high else 0, n_queries, seed, out_path.encode(),
                                      C.byref(n)))
    return n.value


def gen_phrase_log(index_dir: str, out_path: str, n_queries: int = 10_000, seed: int = 7) -> int:
    """tools/gen_synthetic_log.py:254-265 over a synthetic index's phrase pool."""
    n = C.c_int64()
    check(lib.wsr_gen_phrase_log(index_dir.encode(), n_queries, seed, out_path.encode(),
                                 C.byref(n)))
    return n.value


def gen_realistic_log(index_dir: str, out_path: str, n_queries: int = 20_000, phrase_share: float = 0.1,
                      seed: int = 7) -> int:
    """One stream of the reference's mixed log (query_pool.h:363-375: quoted
    phrase lines among plain lines; run_exp.py's "type_realistic"): a share of
    two-term phrases from the index's phrase pool among 1-5-term AND queries
    (gen_mixed_log), interleaved in a seeded random order."""
    import os
    import random
    n_ph = int(round(n_queries * phrase_share))
    tmp_m, tmp_p = out_path + ".and.tmp", out_path + ".phr.tmp"
    gen_mixed_log(index_dir, tmp_m, n_queries=n_queries - n_ph, seed=seed)
    lines = open(tmp_m).read().splitlines()
    if n_ph:
        gen_phrase_log(index_dir, tmp_p, n_queries=n_ph, seed=seed + 1)
        lines += open(tmp_p).read().splitlines()
    for t in (tmp_m, tmp_p):
        if os.path.exists(t):
            os.remove(t)
    random.Random(seed).shuffle(lines)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return len(lines)


def class_order(queries) -> Tuple[List[int], int]:
    """wsr_class_order: a stable order of `queries` (a ctypes array of
    _capi.Query) with the conjunctive queries first, the phrase queries after
    them and the disjunctive ones last -> (order, n_conj).  Batches cut from it
    are class-pure."""
    n = len(queries)
    order = (C.c_int32 * max(n, 1))()
    nc = C.c_int32()
    check(lib.wsr_class_order(queries, n, order, C.byref(nc)))
    return list(order[:n]), nc.value


def class_batches(queries, batch: int) -> List[List[int]]:
    """The engine's batch former for a query stream: indices of `queries`
    (ctypes Query array) in batches of at most `batch`, each class cut
    separately (wsr_class_order), so no batch mixes phrase, conjunctive and
    disjunctive queries."""
    order, nc = class_order(queries)
    n_or = sum(1 for q in queries if q.flags & _capi.QUERY_OR)
    out = []
    for lo, hi in ((0, nc), (nc, len(order) - n_or), (len(order) - n_or, len(order))):
        for s in range(lo, hi, batch):
            out.append(order[s:min(s + batch, hi)])
    return out


def read_query_log(path: str):
    """-> [(terms, is_phrase)]: one query per line, a phrase in double quotes"""
    out = []
    for line in open(path).read().splitlines():
        line = line.strip()
        if not line:
            continue
        ph = len(line) >= 2 and line[0] == '"' and line[-1] == '"'
        out.append(((line[1:-1] if ph else line).split(), ph))
    return out
