"""semantic-indexer service: clean_documents_queue consumer + search HTTP API (port 8003).

Reference (semantic-indexer/indexer.py:11-143):
  * startup: load ``vector_store.faiss`` + ``metadata_store.pkl`` if both exist (resume),
    else build from the ``default_data`` CSVs and save;
  * consume clean documents (prefetch 1): ``text[i:i+500]`` chunks labelled
    ``"Dossier Patient {doc_id}"`` / ``"patient_file"``, add, save, ack;
  * ``add_to_index`` skips blank text.
Fixes, each covered by tests: the whole document is embedded in one packed GPU batch
instead of one encode per chunk; a batch is made durable by one append to a CRC-framed
write-ahead log (store/segment_log.py) and acked, the full snapshot pair is rewritten
only every ``INDEX_SNAPSHOT_EVERY`` batches (the reference rewrites O(N x d) bytes per
document), resume = snapshot + WAL replay; snapshots are atomic (temp + rename, index
before metadata) so a reader never sees mismatched lengths; one writer lock serialises index
mutation (multiple consumers are safe); the QA side shares the live index object in
process (no restart needed to see new documents); metadata ``doc_id`` is the real
document id.
HTTP (the endpoint the reference's synthese-comparative expects but nobody served,
synthese-comparative/core/retrieval_client.py:72-91):
  GET  /api/search/patient-snippets?patient_id&from_date&to_date&focus -> [{doc_id, text}]
  POST /api/search {"query", "k"} -> hits;  GET /api/index/stats;  GET /health
  DELETE /api/index/documents/{doc_id}, DELETE /api/index/patients/{patient_id}
    -> {"removed", "ntotal", "version"}: the patient-file chunks of that document / patient leave
    the index (FAISS remove_ids semantics: later row ids shift down; knowledge-base rows are
    never deleted this way); 404 nothing matches, 422 a sharded store, 503 no index
    optional search_mode dense | lexical | hybrid (default RETRIEVAL_MODE): kNN, BM25 or their
    reciprocal rank fusion; "score" is the leg's own (L2 distance, BM25 score, RRF value)
    optional search_type similarity | mmr (default RETRIEVAL_SEARCH_TYPE) with lambda_mult in
    [0, 1] (MMR_LAMBDA) and fetch_k (MMR_FETCH_K, clamped to k..64): LangChain's maximal
    marginal relevance over the first fetch_k hits of the mode, hits in pick order
    optional patient_id / from_date / to_date / include_knowledge_base scope the search to
    one patient's chunks (inside the window) plus, unless excluded, the knowledge base
"""
from __future__ import annotations

import json
import logging
import threading
import time
from pathlib import Path

import torch
from fastapi import FastAPI
from fastapi.responses import JSONResponse

from ..bus.broker import get_broker
from ..config import Settings, mmr_request
from ..index import faiss_io
from ..index.flat import FlatIndex, removal_mask  # noqa: F401  (FlatIndex: the default store type)
from ..index.hybrid import load_index, make_index
from ..index.lexical import LexicalColumns, fetch_depth
from ..index.scope import ScopeColumns, scope_request
from ..pipeline.corpus import embed_records
from ..schemas import SearchRequest
from ..store import metadata_io
from ..store.segment_log import DeleteFrame, SegmentLog, read_snapshot_marker, write_snapshot_marker
from ..text.chunking import chunk_chars
from ..text.dates import in_window, parse_date
from ..utils import tracing
from ..text.kb import kb_records_from_dir, synthetic_kb_records

logger = logging.getLogger("semantic-indexer")


class PatientIndex:
    """patient key -> its patient-file row ids, kept beside the append-only metadata list.

    ``/api/search/patient-snippets`` (the contract of synthese-comparative/core/
    retrieval_client.py:72-91) used to scan every metadata row under the index lock; at the
    10M-chunk scale of config 2 that stalls every search for seconds.  The map is updated
    by every ``add_records`` / WAL replay and rebuilt once from a loaded snapshot, so a
    lookup costs O(rows of that patient).  A row is reachable by its ``patient_id`` and by
    its ``doc_id`` (the reference keys patient chunks by document id)."""

    def __init__(self):
        self._rows: dict[str, list[int]] = {}
        self.n = 0          # metadata rows covered so far

    def extend(self, metadata: list[dict], start: int | None = None) -> None:
        start = self.n if start is None else start
        for i in range(start, len(metadata)):
            m = metadata[i]
            if m.get("type") != "patient_file":
                continue
            keys = {str(m.get("patient_id")), str(m.get("doc_id"))}
            for k in keys:
                self._rows.setdefault(k, []).append(i)
        self.n = max(self.n, len(metadata))

    def rebuild(self, metadata: list[dict]) -> None:
        self._rows, self.n = {}, 0
        self.extend(metadata, 0)

    def rows(self, key: str) -> list[int]:
        return list(self._rows.get(str(key), ()))


class SemanticIndexer:
    def __init__(self, encoder, tokenizer, settings: Settings | None = None, index: FlatIndex | None = None,
                 metadata: list | None = None, device: str = "cuda", on_indexed=None, on_deleted=None):
        self.st = settings or Settings()
        self.encoder = encoder
        self.tok = tokenizer
        self.device = device
        self.index = index
        self.metadata: list[dict] = metadata if metadata is not None else []
        self.patients = PatientIndex()
        self.patients.rebuild(self.metadata)
        self.scopes = ScopeColumns(device)     # row tags / days of the scoped search
        self.scopes.rebuild(self.metadata)
        # term columns of the lexical / hybrid search: built by the first such request
        # (ensure_lexical), at start-up with LEXICAL_INDEX=1; kept in step once they exist
        self.lexical: LexicalColumns | None = None
        self.lock = threading.RLock()
        self.on_indexed = on_indexed  # callback(doc_id) e.g. docs DB status -> INDEXED
        self.on_deleted = on_deleted  # callback(doc_id) e.g. docs DB status -> DELETED
        # a delete shifts row ids: odd while one is swapping the (index, metadata) pair, even
        # otherwise, and bumped inside the swap's critical section.  Readers that resolve ids
        # after a search without holding ``lock`` (pipeline/rag.py) compare it around their work
        self.generation = 0
        self._ch = None
        self._depth = None          # broker queue-depth probe (group commit), None: per message
        self._pending: list = []
        self.version = 0
        self.wal = SegmentLog(self.index_path.with_name(self.index_path.name + ".wal")) if self.st.index_wal else None
        self._batches_since_snapshot = 0

    # ------------------------------------------------------------------ paths
    @property
    def index_path(self) -> Path:
        return Path(self.st.index_dir) / self.st.index_file

    @property
    def meta_path(self) -> Path:
        return Path(self.st.index_dir) / self.st.metadata_file

    # ------------------------------------------------------------------ lifecycle
    @property
    def marker_path(self) -> Path:
        return self.index_path.with_name(self.index_path.name + ".snapshot.json")

    def startup(self, build_if_missing: bool = True) -> "SemanticIndexer":
        with self.lock:
            dirty = False
            covered = 0
            if self.index_path.exists() and self.meta_path.exists():
                self.index = load_index(self.st, self.index_path, self.device)
                self.metadata = metadata_io.read_metadata(self.meta_path)
                self.patients.rebuild(self.metadata)
                self.scopes.rebuild(self.metadata)
                self._lexical_rebuild()
                if len(self.metadata) != self.index.ntotal:
                    raise RuntimeError(f"index/metadata mismatch: {self.index.ntotal} vs {len(self.metadata)}")
                covered = read_snapshot_marker(self.marker_path)["wal_seq"]
                logger.info("resumed index (%d vectors)", self.index.ntotal)
            else:
                self.index = make_index(self.st, self.encoder.cfg.hidden, self.device)
                self.metadata = []
                self.patients.rebuild(self.metadata)
                self.scopes.rebuild(self.metadata)
                self._lexical_rebuild()
                if build_if_missing:
                    recs = kb_records_from_dir(self.st.default_data_dir) or synthetic_kb_records()
                    self.add_records(recs, log=False)
                    dirty = True
            if self.wal is not None:   # batches made durable after the last snapshot
                replayed = 0
                for _, recs, vecs in self.wal.replay(after_seq=covered):
                    if isinstance(recs, DeleteFrame):
                        self._check_delete_frame(recs)
                        self._apply_delete(recs["rows"])
                        replayed += len(recs["rows"])
                        continue
                    self.index.add(torch.from_numpy(vecs.copy()))
                    self.metadata.extend(recs)
                    self.patients.extend(self.metadata)
                    self.scopes.extend(self.metadata)
                    self._lexical_extend()
                    replayed += len(recs)
                if replayed:
                    logger.info("replayed %d added / removed vectors from the write-ahead log", replayed)
                    self.version += 1
                    dirty = True
            if dirty:
                self.save_state()
            if self.st.lexical_index:
                self.ensure_lexical()
        return self

    # ------------------------------------------------------------------ lexical columns
    def ensure_lexical(self) -> LexicalColumns:
        """The BM25 term columns of the metadata list, built on the first call."""
        with self.lock:
            if self.lexical is None:
                cols = LexicalColumns(self.device)
                cols.rebuild(self.metadata)
                self.lexical = cols
            return self.lexical

    def _lexical_extend(self) -> None:
        if self.lexical is not None:
            self.lexical.extend(self.metadata)

    def _lexical_rebuild(self) -> None:
        if self.lexical is not None:
            self.lexical.rebuild(self.metadata)

    def save_state(self) -> None:
        with self.lock:
            Path(self.st.index_dir).mkdir(parents=True, exist_ok=True)
            self.index.save(self.index_path)            # atomic
            metadata_io.write_metadata(self.meta_path, self.metadata)  # atomic
            if self.wal is not None:                    # snapshot covers the whole log
                seq = self.wal.last_seq
                write_snapshot_marker(self.marker_path, seq, self.index.ntotal)
                self.wal.reset(seq)
            self._batches_since_snapshot = 0

    def commit(self) -> None:
        """Make the batches indexed so far durable: a WAL append already did; take a
        full snapshot every ``snapshot_every`` batches (always, without a WAL)."""
        self._batches_since_snapshot += 1
        if self.wal is None or self._batches_since_snapshot >= self.st.snapshot_every:
            self.save_state()

    # ------------------------------------------------------------------ mutation
    def add_records(self, records: list[dict], log: bool = True) -> int:
        recs = [r for r in records if r.get("text_content", "").strip()]
        if not recs:
            return 0
        with tracing.span("indexer.embed", chunks=len(recs)):
            emb = embed_records(self.encoder, self.tok, recs)
        with self.lock:
            if self.index is None:
                self.index = make_index(self.st, self.encoder.cfg.hidden, self.device)
            if log and self.wal is not None:           # durable before it is visible
                self.wal.append(recs, emb.float().cpu().numpy())
            self.index.add(emb)
            self.metadata.extend(recs)
            self.patients.extend(self.metadata)
            self.scopes.extend(self.metadata)
            self._lexical_extend()
            self.version += 1
        return len(recs)

    def add_to_index(self, text: str, source_name: str, doc_type: str = "knowledge_base", doc_id: str = "KB") -> bool:
        """Reference-compatible single add (blank text skipped)."""
        return self.add_records([{"doc_id": doc_id, "text_content": text, "source": source_name,
                                  "type": doc_type}]) == 1

    def index_document(self, doc_id, text: str, metadata: dict | None = None) -> int:
        md = metadata or {}
        recs = [{"doc_id": str(doc_id), "text_content": c, "source": f"Dossier Patient {doc_id}",
                 "type": "patient_file", "patient_id": md.get("patient_id", str(doc_id)),
                 "filename": md.get("filename"), "note_date": parse_date(md.get("note_date"))}
                for c in chunk_chars(text or "", self.st.chunk_size)]
        return self.add_records(recs)

    # ------------------------------------------------------------------ deletion
    def delete_document(self, doc_id) -> int:
        """Remove every chunk of the patient document ``doc_id``; returns the rows removed."""
        return self._delete("doc_id", doc_id)

    def delete_patient(self, patient_id) -> int:
        """Remove every chunk of every document of ``patient_id`` (erasure on request)."""
        return self._delete("patient_id", patient_id)

    def _delete(self, field: str, key) -> int:
        """FAISS ``remove_ids`` semantics (surviving rows keep their order, later ids shift
        down) for the ``patient_file`` rows whose ``field`` is ``key``; knowledge-base rows are
        never deleted this way.  No matching row: 0, nothing logged.  Otherwise, under the
        writer lock: the WAL frame first (durable before visible), then vectors, metadata,
        scope / lexical columns and the patient map swapped together under the index lock."""
        key = str(key)
        with self.lock:
            if self.index is None:
                return 0
            meta = self.metadata
            rows = sorted(i for i in set(self.patients.rows(key))
                          if meta[i].get("type") == "patient_file" and str(meta[i].get(field)) == key)
            if not rows:
                return 0
            if not getattr(self.index, "can_remove", True):
                self.index.remove_ids(rows)                # a sharded store: raises NotImplementedError
            if self.wal is not None:                       # durable before it is visible
                self.wal.append_delete(field, [key], rows, self.index.ntotal)
            self._apply_delete(rows)
            self.version += 1
            self.commit()
        logger.info("deleted %s=%s (%d chunks)", field, key, len(rows))
        return len(rows)

    def _check_delete_frame(self, frame: DeleteFrame) -> None:
        rows, field, keys = frame["rows"], frame["field"], set(frame["keys"])
        n = self.index.ntotal
        if frame["ntotal_before"] != n or len(self.metadata) != n:
            raise RuntimeError(f"delete frame expects {frame['ntotal_before']} rows, the index holds {n} "
                               f"({len(self.metadata)} records)")
        for i in rows:
            m = self.metadata[i] if 0 <= i < n else {}
            if m.get("type") != "patient_file" or str(m.get(field)) not in keys:
                raise RuntimeError(f"delete frame names row {i}, which does not carry {field} in {sorted(keys)}")

    def _apply_delete(self, rows: list[int]) -> None:
        """Rows ``rows`` (ascending, unique, valid) leave the index, the metadata list (in place:
        the QA side shares the list object), the columns and the patient map in one swap."""
        n = self.index.ntotal
        keep, pos, removed = removal_mask(rows, n, self.index.device)
        gone = [self.metadata[i] for i in rows]

        if removed != len(rows):
            raise RuntimeError("delete: the rows named are not unique rows of the index")

        def swap():
            # everything that can fail -- the checks, the new device buffers -- comes first and
            # changes nothing; from the bump on there are only list surgery and reference swaps
            commit_scopes = self.scopes.prepare_remove(keep, pos, n - removed)
            commit_lexical = (self.lexical.prepare_remove(keep, pos, n - removed, gone)
                              if self.lexical is not None else None)
            self.generation += 1                           # odd: ids and records are changing
            metadata_io.drop_rows(self.metadata, rows)
            commit_scopes()
            if commit_lexical is not None:
                commit_lexical()
            self.patients.rebuild(self.metadata)

        def swapped():                                     # last statement under the index lock
            self.generation += 1

        try:
            self.index.remove_ids(rows, before_swap=swap, after_swap=swapped, mask=(keep, pos, removed))
        finally:
            if self.generation & 1:                        # the swap itself failed half-way
                self.generation += 1

    # ------------------------------------------------------------------ queue
    def callback(self, ch, method, properties, body):
        """Queue consumer (reference semantics: chunk, embed, persist, then ack).

        Adaptive group commit: while more clean documents are already waiting in the
        queue (up to ``BATCH_DOCS``), messages are only collected; the batch is then
        embedded in one packed encoder forward, persisted with ONE atomic snapshot and
        acked together.  An idle queue flushes at once, so single-document latency is
        unchanged; a burst no longer pays one index snapshot per document."""
        self._pending.append((ch, method, body))
        waiting = self._depth(self.st.clean_queue) if self._depth is not None else 0
        if waiting > 0 and len(self._pending) < self.BATCH_DOCS:
            return
        batch, self._pending = self._pending, []
        recs, done, deleted = [], [], False
        for c, m, b in batch:
            try:
                msg = json.loads(b)
                doc_id = msg.get("doc_id")
                if msg.get("op") == "delete":
                    # order on the queue is order in the index: the adds collected so far first
                    if done:
                        self._flush_adds(recs, done)
                        recs, done = [], []
                    self._delete_message(c, m, doc_id)
                    deleted = True
                    continue
                md = msg.get("metadata") or {}
                recs.extend({"doc_id": str(doc_id), "text_content": chunk, "source": f"Dossier Patient {doc_id}",
                             "type": "patient_file", "patient_id": md.get("patient_id", str(doc_id)),
                             "filename": md.get("filename"), "note_date": parse_date(md.get("note_date"))}
                            for chunk in chunk_chars(msg.get("original_text_masked", "") or "", self.st.chunk_size))
                done.append((c, m, doc_id))
            except Exception as e:  # noqa: BLE001 - malformed message: dead-letter it
                logger.error("indexing error: %s", e)
                c.basic_nack(delivery_tag=m.delivery_tag, requeue=False)
        if done or not deleted:
            self._flush_adds(recs, done)

    def _flush_adds(self, recs: list, done: list) -> None:
        try:
            n = self.add_records(recs)
            self.commit()
        except Exception as e:  # noqa: BLE001
            logger.error("indexing error: %s", e)
            for c, m, _ in done:
                c.basic_nack(delivery_tag=m.delivery_tag, requeue=False)
            return
        for c, m, doc_id in done:
            c.basic_ack(delivery_tag=m.delivery_tag)
            if self.on_indexed is not None and isinstance(doc_id, int):
                self.on_indexed(doc_id)
        logger.info("indexed %d doc(s) (%d chunks)", len(done), n)

    def _delete_message(self, c, m, doc_id) -> None:
        try:
            self.delete_document(doc_id)
        except Exception as e:  # noqa: BLE001
            logger.error("delete error: %s", e)
            c.basic_nack(delivery_tag=m.delivery_tag, requeue=False)
            return
        c.basic_ack(delivery_tag=m.delivery_tag)
        if self.on_deleted is not None and isinstance(doc_id, int):
            self.on_deleted(doc_id)

    BATCH_DOCS = 64

    def start_consumer(self, broker=None) -> threading.Thread:
        broker = broker or get_broker(self.st)
        ch = broker.channel()
        self._ch = ch
        self._depth = getattr(broker, "depth", None)
        ch.queue_declare(queue=self.st.clean_queue, durable=True)
        ch.basic_qos(prefetch_count=self.BATCH_DOCS if self._depth is not None else 1)
        ch.basic_consume(queue=self.st.clean_queue, on_message_callback=self.callback)
        t = threading.Thread(target=ch.start_consuming, name="indexer-consumer", daemon=True)
        t.start()
        return t

    def stop_consumer(self) -> None:
        if self._ch is not None:
            self._ch.stop_consuming()

    # ------------------------------------------------------------------ query
    @torch.inference_mode()
    def search(self, query: str, k: int = 3, scope: dict | None = None, mode: str | None = None,
               mmr: tuple | None = None) -> list[dict]:
        """``scope``: None, or a scope request (index/scope.py ``scope_request``) -- the hits
        then come from that patient / window (and the knowledge base unless excluded) only.
        ``mode``: None / ``"dense"`` (the kNN search, ``score`` = L2 distance), ``"lexical"``
        (BM25, ``score`` = BM25 score) or ``"hybrid"`` (reciprocal rank fusion of both at depth
        ``HYBRID_FETCH_K``, ``score`` = RRF value).  ``mmr``: None or ``(lambda_mult, fetch_k)``
        -- the k hits are re-selected for diversity (``ops.mmr_select``) out of the mode's first
        ``fetch_k`` (clamped to k..64), in pick order, ``score`` still the mode's own."""
        # the lexical mode uses the embedding only for the MMR relevance term
        q = (None if mode == "lexical" and mmr is None
             else self.encoder.encode(self.tok.encode_batch([query])))
        with self.lock:
            if mmr is not None:
                D, I = self._search_mmr(q, query, k, scope, mode, mmr)
            elif mode is not None and mode != "dense":
                D, I = self._search_mode(q, query, k, scope, mode)
            elif scope is None:
                D, I = self.index.search(q, k)
            else:
                D, I = self.index.search_scoped(q, k, self.scopes, self.scopes.scope_rows([scope]))
            dl, il = D[0].tolist(), I[0].tolist()
            # a sharded index: surface a failed cross-rank gather (stale peer rows) after the
            # host sync above instead of serving it (index/sharded.py check_gather)
            check = getattr(self.index, "check_gather", None)
            if check is not None:
                check()
            out = []
            for d, i in zip(dl, il):
                if 0 <= i < len(self.metadata):
                    m = self.metadata[i]
                    out.append({"id": i, "score": d, "text": m.get("text_content", ""), "source": m.get("source"),
                                "type": m.get("type"), "doc_id": str(m.get("doc_id"))})
            return out

    def _search_mmr(self, q, query: str, k: int, scope, mode, mmr):
        """The mode's first ``fetch_k`` hits, then one ``mmr_select`` launch picks k of them;
        D = the mode's score of each pick."""
        if not 1 <= k <= 64:
            raise ValueError("mmr search serves k in 1..64")
        lam, fk = float(mmr[0]), min(64, max(k, int(mmr[1])))
        if mode is not None and mode != "dense":
            Dc, C = self._search_mode(q, query, fk, scope, mode, base_k=k)
        elif scope is None:
            Dc, C = self.index.search(q, fk)
        else:
            Dc, C = self.index.search_scoped(q, fk, self.scopes, self.scopes.scope_rows([scope]))
        dev = C.device
        _, I, P = self.index.mmr_select(q, C, torch.full((1,), fk, dtype=torch.int32, device=dev),
                                        torch.full((1,), lam, dtype=torch.float32, device=dev), k)
        return torch.gather(Dc, 1, P.clamp(min=0).long()), I

    def _search_mode(self, q, query: str, k: int, scope, mode: str, base_k: int | None = None):
        from .. import ops

        if mode not in ("lexical", "hybrid"):
            raise ValueError(f"search mode must be dense, lexical or hybrid, got {mode!r}")
        if not 1 <= k <= 64:
            raise ValueError("lexical / hybrid search serves k in 1..64")
        lex = self.ensure_lexical()
        cols, rows = (self.scopes, self.scopes.scope_rows([scope])) if scope is not None else (None, None)
        qt, qw, avgdl = lex.query_rows([query])
        if mode == "lexical":
            return self.index.search_lexical(lex, qt, qw, avgdl, k, scope_cols=cols, scope=rows)
        # under MMR k is fetch_k: the legs run at max(fetch_depth(k of the request), fetch_k)
        depth = fetch_depth(k) if base_k is None else max(fetch_depth(base_k), k)
        _, Id = self.index.search(q, depth) if scope is None else self.index.search_scoped(q, depth, cols, rows)
        _, Il = self.index.search_lexical(lex, qt, qw, avgdl, depth, scope_cols=cols, scope=rows)
        return ops.rank_fuse(Id, Il, torch.full((1,), 2, dtype=torch.int32, device=Id.device), k)

    def patient_snippets(self, patient_id: str, from_date=None, to_date=None, focus=None, limit: int = 20) -> list[dict]:
        """The patient's chunks, optionally restricted to notes dated in [from_date, to_date]
        (each chunk's ``note_date``, set at ingest: text/dates.py) and ranked by distance to
        the ``focus`` text."""
        pid = str(patient_id)
        lo, hi = parse_date(from_date), parse_date(to_date)
        # row ids are positions and a delete shifts them: the id list, the records and the
        # vectors are read under ONE hold of the lock (the focus is embedded before it)
        q = self.encoder.encode(self.tok.encode_batch([focus])) if focus else None
        xb = None
        with self.lock:   # O(rows of this patient): the per-patient map, never a metadata scan
            meta = self.metadata
            rows = [(i, meta[i]) for i in self.patients.rows(pid) if in_window(meta[i].get("note_date"), lo, hi)]
            if q is not None and rows:
                ids = torch.tensor([i for i, _ in rows], device=self.index.xb.device)
                xb = self.index.xb.index_select(0, ids).float()
        if xb is not None:
            d = ((xb - q.to(xb.device)) ** 2).sum(1)
            order = d.argsort().tolist()
            rows = [rows[j] for j in order]
        return [{"doc_id": str(m.get("doc_id")), "text": m.get("text_content", "")} for _, m in rows[:limit]]


def create_app(indexer: SemanticIndexer) -> FastAPI:
    app = FastAPI(title="Semantic Indexer (MI355X)")
    app.state.indexer = indexer

    @app.get("/health")
    def health():
        return {"status": "ok", "service": "semantic-indexer"}

    @app.get("/debug/trace")
    def trace_dump():
        return tracing.chrome_trace()

    @app.get("/api/index/stats")
    def stats():
        idx = indexer.index
        return {"ntotal": idx.ntotal if idx is not None else 0, "dim": idx.d if idx is not None else None,
                "metric": idx.metric if idx is not None else None, "version": indexer.version,
                "lexical": indexer.lexical.stats() if indexer.lexical is not None else None}

    @app.post("/api/search")
    def search(req: SearchRequest):
        if indexer.index is None:
            return JSONResponse(status_code=503, content={"detail": "Index non chargé."})
        try:
            scope = scope_request(req.patient_id, req.from_date, req.to_date, req.include_knowledge_base)
        except ValueError as e:
            return JSONResponse(status_code=422, content={"detail": str(e)})
        mode = req.search_mode or indexer.st.retrieval_mode
        try:
            mmr = mmr_request(req.search_type, req.lambda_mult, req.fetch_k, indexer.st)
        except ValueError as e:
            return JSONResponse(status_code=422, content={"detail": str(e)})
        if mode != "dense" or mmr is not None:
            try:
                return indexer.search(req.query, req.k, scope, mode, mmr)
            except (ValueError, NotImplementedError) as e:
                return JSONResponse(status_code=422, content={"detail": str(e)})
        if scope is None:
            return indexer.search(req.query, req.k)
        return indexer.search(req.query, req.k, scope)

    def _delete(fn, key):
        if indexer.index is None:
            return JSONResponse(status_code=503, content={"detail": "Index non chargé."})
        try:
            removed = fn(key)
        except NotImplementedError as e:
            return JSONResponse(status_code=422, content={"detail": str(e)})
        if not removed:
            return JSONResponse(status_code=404, content={"detail": "No indexed chunk matches"})
        return {"removed": removed, "ntotal": indexer.index.ntotal, "version": indexer.version}

    @app.delete("/api/index/documents/{doc_id}")
    def delete_document(doc_id: str):
        return _delete(indexer.delete_document, doc_id)

    @app.delete("/api/index/patients/{patient_id}")
    def delete_patient(patient_id: str):
        return _delete(indexer.delete_patient, patient_id)

    @app.get("/api/search/patient-snippets")
    def patient_snippets(patient_id: str, from_date: str | None = None, to_date: str | None = None,
                         focus: str | None = None):
        return indexer.patient_snippets(patient_id, from_date, to_date, focus)

    return app
