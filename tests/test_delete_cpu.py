"""Document deletion on the CPU (reference ops): write-ahead-log delete frames, the indexer's
``delete_document`` / ``delete_patient``, restart replay, the follower, the queue message, the
HTTP routes of the three services, and the RAG pipeline's generation check.
"""
from __future__ import annotations

import json

import httpx
import numpy as np
import pytest
import torch

from docqa_amd.store import docs_db
from docqa_amd.store.segment_log import MAGIC, DeleteFrame, SegmentLog, tail_frames

WORD = "zorglubine"


# ------------------------------------------------------------------ reference ops, list surgery
def test_reference_ops_against_numpy():
    from docqa_amd import ops

    rng = np.random.default_rng(0)
    for n in (0, 1, 7, 300):
        keep = (rng.random(n) < 0.6).astype(np.uint8)
        lens = rng.integers(0, 5, size=n).astype(np.int64)
        k, w = torch.from_numpy(keep), torch.from_numpy(lens)
        pos, epos = ops.masked_scan(k), ops.masked_scan(k, w)
        assert pos.tolist() == [0] + np.cumsum(keep != 0).tolist()
        assert epos.tolist() == [0] + np.cumsum(np.where(keep != 0, lens, 0)).tolist()
        src = torch.from_numpy(rng.integers(0, 99, size=(n, 3)))
        assert torch.equal(ops.gather_rows(src, k, pos, int(pos[-1])), src[k.bool()])
        row_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))
        E = int(row_ptr[-1])
        terms, tfs = torch.arange(E, dtype=torch.int32), (torch.arange(E) % 200).to(torch.uint8)
        p2, t2, f2 = ops.csr_gather(row_ptr, k, pos, epos, terms, tfs, int(pos[-1]), int(epos[-1]))
        esel = np.repeat(keep != 0, lens)
        assert p2.tolist() == [0] + np.cumsum(lens[keep != 0]).tolist()
        assert t2.tolist() == terms.numpy()[esel].tolist() and f2.tolist() == tfs.numpy()[esel].tolist()
        ids = torch.from_numpy(np.nonzero(keep)[0].astype(np.int64))
        assert ops.remap_ids(ids, pos).tolist() == list(range(ids.numel()))


def test_drop_rows_in_place_by_runs():
    from docqa_amd.store.metadata_io import drop_rows

    for rows in ([], [0], [9], [0, 1, 2], [3, 4, 7, 8, 9], [0, 2, 4, 6, 8], list(range(10))):
        lst = list(range(10))
        same = lst
        drop_rows(lst, rows)
        assert lst is same and lst == [i for i in range(10) if i not in rows]
    lst = list(range(1000))                              # a scattered delete: one pass, still in place
    same, rows = lst, list(range(0, 1000, 3))
    drop_rows(lst, rows)
    assert lst is same and lst == [i for i in range(1000) if i % 3]


# ------------------------------------------------------------------ delete frames
def _vecs(n, d=4, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def test_delete_frame_round_trip_and_interleaving(tmp_path):
    log = SegmentLog(tmp_path / "x.wal", fsync=False)
    a, b = [{"doc_id": "1", "text_content": "a"}], [{"doc_id": "2", "text_content": "b"}, {"doc_id": "2", "text_content": "c"}]
    assert log.append(a, _vecs(1)) == 1
    second = (tmp_path / "x.wal").stat().st_size
    assert log.append_delete("doc_id", [1], [0], 1) == 2
    assert log.append(b, _vecs(2, seed=1)) == 3
    assert log.append_delete("patient_id", ["P"], [0, 1], 2) == 4
    log.close()
    with pytest.raises(ValueError):
        log.append_delete("source", ["x"], [0], 1)
    log.close()

    again = SegmentLog(tmp_path / "x.wal", fsync=False)
    frames = list(again.replay())
    assert [f[0] for f in frames] == [1, 2, 3, 4] and again.last_seq == 4
    assert frames[0][1] == a and np.array_equal(frames[0][2], _vecs(1))            # the add tuple is unchanged
    assert isinstance(frames[1][1], DeleteFrame) and frames[1][2] is None
    assert frames[1][1] == {"field": "doc_id", "keys": ["1"], "rows": [0], "ntotal_before": 1}
    assert frames[3][1] == {"field": "patient_id", "keys": ["P"], "rows": [0, 1], "ntotal_before": 2}
    assert [f[0] for f in again.replay(after_seq=2)] == [3, 4]
    tailed, off = tail_frames(tmp_path / "x.wal", 0)
    assert [f[0] for f in tailed] == [1, 2, 3, 4] and off == (tmp_path / "x.wal").stat().st_size
    assert isinstance(tailed[3][1], DeleteFrame) and tail_frames(tmp_path / "x.wal", off) == ([], off)
    # its own magic: a reader that only knows add frames stops there instead of misreading it
    raw = (tmp_path / "x.wal").read_bytes()
    assert int.from_bytes(raw[:4], "little") == MAGIC
    assert raw[second:second + 4] == b"DQD1" and int.from_bytes(raw[second:second + 4], "little") != MAGIC


@pytest.mark.parametrize("kind", ["add", "delete"])
def test_torn_frame_is_truncated(tmp_path, kind):
    p = tmp_path / "t.wal"
    log = SegmentLog(p, fsync=False)
    log.append([{"doc_id": "1", "text_content": "a"}], _vecs(1))
    log.append_delete("doc_id", ["1"], [0], 1)
    good = p.stat().st_size
    if kind == "add":
        log.append([{"doc_id": "2", "text_content": "b"}], _vecs(1))
    else:
        log.append_delete("doc_id", ["2"], [0, 1, 2], 3)
    log.close()
    whole = p.read_bytes()
    for cut in (len(whole) - 1, good + 10):                  # torn inside the payload, inside the header
        p.write_bytes(whole[:cut])
        tailed, off = tail_frames(p, 0)                      # a tail never truncates
        assert [f[0] for f in tailed] == [1, 2] and off == good and p.stat().st_size == cut
        r = SegmentLog(p, fsync=False)
        assert [f[0] for f in r.replay()] == [1, 2]
        assert p.stat().st_size == good and r.last_seq == 2
    flipped = bytearray(whole)
    flipped[-1] ^= 0xFF                                       # CRC mismatch
    p.write_bytes(bytes(flipped))
    assert [f[0] for f in SegmentLog(p, fsync=False).replay()] == [1, 2] and p.stat().st_size == good


# ------------------------------------------------------------------ indexer
def _settings(d, snapshot_every=100):
    from docqa_amd.config import Settings

    st = Settings()
    st.index_dir = str(d)
    st.default_data_dir = str(d / "nodata")
    st.snapshot_every = snapshot_every
    return st


@pytest.fixture(scope="module")
def encoder():
    from docqa_amd.models.bert import BertConfig, BertEncoder

    return BertEncoder(BertConfig.preset("tiny-bert"), device="cpu")


def _indexer(d, encoder, **kw):
    from docqa_amd.services.indexer import SemanticIndexer
    from docqa_amd.text.tokenizer import WordPieceTokenizer

    return SemanticIndexer(encoder, WordPieceTokenizer(), _settings(d), device="cpu", **kw).startup()


def _fill(ix):
    for pid in ("A", "B"):
        for j in range(3):
            extra = f" Traitement par {WORD} 5 mg." if (pid, j) == ("B", 1) else ""
            ix.index_document(f"{pid}{j}", f"Note {j} du patient {pid} : tension stable, bilan normal.{extra} " * 12,
                              {"patient_id": pid, "note_date": f"2024-01-{j + 1:02d}"})


def _state(ix):
    return (ix.index.xb.clone(), [dict(m) for m in ix.metadata], ix.scopes.days.clone(),
            {k: list(v) for k, v in ix.patients._rows.items() if v})


def _all_modes(ix, query, k=50):
    out = []
    for mode in (None, "lexical", "hybrid"):
        for scope in (None, {"patient_id": "B", "from_date": None, "to_date": None, "include_knowledge_base": True}):
            out += ix.search(query, k=min(k, 64), scope=scope, mode=mode)
        out += ix.search(query, k=5, mode=mode, mmr=(0.5, 20))
    return out


def test_delete_document_and_patient(tmp_path, encoder):
    from docqa_amd.index.lexical import LexicalColumns

    ix = _indexer(tmp_path, encoder)
    kb = sum(m["type"] != "patient_file" for m in ix.metadata)
    assert kb > 0
    _fill(ix)
    ix.ensure_lexical()
    meta_list, n0, v0 = ix.metadata, ix.index.ntotal, ix.version
    assert any(h["doc_id"] == "B1" for h in ix.search(WORD, k=3, mode="lexical"))
    b1 = [i for i, m in enumerate(ix.metadata) if m["doc_id"] == "B1"]
    assert len(b1) > 1 and ix.delete_document("nope") == 0 and ix.version == v0 and ix.wal.last_seq > 0
    seq = ix.wal.last_seq

    assert ix.delete_document("B1") == len(b1)
    assert ix.wal.last_seq == seq + 1 and ix.version == v0 + 1 and ix.generation % 2 == 0 and ix.generation > 0
    assert ix.metadata is meta_list and len(meta_list) == ix.index.ntotal == n0 - len(b1)
    assert ix.scopes.n == ix.lexical.n == ix.patients.n == ix.index.ntotal
    assert not any(h["doc_id"] == "B1" for h in _all_modes(ix, f"patient B {WORD}"))
    assert ix.search(WORD, k=3, mode="lexical") == []                   # df fell to 0 with its only row
    fresh = LexicalColumns("cpu")
    fresh.rebuild(ix.metadata)
    assert fresh.df == ix.lexical.df and torch.equal(fresh.terms, ix.lexical.terms)
    assert ix.patients.rows("B1") == [] and ix.patient_snippets("B", focus="tension")
    assert all(ix.metadata[i]["patient_id"] == "B" for i in ix.patients.rows("B"))
    assert ix.delete_document("B1") == 0

    # a patient: every document of theirs, and only theirs
    nb = len(ix.patients.rows("B"))
    assert ix.delete_patient("B") == nb and ix.patients.rows("B") == [] and ix.patient_snippets("B") == []
    assert not any(h["doc_id"].startswith("B") for h in _all_modes(ix, "patient B tension"))
    assert {m["doc_id"] for m in ix.metadata if m["type"] == "patient_file"} == {"A0", "A1", "A2"}

    # the knowledge base is protected: its doc_id names no patient file
    assert ix.delete_document("KB") == 0 and ix.delete_patient("KB") == 0 and ix.delete_patient("None") == 0
    assert sum(m["type"] != "patient_file" for m in ix.metadata) == kb

    # after the deletes the store keeps following adds
    ix.index_document("C0", f"Reprise de la {WORD}.", {"patient_id": "C"})
    assert [h["doc_id"] for h in ix.search(WORD, k=3, mode="lexical")] == ["C0"]


def test_restart_replays_add_delete_add(tmp_path, encoder):
    ix = _indexer(tmp_path, encoder)
    ix.save_state()                                     # the knowledge base is in the snapshot
    _fill(ix)                                           # WAL: adds ...
    assert ix.delete_document("A1") > 0                 # ... a delete ...
    ix.index_document("C0", "Une note de plus.", {"patient_id": "C"})   # ... an add
    assert ix.delete_patient("B") > 0
    want = _state(ix)
    ix.wal.close()

    back = _indexer(tmp_path, encoder)
    got = _state(back)
    assert torch.equal(got[0], want[0]) and got[1] == want[1] and torch.equal(got[2], want[2]) and got[3] == want[3]
    assert back.index.ntotal == len(back.metadata)
    back.wal.close()
    # the replay took a snapshot: a third start loads it without any frame
    third = _indexer(tmp_path, encoder)
    assert torch.equal(_state(third)[0], want[0]) and _state(third)[1] == want[1]


def test_replay_with_wrong_ntotal_before_raises(tmp_path, encoder):
    ix = _indexer(tmp_path, encoder)
    ix.save_state()
    _fill(ix)
    rows = ix.patients.rows("A1")
    ix.wal.append_delete("doc_id", ["A1"], rows, ix.index.ntotal + 1)
    ix.wal.close()
    with pytest.raises(RuntimeError, match="delete frame"):
        _indexer(tmp_path, encoder)


def test_replay_with_rows_of_another_document_raises(tmp_path, encoder):
    ix = _indexer(tmp_path, encoder)
    ix.save_state()
    _fill(ix)
    ix.wal.append_delete("doc_id", ["A1"], ix.patients.rows("A2"), ix.index.ntotal)
    ix.wal.close()
    with pytest.raises(RuntimeError, match="does not carry"):
        _indexer(tmp_path, encoder)


def test_follower_applies_deletes(tmp_path, encoder):
    from docqa_amd.index.follower import IndexFollower

    w = _indexer(tmp_path, encoder)
    w.save_state()
    f = IndexFollower(str(tmp_path), d=encoder.cfg.hidden, device="cpu")
    f.poll()
    f.ensure_lexical()
    _fill(w)
    assert f.poll() == len(w.metadata) - sum(m["type"] != "patient_file" for m in w.metadata)
    g0, v0, meta_list = f.generation, f.version, f.metadata
    w.delete_document("A1")
    w.index_document("C0", "Une note de plus.", {"patient_id": "C"})
    w.delete_patient("B")
    assert f.poll() == 1
    assert f.metadata is meta_list and f.metadata == w.metadata and torch.equal(f.index.xb, w.index.xb)
    assert f.generation == g0 + 4 and f.version == v0 + 1
    assert f.scopes.n == f.lexical.n == f.index.ntotal and torch.equal(f.scopes.days, w.scopes.days)
    w.ensure_lexical()
    assert f.lexical.df == w.lexical.df and torch.equal(f.lexical.row_ptr, w.lexical.row_ptr)
    w.delete_document("A0")
    w.save_state()                                      # a snapshot after a delete: an ordinary reload
    f.poll()
    assert f.metadata == w.metadata and torch.equal(f.index.xb, w.index.xb)


# ------------------------------------------------------------------ queue
class _Channel:
    def __init__(self):
        self.acked, self.nacked = [], []

    def basic_ack(self, delivery_tag):
        self.acked.append(delivery_tag)

    def basic_nack(self, delivery_tag, requeue=False):
        self.nacked.append(delivery_tag)


class _Method:
    def __init__(self, tag):
        self.delivery_tag = tag


def test_queue_add_then_delete_in_one_batch(tmp_path, encoder):
    indexed, deleted = [], []
    ix = _indexer(tmp_path, encoder, on_indexed=indexed.append, on_deleted=deleted.append)
    ch = _Channel()
    waiting = [2, 1, 0]                                 # the queue depth the consumer sees per message
    ix._depth = lambda q: waiting.pop(0)

    def add(doc_id, text):
        return json.dumps({"doc_id": doc_id, "original_text_masked": text, "metadata": {"patient_id": "Q"}}).encode()

    ix.callback(ch, _Method(1), None, add(41, f"Note avec {WORD}."))
    ix.callback(ch, _Method(2), None, json.dumps({"op": "delete", "doc_id": 41}).encode())
    assert ch.acked == [] and ix.patients.rows("41") == []           # still collecting the batch
    ix.callback(ch, _Method(3), None, add(42, "Une autre note."))
    assert ch.acked == [1, 2, 3] and ch.nacked == []
    assert indexed == [41, 42] and deleted == [41]
    # the add was applied before its delete (the other order would have left document 41 indexed)
    assert ix.patients.rows("41") == [] and len(ix.patients.rows("42")) == 1
    frames = list(SegmentLog(ix.wal.path, fsync=False).replay())
    kinds = ["delete" if isinstance(f[1], DeleteFrame) else "add" for f in frames]
    assert kinds[-3:] == ["add", "delete", "add"]
    # a delete of something that is not indexed is acknowledged too
    ix._depth = lambda q: 0
    ix.callback(ch, _Method(4), None, json.dumps({"op": "delete", "doc_id": 99}).encode())
    assert ch.acked[-1] == 4 and deleted == [41, 99]


# ------------------------------------------------------------------ HTTP: indexer
def test_indexer_routes(tmp_path, encoder):
    from fastapi.testclient import TestClient

    from docqa_amd.index.sharded import ShardedIndex
    from docqa_amd.services.indexer import create_app

    ix = _indexer(tmp_path, encoder)
    _fill(ix)
    c = TestClient(create_app(ix))
    n = ix.index.ntotal
    r = c.delete("/api/index/documents/A1")
    assert r.status_code == 200
    assert r.json() == {"removed": n - ix.index.ntotal, "ntotal": ix.index.ntotal, "version": ix.version}
    assert r.json()["removed"] > 0 and c.get("/api/index/stats").json()["ntotal"] == ix.index.ntotal
    assert c.delete("/api/index/documents/A1").status_code == 404
    assert c.delete("/api/index/documents/KB").status_code == 404
    r = c.delete("/api/index/patients/B")
    assert r.status_code == 200 and r.json()["removed"] > 0
    assert c.delete("/api/index/patients/B").status_code == 404
    assert not any(h["doc_id"].startswith("B") for h in c.post("/api/search", json={"query": "patient B", "k": 20}).json())

    # a sharded store refuses before anything is logged
    real, seq = ix.index, ix.wal.last_seq
    sharded = object.__new__(ShardedIndex)
    sharded.ntotal_probe = None
    ix.index = sharded
    assert c.delete("/api/index/documents/A0").status_code == 422 and ix.wal.last_seq == seq
    ix.index = None
    assert c.delete("/api/index/documents/A0").status_code == 503
    ix.index = real
    assert len(ix.patients.rows("A0")) > 0


def test_sharded_index_refuses():
    from docqa_amd.index.sharded import ShardedIndex, ShardedIVFPQIndex

    for cls in (ShardedIndex, ShardedIVFPQIndex):
        assert cls.can_remove is False
        with pytest.raises(NotImplementedError):
            cls.remove_ids(object.__new__(cls), [0])


# ------------------------------------------------------------------ HTTP: ingest, UI
class _Broker:
    def __init__(self):
        self.sent, self.fail = [], False

    def publish(self, queue, body):
        if self.fail:
            raise RuntimeError("bus down")
        self.sent.append((queue, json.loads(body)))


def test_ingest_delete_route(tmp_path):
    from fastapi.testclient import TestClient

    from docqa_amd.config import Settings
    from docqa_amd.services import ingest

    st = Settings()
    st.upload_dir = str(tmp_path / "up")
    db, broker = docs_db.DocsDB("sqlite://"), _Broker()
    c = TestClient(ingest.create_app(st, db, broker))
    assert c.delete("/documents/12345").status_code == 404

    def doc(status):
        i = db.create("note.txt", "compte-rendu", status)
        (tmp_path / "up" / f"{i}_note.txt").write_text("x")
        return i, tmp_path / "up" / f"{i}_note.txt"

    for status in (docs_db.STATUS_PENDING, docs_db.STATUS_PROCESSED):
        i, path = doc(status)
        r = c.delete(f"/documents/{i}")
        assert r.status_code == 409 and db.get(i)["status"] == status and path.exists() and broker.sent == []

    i, path = doc(docs_db.STATUS_INDEXED)
    r = c.delete(f"/documents/{i}")
    assert r.status_code == 202 and r.json() == {"doc_id": i, "status": "DELETING"}
    assert db.get(i)["status"] == docs_db.STATUS_DELETING and not path.exists()
    assert broker.sent == [(st.clean_queue, {"op": "delete", "doc_id": i})]
    # DELETING may be deleted again: the message is idempotent, an indexer that dead-lettered the
    # first one gets another
    assert c.delete(f"/documents/{i}").status_code == 202 and len(broker.sent) == 2
    assert broker.sent[1] == broker.sent[0] and db.get(i)["status"] == docs_db.STATUS_DELETING
    broker.fail = True
    assert c.delete(f"/documents/{i}").status_code == 503 and db.get(i)["status"] == docs_db.STATUS_DELETING
    broker.fail = False
    db.set_status(i, docs_db.STATUS_DELETED)                            # what on_deleted does
    assert c.delete(f"/documents/{i}").status_code == 200 and len(broker.sent) == 2

    for status in (docs_db.STATUS_ERROR_EXTRACTION, docs_db.STATUS_ERROR_QUEUE):
        j, path = doc(status)
        r = c.delete(f"/documents/{j}")
        assert r.status_code == 200 and r.json()["status"] == "DELETED" and not path.exists()
        assert db.get(j)["status"] == docs_db.STATUS_DELETED and len(broker.sent) == 2

    k, path = doc(docs_db.STATUS_INDEXED)                                # the bus is down: nothing changes state
    broker.fail = True
    assert c.delete(f"/documents/{k}").status_code == 503 and db.get(k)["status"] == docs_db.STATUS_INDEXED
    assert path.exists()                                                # the file goes only with a published delete
    assert c.get(f"/documents/{k}").json()["status"] == "INDEXED"


def test_stack_wires_on_deleted(tmp_path):
    """The delete message of the ingestor, handled by the stack's indexer, ends in DELETED."""
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = _settings(tmp_path)
    st.database_url = "sqlite://"
    st.upload_dir = str(tmp_path / "up")
    s = DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu", max_batch=4,
                                max_context=1024, use_graphs=False, services=("ingest", "indexer")), st)
    try:
        i = s.db.create("note.txt", "compte-rendu", docs_db.STATUS_INDEXED)
        s.indexer.index_document(i, f"Note avec {WORD}.", {"patient_id": "Z"})
        assert len(s.indexer.patients.rows(str(i))) == 1
        s.indexer.stop_consumer()
        s.indexer._depth = lambda q: 0
        ch = _Channel()
        s.indexer.callback(ch, _Method(1), None, json.dumps({"op": "delete", "doc_id": i}).encode())
        assert ch.acked == [1]
        assert s.db.get(i)["status"] == docs_db.STATUS_DELETED and s.indexer.patients.rows(str(i)) == []
    finally:
        s.close()


def test_ui_proxies_the_delete(monkeypatch):
    from fastapi.testclient import TestClient

    from docqa_amd.services import ui

    seen = []

    def handler(req: httpx.Request) -> httpx.Response:
        seen.append((req.method, req.url.port, req.url.path))
        if req.url.path == "/documents/7":
            return httpx.Response(202, json={"doc_id": 7, "status": "DELETING"})
        return httpx.Response(404, json={"detail": "Document not found"})

    real = httpx.AsyncClient

    class Mocked(real):
        def __init__(self, *a, **kw):
            kw["transport"] = httpx.MockTransport(handler)
            super().__init__(*a, **kw)

    monkeypatch.setattr(ui.httpx, "AsyncClient", Mocked)
    c = TestClient(ui.create_app())
    r = c.delete("/ui/documents/7")
    assert r.status_code == 202 and r.json() == {"doc_id": 7, "status": "DELETING"}
    assert c.delete("/ui/documents/8").status_code == 404
    assert seen == [("DELETE", 8000, "/documents/7"), ("DELETE", 8000, "/documents/8")]


# ------------------------------------------------------------------ RAG pipeline
@pytest.fixture()
def rag(tmp_path):
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = _settings(tmp_path)
    st.database_url = "sqlite://"
    st.max_new_tokens = 2
    s = DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu", max_batch=4,
                                max_context=1024, use_graphs=False, services=("indexer", "qa")), st)
    _fill(s.indexer)
    yield s
    s.close()


def test_pipeline_drops_caches_on_a_generation_change(rag):
    pipe, ix = rag.pipeline, rag.indexer
    assert pipe.owner is ix and pipe.metadata is ix.metadata
    qs = ["tension du patient A ?", f"traitement par {WORD} ?"]
    pipe.answer_batch(qs)
    assert pipe._chunk_ids and pipe._generation == ix.generation == 0
    cached = dict(pipe._chunk_ids)
    pipe.answer_batch(qs)
    assert pipe._chunk_ids == cached                                    # no delete: the caches stay
    ix.delete_document("A0")
    pipe._chunk_ids[10 ** 9] = [1]                                       # a stale entry under an old id
    pipe._seen.add((10 ** 9,))
    ans = pipe.answer_batch(qs)
    assert pipe._generation == ix.generation == 2
    assert 10 ** 9 not in pipe._chunk_ids and (10 ** 9,) not in pipe._seen
    for a in ans:
        assert a.sources == [ix.metadata[i]["source"] for i in a.chunk_ids]
        assert "Dossier Patient A0" not in a.sources
    for i, toks in pipe._chunk_ids.items():                             # every cached piece is its row's text
        assert toks == pipe.chat_tok.encode(ix.metadata[i]["text_content"])


def test_delete_between_search_and_resolve_triggers_a_retry(rag):
    pipe, ix = rag.pipeline, rag.indexer
    victim = "B1"
    q = [f"traitement par {WORD} 5 mg ?"]
    before = pipe.answer_batch(q)[0]
    assert "Dossier Patient B1" in before.sources                       # the document is what the question finds
    calls = []

    def hook():
        calls.append(ix.generation)
        if len(calls) == 1:
            assert ix.delete_document(victim) > 0                       # ids shift under the resolved hits

    pipe._after_search = hook
    ans = pipe.answer_batch(q)[0]
    assert len(calls) == 2 and calls[1] == calls[0] + 2                 # searched again under the new generation
    assert "Dossier Patient B1" not in ans.sources and ans.sources
    assert ans.sources == [ix.metadata[i]["source"] for i in ans.chunk_ids]
    pipe._after_search = None


def test_pipelined_and_served_paths_retry_too(rag):
    from fastapi.testclient import TestClient

    pipe, ix = rag.pipeline, rag.indexer
    q = f"traitement par {WORD} 5 mg ?"
    calls = []

    def hook():
        calls.append(1)
        if len(calls) == 1:
            assert ix.delete_document("B1") > 0

    pipe._after_search = hook
    out = list(pipe.answer_pipelined([[q], ["tension du patient A ?"]]))
    assert len(calls) == 3                                              # batch 0 searched twice, batch 1 once
    for answers, _, _ in out:
        for a in answers:
            assert "Dossier Patient B1" not in a.sources
            assert a.sources == [ix.metadata[i]["source"] for i in a.chunk_ids]
    # the service's batcher resolves through the same guard
    calls.clear()
    victim = "A2"

    def hook2():
        calls.append(1)
        if len(calls) == 1:
            assert ix.delete_document(victim) > 0

    pipe._after_search = hook2
    r = TestClient(rag.qa_app).post("/ask/", json={"question": "Note 2 du patient A : tension ?"})
    assert r.status_code == 200 and len(calls) == 2
    assert "Dossier Patient A2" not in r.json()["sources"]
    pipe._after_search = None


def test_pipeline_without_an_owner_checks_nothing(rag):
    from docqa_amd.pipeline.rag import RAGPipeline

    p = rag.pipeline
    plain = RAGPipeline(p.encoder, p.enc_tok, p.index, p.metadata, p.engine, p.chat_tok, k=p.k)
    assert plain.owner is None
    a = plain.answer_batch(["tension du patient A ?"])[0]
    assert a.sources == [p.metadata[i]["source"] for i in a.chunk_ids]


# ------------------------------------------------------------------ failure and timing of the swap
def test_failed_column_compaction_changes_nothing(tmp_path, encoder, monkeypatch):
    ix = _indexer(tmp_path, encoder)
    _fill(ix)
    ix.ensure_lexical()
    before, gen = _state(ix), ix.generation
    lex = (ix.lexical.n, ix.lexical.entries, dict(ix.lexical.df), ix.lexical.terms.clone())

    def boom(*a, **kw):
        raise ValueError("the removed records do not match")

    monkeypatch.setattr(ix.lexical, "prepare_remove", boom)
    with pytest.raises(ValueError):
        ix._apply_delete(sorted(ix.patients.rows("A1")))
    after = _state(ix)
    assert torch.equal(after[0], before[0]) and after[1] == before[1] and after[3] == before[3]
    assert torch.equal(after[2], before[2]) and ix.scopes.n == len(ix.metadata) == ix.index.ntotal
    assert (ix.lexical.n, ix.lexical.entries, ix.lexical.df) == lex[:3] and torch.equal(ix.lexical.terms, lex[3])
    assert ix.generation == gen                         # never went odd: nothing was being swapped
    monkeypatch.undo()
    assert ix.delete_document("A1") > 0 and ix.generation == gen + 2


def test_generation_is_even_again_before_the_index_lock_is_released(tmp_path, encoder):
    from docqa_amd.index.follower import IndexFollower

    w = _indexer(tmp_path, encoder)
    w.save_state()
    f = IndexFollower(str(tmp_path), d=encoder.cfg.hidden, device="cpu")
    f.poll()
    _fill(w)
    f.poll()
    seen = []
    for owner in (w, f):
        lock = owner.index._lock
        real_release = lock.release

        class Spy:                                      # the RLock, recording the counter at each release
            def __enter__(self):
                return lock.__enter__()

            def __exit__(self, *a):
                seen.append(owner.generation)
                return lock.__exit__(*a)

            def acquire(self, *a, **kw):
                return lock.acquire(*a, **kw)

            def release(self):
                seen.append(owner.generation)
                return real_release()

        owner.index._lock = Spy()
    w.delete_document("A1")
    f.poll()
    w.save_state()
    w.index_document("C0", "Une note.", {"patient_id": "C"})
    f.poll()                                            # a snapshot reload swaps too
    assert seen and all(g % 2 == 0 for g in seen) and w.generation == 2 and f.generation >= 4
