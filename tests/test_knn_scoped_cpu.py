"""Scoped retrieval on the CPU: the fp32 reference against a brute-force loop, the row
attribute columns and scope rows (index/scope.py), ``search_scoped`` on both store types, and
the /ask/ and /api/search contracts through both batchers and the index follower (tiny random
models, in-process stack as test_services_cpu.py builds it)."""
import concurrent.futures as cf
import datetime
import time

import pytest
import torch
from fastapi.testclient import TestClient

from docqa_amd.config import Settings

IMIN, IMAX = -(1 << 31), (1 << 31) - 1


# ------------------------------------------------------------------ reference
def _brute(xb, tags, days, xq, scope, k, ip, id_offset):
    out_d, out_i = [], []
    for q in range(xq.shape[0]):
        tag, alt, lo, hi = scope[q].tolist()
        cand = []
        for r in range(xb.shape[0]):
            rt, rd = int(tags[r]), int(days[r])
            if rt == alt or ((tag < 0 or rt == tag) and lo <= rd <= hi):
                dot = float((xb[r].double() * xq[q].double()).sum())
                dist = -dot if ip else float(((xb[r].double() - xq[q].double()) ** 2).sum())
                cand.append((dist, r))
        cand.sort()
        cand = cand[:k]
        out_d.append([(-d if ip else d) for d, _ in cand])
        out_i.append([r + id_offset for _, r in cand] + [-1] * (k - len(cand)))
    return out_d, out_i


@pytest.mark.parametrize("ip", [False, True])
def test_reference_vs_brute_force(ip):
    from docqa_amd.ops import knn_scoped
    from docqa_amd.ops import reference as R

    g = torch.Generator().manual_seed(0)
    N, d, k = 23, 8, 5
    xb = torch.randn(N, d, generator=g)
    xq = torch.randn(9, d, generator=g)
    tags = torch.tensor([0, 0, 1, 1, 1, 2, 2, 0, 3, 3, 3, 3, 1, 0, 4, 4, 2, 2, 0, 5, 5, 5, 0], dtype=torch.int32)
    days = torch.tensor([IMIN if i % 4 == 0 else 700000 + i for i in range(N)], dtype=torch.int32)
    scope = torch.tensor([
        (-1, -1, IMIN, IMAX),               # any scope: undated rows pass
        (1, -1, IMIN, IMAX),                # one patient
        (1, 0, IMIN, IMAX),                 # patient + knowledge base
        (3, 0, 700009, 700010),             # window; the knowledge base is exempt from it
        (-1, -1, IMIN + 1, 700012),         # only an upper bound: undated rows excluded
        (-1, -1, 700012, IMAX),             # only a lower bound
        (0, -1, IMIN, IMAX),                # knowledge base only
        (IMAX, -1, IMIN, IMAX),             # unknown patient: nothing
        (IMAX, 0, 5, 6),                    # unknown patient + knowledge base
    ], dtype=torch.int32)
    norms = (xb ** 2).sum(1)
    D, I = R.knn_scoped(xb, norms, tags, days, xq, scope, k, ip, 100)
    D_op, I_op = knn_scoped(xb, norms, tags, days, xq, scope, k, ip, 100)   # CPU tensors -> the reference
    assert torch.equal(D, D_op) and torch.equal(I, I_op)
    bd, bi = _brute(xb, tags, days, xq, scope, k, ip, 100)
    assert I.tolist() == bi
    sent = -3.4028234663852886e38 if ip else 3.4028234663852886e38
    for q in range(len(bd)):
        n = len(bd[q])
        assert torch.allclose(D[q, :n].double(), torch.tensor(bd[q], dtype=torch.float64), atol=1e-4)
        assert (D[q, n:] == sent).all()
    assert (I[7] == -1).all()
    assert all(i % 4 and i <= 12 for i in (I[4] - 100).tolist())       # dated, up to the bound
    # the any-scope row is the unscoped search
    Dk, Ik = R.knn(xb, norms, xq[:1], k, ip, 100)
    assert torch.equal(I[:1], Ik) and torch.allclose(D[:1], Dk)
    # empty inputs
    De, Ie = R.knn_scoped(xb[:0], norms[:0], tags[:0], days[:0], xq, scope, k, ip, 0)
    assert (Ie == -1).all() and (De == sent).all()


# ------------------------------------------------------------------ ScopeColumns
def _meta():
    return [
        {"doc_id": "KB", "type": "knowledge_base", "text_content": "a", "source": "kb.csv"},
        {"doc_id": "7", "type": "patient_file", "patient_id": "P1", "note_date": "2021-03-12", "text_content": "b"},
        {"doc_id": "8", "type": "patient_file", "patient_id": "P2", "note_date": None, "text_content": "c"},
        {"doc_id": "9", "type": "patient_file", "text_content": "d"},                     # no patient_id: doc_id
        {"doc_id": "10", "type": "patient_file", "patient_id": "P1", "note_date": "2023-05-01", "text_content": "e"},
        {"doc_id": "11", "type": "knowledge_base", "patient_id": "P1", "text_content": "f"},  # not a patient file
        {"doc_id": "12", "type": "patient_file", "patient_id": 9, "note_date": "2022-01-31", "text_content": "g"},
    ]


def test_scope_columns_extend_and_rebuild():
    from docqa_amd.index.scope import UNDATED, ScopeColumns

    meta = _meta()
    a = ScopeColumns("cpu", capacity=2)
    a.rebuild(meta[:3])
    assert a.n == 3
    a.extend(meta[:5])
    a.extend(meta)
    a.extend(meta)                      # nothing new
    b = ScopeColumns("cpu")
    b.rebuild(meta)
    assert a.n == b.n == len(meta)
    assert torch.equal(a.tags, b.tags) and torch.equal(a.days, b.days)
    assert a.tags.dtype == torch.int32 and a.days.dtype == torch.int32
    # P1 -> 1, P2 -> 2, doc 9 -> 3 (the doc_id fallback; the integer patient 9 shares the key "9")
    assert a.tags.tolist() == [0, 1, 2, 3, 1, 0, 3]
    day = lambda s: datetime.date.fromisoformat(s).toordinal()  # noqa: E731
    assert a.days.tolist() == [UNDATED, day("2021-03-12"), UNDATED, UNDATED, day("2023-05-01"), UNDATED,
                               day("2022-01-31")]
    assert a.tag("P1") == 1 and a.tag(9) == 3 and a.tag("nobody") == IMAX
    b.rebuild(meta[3:])                 # a rebuild starts over
    assert b.n == 4 and b.tags.tolist() == [1, 2, 0, 1]


def test_scope_rows_every_request_form():
    from docqa_amd.index.scope import ScopeColumns, scope_request

    c = ScopeColumns("cpu")
    c.rebuild(_meta())
    day = lambda s: datetime.date.fromisoformat(s).toordinal()  # noqa: E731
    reqs = [
        None,
        {"patient_id": "P1"},
        {"patient_id": "P1", "include_knowledge_base": False},
        {"patient_id": "P2", "from_date": "2021-01-01"},
        {"patient_id": "P2", "to_date": "31/12/2022", "include_knowledge_base": False},
        {"patient_id": "P1", "from_date": "2021-01-01", "to_date": "12 mars 2021"},
        {"patient_id": "nobody"},
        {"from_date": "2021-01-01", "include_knowledge_base": False},
        {"patient_id": None, "from_date": None, "to_date": None, "include_knowledge_base": True},
    ]
    rows = c.scope_rows(reqs)
    assert rows.dtype == torch.int32 and rows.shape == (len(reqs), 4)
    assert rows.tolist() == [
        [-1, -1, IMIN, IMAX],
        [1, 0, IMIN, IMAX],
        [1, -1, IMIN, IMAX],
        [2, 0, day("2021-01-01"), IMAX],
        [2, -1, IMIN + 1, day("2022-12-31")],
        [1, 0, day("2021-01-01"), day("2021-03-12")],
        [IMAX, 0, IMIN, IMAX],
        [-1, -1, day("2021-01-01"), IMAX],
        [-1, -1, IMIN, IMAX],
    ]
    assert c.scope_rows([]).shape == (0, 4)
    with pytest.raises(ValueError):
        c.scope_rows([{"patient_id": "P1", "from_date": "soon"}])
    # the wire fields: nothing set -> no scope at all (the unscoped path)
    assert scope_request() is None and scope_request(None, "", None, True) is None
    assert scope_request("P1", "12/03/2021", None, False) == {
        "patient_id": "P1", "from_date": "2021-03-12", "to_date": None, "include_knowledge_base": False}
    with pytest.raises(ValueError):
        scope_request("P1", None, "not a date")
    with pytest.raises(ValueError):
        scope_request(include_knowledge_base=False)


# ------------------------------------------------------------------ search_scoped
def test_search_scoped_flat_ivfpq_sharded():
    from docqa_amd.index.flat import FlatIndex
    from docqa_amd.index.hybrid import IVFPQRefineIndex
    from docqa_amd.index.scope import ScopeColumns
    from docqa_amd.index.sharded import ShardedIndex
    from docqa_amd.ops import reference as R

    g = torch.Generator().manual_seed(1)
    d, N = 16, 300
    x = torch.randn(N, d, generator=g)
    q = torch.randn(5, d, generator=g)
    meta = [({"doc_id": str(i // 7), "type": "patient_file", "patient_id": f"P{i // 20}",
              "note_date": f"2022-01-{1 + i % 28:02d}", "text_content": "x"} if i % 5 else
             {"doc_id": "KB", "type": "knowledge_base", "text_content": "x"}) for i in range(N)]
    cols = ScopeColumns("cpu")
    cols.rebuild(meta)
    scope = cols.scope_rows([None, {"patient_id": "P3"}, {"patient_id": "P3", "include_knowledge_base": False},
                             {"patient_id": "P4", "from_date": "2022-01-10", "to_date": "2022-01-12"},
                             {"patient_id": "nobody", "include_knowledge_base": False}])
    flat = FlatIndex(d, "l2", "cpu")
    flat.add(x)
    for trained in (False, True):
        ivf = IVFPQRefineIndex(d, nlist=4, M=4, nprobe=4, train_min=(100 if trained else 10_000), device="cpu")
        ivf.add(x)
        assert ivf.trained == trained
        D1, I1 = flat.search_scoped(q, 4, cols, scope, id_offset=10)
        D2, I2 = ivf.search_scoped(q, 4, cols, scope, id_offset=10)
        assert torch.equal(I1, I2) and torch.equal(D1, D2)
    Dr, Ir = R.knn_scoped(x, (x ** 2).sum(1), cols.tags, cols.days, q, scope, 4, False, 10)
    assert torch.equal(I1, Ir)
    assert torch.equal(I1[0], flat.search(q[:1], 4, id_offset=10)[1][0])
    assert all(meta[i - 10].get("patient_id") == "P3" for i in I1[2].tolist())
    assert all(meta[i - 10].get("patient_id") in ("P3", None) for i in I1[1].tolist())
    assert (I1[4] == -1).all()
    # columns that cover fewer rows than the index: only those rows are searched
    part = ScopeColumns("cpu")
    part.rebuild(meta[:50])
    _, Ip = flat.search_scoped(q, 4, part, part.scope_rows([None] * 5))
    assert int(Ip.max()) < 50
    with pytest.raises(NotImplementedError, match="sharding the deployed index"):
        ShardedIndex(flat).search_scoped(q, 4, cols, scope)


# ------------------------------------------------------------------ services
QUESTION = "Quel est le traitement anticoagulant en cours du patient ?"
KB_ONLY = {"patient_id": "PA", "from_date": "2030-01-01"}


def _fill(indexer):
    """Two patients + the synthetic knowledge base; patient PB's chunks repeat the test
    question, so they are the question's global nearest neighbours."""
    indexer.index_document(101, "Consultation de suivi : tension artérielle stable, poursuite du ramipril.",
                           {"patient_id": "PA", "note_date": "2021-03-12"})
    indexer.index_document(102, "Bilan biologique : créatinine normale, kaliémie normale.",
                           {"patient_id": "PA", "note_date": "2023-05-01"})
    for doc in (201, 202, 203):
        indexer.index_document(doc, QUESTION, {"patient_id": "PB", "note_date": "2022-06-01"})


def _stack(tmp, mode):
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = Settings()
    st.index_dir = str(tmp)
    st.default_data_dir = str(tmp / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 3
    st.serving_mode = mode
    s = DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu",
                                max_batch=4, max_context=1024, use_graphs=False), st)
    _fill(s.indexer)
    return s


@pytest.fixture(scope="module", params=["continuous", "batch"])
def stack(request, tmp_path_factory):
    s = _stack(tmp_path_factory.mktemp("scoped_" + request.param), request.param)
    yield s
    s.close()


PA_SRC = {"Dossier Patient 101", "Dossier Patient 102"}
PB_SRC = {"Dossier Patient 201", "Dossier Patient 202", "Dossier Patient 203"}


def _is_kb(src):
    return src is not None and not src.startswith("Dossier Patient")


def _assert_scoped(srcs_by_scope):
    """What each of the four request forms must have retrieved."""
    plain, pa, pa_only, kb_only = srcs_by_scope
    assert set(plain) & PB_SRC, "the corpus must put another patient's chunk in the unscoped top-k"
    assert len(pa) == 3 and not set(pa) & PB_SRC and all(s in PA_SRC or _is_kb(s) for s in pa)
    assert sorted(pa_only) == sorted(PA_SRC)               # the patient's two chunks, nothing else
    assert len(kb_only) == 3 and all(_is_kb(s) for s in kb_only)


def test_ask_scopes(stack):
    qa = TestClient(stack.qa_app)

    def ask(**kw):
        r = qa.post("/ask/", json={"question": QUESTION, **kw})
        assert r.status_code == 200 and set(r.json()) == {"answer", "sources"}
        return r.json()["sources"]

    _assert_scoped([ask(), ask(patient_id="PA"), ask(patient_id="PA", include_knowledge_base=False), ask(**KB_ONLY)])
    unknown = ask(patient_id="nobody")
    assert len(unknown) == 3 and all(_is_kb(s) for s in unknown)
    assert ask(patient_id="nobody", include_knowledge_base=False) == []      # empty context, still answered
    assert len(ask(patient_id="PB", include_knowledge_base=False, from_date="01/06/2022", to_date="2022-06-01")) == 3
    assert ask(patient_id="PB", include_knowledge_base=False, to_date="2022-05-31") == []
    assert qa.post("/ask/", json={"question": QUESTION, "patient_id": "PA", "from_date": "hier"}).status_code == 422


def test_ask_mixed_batch_through_the_batcher(stack):
    """Scoped and unscoped asks queued together are one prep batch (one scoped launch); an
    unscoped ask's payload stays a plain string."""
    from docqa_amd.index.scope import scope_request
    from docqa_amd.services.qa import ask_payload

    assert ask_payload(QUESTION, scope_request()) == QUESTION
    b = stack.qa_app.state.batcher
    scopes = [None, scope_request("PA"), scope_request("PA", include_knowledge_base=False), scope_request(**KB_ONLY)]
    items = [("ask", ask_payload(QUESTION, s), cf.Future(), time.perf_counter()) for s in scopes]
    with torch.inference_mode():
        (b._admit if hasattr(b, "_admit") else b._run)(items)
    _assert_scoped([it[2].result(timeout=300)["sources"] for it in items])
    # and through the front door, concurrently
    qa = TestClient(stack.qa_app)
    bodies = [{"question": QUESTION}, {"question": QUESTION, "patient_id": "PA"},
              {"question": QUESTION, "patient_id": "PA", "include_knowledge_base": False},
              {"question": QUESTION, **KB_ONLY}] * 2
    with cf.ThreadPoolExecutor(8) as ex:
        res = [f.result(timeout=300) for f in [ex.submit(qa.post, "/ask/", json=body) for body in bodies]]
    assert all(r.status_code == 200 for r in res)
    for i in (0, 4):
        _assert_scoped([r.json()["sources"] for r in res[i:i + 4]])


def test_pipeline_scopes_lazy_columns(stack):
    """A pipeline nobody handed ScopeColumns builds them from its metadata at search time."""
    from docqa_amd.pipeline.rag import RAGPipeline

    p = stack.pipeline
    own = RAGPipeline(p.encoder, p.enc_tok, p.index, p.metadata, p.engine, p.chat_tok, k=3)
    assert own.scopes is None
    D0, I0 = own.retrieve([QUESTION])
    assert own.scopes is None                               # unscoped: the plain search, nothing built
    D, I = own.retrieve([QUESTION, QUESTION], scopes=[None, {"patient_id": "PA", "include_knowledge_base": False}])
    assert own.scopes is not None and own.scopes.n == len(p.metadata)
    assert torch.equal(I[0], I0[0])
    srcs = [p.metadata[i]["source"] for i in I[1].tolist() if i >= 0]
    assert sorted(srcs) == sorted(PA_SRC) and I[1, 2] == -1


def test_api_search_scopes(stack):
    idx = TestClient(stack.indexer_app)

    def search(**kw):
        r = idx.post("/api/search", json={"query": QUESTION, "k": 3, **kw})
        assert r.status_code == 200
        return [h["source"] for h in r.json()]

    _assert_scoped([search(), search(patient_id="PA"), search(patient_id="PA", include_knowledge_base=False),
                    search(**KB_ONLY)])
    assert search(patient_id="nobody", include_knowledge_base=False) == []
    r = idx.post("/api/search", json={"query": QUESTION, "patient_id": "PA", "to_date": "32/13/2021"})
    assert 400 <= r.status_code < 500 and "to_date" in r.json()["detail"]
    # the unscoped request is served exactly as before
    hits = idx.post("/api/search", json={"query": QUESTION, "k": 2}).json()
    assert [h["id"] for h in hits] == [h["id"] for h in stack.indexer.search(QUESTION, 2)]
    # patient-snippets is untouched
    snips = idx.get("/api/search/patient-snippets", params={"patient_id": "PA"}).json()
    assert len(snips) == 2


def test_replica_router_forwards_scope(stack):
    """The local leg of the router turns the wire fields back into the batcher's scope."""
    import asyncio

    from docqa_amd.services.qa import ReplicaRouter

    router = ReplicaRouter(stack.qa_app.state.batcher, [])
    out = asyncio.run(router.call("ask", "/ask/", {"question": QUESTION, "patient_id": "PA",
                                                   "from_date": None, "to_date": None,
                                                   "include_knowledge_base": False}, "question"))
    assert sorted(out["sources"]) == sorted(PA_SRC)
    out = asyncio.run(router.call("ask", "/ask/", {"question": QUESTION}, "question"))
    assert set(out["sources"]) & PB_SRC


def test_index_follower_keeps_scopes(tmp_path):
    """Rows appended through the WAL are reachable by scope after poll(); a snapshot reload
    keeps them reachable."""
    from docqa_amd.index.follower import IndexFollower
    from docqa_amd.models.bert import BertConfig, BertEncoder
    from docqa_amd.services.indexer import SemanticIndexer
    from docqa_amd.text.tokenizer import WordPieceTokenizer

    st = Settings()
    st.index_dir = str(tmp_path)
    st.default_data_dir = str(tmp_path / "nodata")
    st.snapshot_every = 100
    enc = BertEncoder(BertConfig.preset("tiny-bert"), device="cpu")
    tok = WordPieceTokenizer()
    w = SemanticIndexer(enc, tok, st, device="cpu").startup(build_if_missing=True)
    f = IndexFollower(str(tmp_path), d=enc.cfg.hidden, device="cpu")
    f.poll()
    n_kb = f.index.ntotal
    assert f.scopes.n == n_kb and not f.scopes.tags.any()
    q = enc.encode(tok.encode_batch([QUESTION]))

    def patient_rows(fol, pid):
        sc = fol.scopes.scope_rows([{"patient_id": pid, "include_knowledge_base": False}])
        _, I = fol.index.search_scoped(q, 3, fol.scopes, sc)
        return [fol.metadata[i]["source"] for i in I[0].tolist() if i >= 0]

    assert patient_rows(f, "PA") == []
    _fill(w)                                        # WAL frames, no snapshot
    assert f.poll() == 5
    assert f.scopes.n == f.index.ntotal == len(f.metadata) == n_kb + 5
    assert sorted(patient_rows(f, "PA")) == sorted(PA_SRC)
    assert set(patient_rows(f, "PB")) <= PB_SRC and len(patient_rows(f, "PB")) == 3
    w.save_state()                                  # snapshot + log rotation: the follower reloads
    w.index_document(103, "Courrier de sortie.", {"patient_id": "PA", "note_date": "2024-01-01"})
    f.poll()
    assert f.scopes.n == f.index.ntotal == n_kb + 6
    assert torch.equal(f.scopes.tags, w.scopes.tags) and torch.equal(f.scopes.days, w.scopes.days)
    assert sorted(patient_rows(f, "PA")) == sorted(PA_SRC | {"Dossier Patient 103"})
    g = IndexFollower(str(tmp_path), d=enc.cfg.hidden, device="cpu")   # a late joiner loads the snapshot
    g.poll()
    assert sorted(patient_rows(g, "PA")) == sorted(PA_SRC | {"Dossier Patient 103"})
