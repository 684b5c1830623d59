"""Maximal marginal relevance on the CPU: ``ops.reference.mmr_select`` against an fp64 oracle
written out here (the replay check and the exact-arithmetic cases of tests/test_mmr_gpu.py at
small shapes), and ``search_type=mmr`` through the services on the tiny CPU stack."""
from __future__ import annotations

import pytest
import torch

from docqa_amd.ops import reference as ref

# the fp64 oracle, the replay check and the case builders are written out in the GPU test file
from tests.test_mmr_gpu import check_exact, check_mixed_pipeline, cluster_lists, cluster_rows, replay


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("d,dtype", [(8, torch.float32), (40, torch.float32), (48, torch.bfloat16)])
def test_reference_replays_against_fp64(d, dtype):
    N, nq = 500, 13
    tol = 4 * (d + 8) * 2.0 ** -24
    cent, xb, xb64 = cluster_rows(N, d, dtype)
    for F in (1, 3, 20):
        xq, cand, ncand, lam = cluster_lists(cent, N, nq, F, seed=F)
        for k in sorted({1, min(3, F), F}):
            S, I, P = ref.mmr_select(xb, (xb.float() ** 2).sum(1), torch.from_numpy(xq), torch.from_numpy(cand),
                                     torch.from_numpy(ncand), torch.from_numpy(lam), k)
            assert S.dtype == torch.float32 and I.dtype == torch.int64 and P.dtype == torch.int32
            assert S.shape == I.shape == P.shape == (nq, k)
            replay(xb64, xq, cand, ncand, lam, k, S.numpy(), I.numpy(), P.numpy(), tol)


@pytest.mark.parametrize("d,F,k", [(64, 20, 3), (64, 64, 64), (384, 20, 3)])
def test_reference_exact_arithmetic_and_ties(d, F, k):
    check_exact(ref.mmr_select, d, F, k)


def test_reference_empty_and_padded():
    xb = torch.randn(10, 8)
    nm = (xb * xb).sum(1)
    S, I, P = ref.mmr_select(xb, nm, torch.zeros(0, 8), torch.zeros(0, 4, dtype=torch.long),
                             torch.zeros(0, dtype=torch.int32), torch.zeros(0), 3)
    assert S.shape == I.shape == P.shape == (0, 3)
    S, I, P = ref.mmr_select(xb, nm, torch.randn(2, 8), torch.tensor([[1, 2, 3, 4], [5, 6, 7, 8]]),
                             torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0.5, 0.5]), 3)
    assert I[0].tolist() == [-1, -1, -1] and P[0].tolist() == [-1, -1, -1] and S[0].tolist() == [0, 0, 0]
    assert sorted(I[1, :2].tolist()) == [5, 6] and I[1, 2] == -1 and P[1, 2] == -1 and S[1, 2] == 0


def test_pipeline_mixed_batch_on_the_reference():
    """The mixed dense / hybrid / lexical, scoped / unscoped, MMR on / off batch of the GPU
    suite, on the CPU ops."""
    check_mixed_pipeline("cpu")


def test_sharded_index_refuses():
    from docqa_amd.index.sharded import ShardedIndex

    with pytest.raises(NotImplementedError):
        ShardedIndex.mmr_select(object.__new__(ShardedIndex), None, None, None, None, 3)


# ------------------------------------------------------------------ services (tiny models)
NOTE = "Compte rendu : patient sous traitement anticoagulant, tension stable, bilan biologique normal."


def _make_stack(d, serving=None, monkeypatch=None):
    from docqa_amd.config import Settings
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = Settings()
    st.index_dir = str(d)
    st.default_data_dir = str(d / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 2
    if serving is not None:
        st.serving_mode = serving
    s = DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu", max_batch=4,
                                max_context=1024, use_graphs=False, services=("indexer", "qa")), st)
    # the same note uploaded twice (nothing deletes or replaces a document), beside other notes
    s.indexer.index_document("N1", NOTE, {"patient_id": "A", "note_date": "2024-01-01"})
    s.indexer.index_document("N2", NOTE, {"patient_id": "A", "note_date": "2024-01-01"})
    for j in range(4):
        s.indexer.index_document(f"M{j}", f"Note {j} : patient vu en consultation de suivi numero {j}, tension correcte.",
                                 {"patient_id": "A", "note_date": f"2024-02-{j + 1:02d}"})
    return s


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    s = _make_stack(tmp_path_factory.mktemp("mmrstack"))
    yield s
    s.close()


def _texts(stack, sources):
    by = {m.get("source"): m["text_content"] for m in stack.indexer.metadata}
    return [by[s] for s in sources]


def test_service_mmr_returns_distinct_sources(stack):
    from fastapi.testclient import TestClient

    idx = TestClient(stack.indexer_app)
    body = {"query": NOTE, "k": 2, "patient_id": "A", "include_knowledge_base": False}
    plain = idx.post("/api/search", json=body).json()
    assert [h["text"] for h in plain] == [NOTE, NOTE]                  # the two uploads of one note
    mmr = idx.post("/api/search", json={**body, "search_type": "mmr", "fetch_k": 6}).json()
    assert len(mmr) == 2 and mmr[0]["text"] == NOTE and mmr[1]["text"] != NOTE
    # (either upload: the two tie exactly, and a search's order among ties depends on its depth)
    assert mmr[0]["id"] in {h["id"] for h in plain}
    assert mmr[0]["score"] == pytest.approx(plain[0]["score"], rel=1e-5, abs=1e-6)
    # the score is the leg's own: the L2 distance of that row
    deep = {h["id"]: h["score"] for h in idx.post("/api/search", json={**body, "k": 6}).json()}
    assert all(h["score"] == pytest.approx(deep[h["id"]], rel=1e-5, abs=1e-6) for h in mmr)
    # lambda_mult = 1: relevance alone, the duplicates again
    rel = idx.post("/api/search", json={**body, "search_type": "mmr", "fetch_k": 6, "lambda_mult": 1.0}).json()
    assert [h["text"] for h in rel] == [NOTE, NOTE]
    # composes with the modes: hybrid and lexical candidates, relevance by the embedding
    for mode in ("hybrid", "lexical"):
        h = idx.post("/api/search", json={**body, "search_type": "mmr", "fetch_k": 6, "search_mode": mode}).json()
        assert len(h) == 2 and len({x["text"] for x in h}) == 2, mode
    qa = TestClient(stack.qa_app)
    k = stack.pipeline.k
    q = {"question": NOTE, "patient_id": "A", "include_knowledge_base": False}
    a = qa.post("/ask/", json=q)
    # (the tiny encoder's embeddings all lie close together: a small lambda_mult keeps the
    # second upload behind every other note)
    b = qa.post("/ask/", json={**q, "search_type": "mmr", "fetch_k": 6, "lambda_mult": 0.1})
    assert a.status_code == b.status_code == 200
    ta, tb = _texts(stack, a.json()["sources"]), _texts(stack, b.json()["sources"])
    assert len(ta) == len(tb) == k and ta[:2] == [NOTE, NOTE]
    assert len(set(tb)) == k                                            # every prompt slot a different text


def test_service_422s(stack):
    from fastapi.testclient import TestClient

    idx, qa = TestClient(stack.indexer_app), TestClient(stack.qa_app)
    for bad in ({"search_type": "diverse"}, {"search_type": "mmr", "lambda_mult": 1.5},
                {"search_type": "mmr", "lambda_mult": -0.1}, {"search_type": "mmr", "fetch_k": 0}):
        assert idx.post("/api/search", json={"query": "x", **bad}).status_code == 422, bad
        assert qa.post("/ask/", json={"question": "x", **bad}).status_code == 422, bad


def test_env_defaults(monkeypatch):
    from docqa_amd.config import Settings, mmr_request

    for v in ("RETRIEVAL_SEARCH_TYPE", "MMR_LAMBDA", "MMR_FETCH_K"):
        monkeypatch.delenv(v, raising=False)
    st = Settings()
    assert (st.retrieval_search_type, st.mmr_lambda, st.mmr_fetch_k) == ("similarity", 0.5, 20)
    assert mmr_request(None, None, None, st) is None
    assert mmr_request("mmr", None, None, st) == (0.5, 20)
    assert mmr_request("mmr", 0.25, 7, st) == (0.25, 7)
    monkeypatch.setenv("RETRIEVAL_SEARCH_TYPE", "mmr")
    monkeypatch.setenv("MMR_LAMBDA", "0.75")
    monkeypatch.setenv("MMR_FETCH_K", "12")
    st = Settings()
    assert mmr_request(None, None, None, st) == (0.75, 12)
    assert mmr_request("similarity", None, None, st) is None             # the request's own wins
    monkeypatch.setenv("RETRIEVAL_SEARCH_TYPE", "fuzzy")
    with pytest.raises(ValueError):
        mmr_request(None, None, None, Settings())


def test_env_default_serves_mmr(stack, monkeypatch):
    from fastapi.testclient import TestClient

    monkeypatch.setattr(stack.indexer.st, "retrieval_search_type", "mmr")
    monkeypatch.setattr(stack.indexer.st, "mmr_fetch_k", 6)
    body = {"query": NOTE, "k": 2, "patient_id": "A", "include_knowledge_base": False}
    hits = TestClient(stack.indexer_app).post("/api/search", json=body).json()
    assert len({h["text"] for h in hits}) == 2
    hits = TestClient(stack.indexer_app).post("/api/search", json={**body, "search_type": "similarity"}).json()
    assert [h["text"] for h in hits] == [NOTE, NOTE]


def test_router_payload_carries_the_fields(stack):
    """The front end resolves the defaults and forwards LangChain's three fields; the local
    replica's batcher payload carries (lambda_mult, fetch_k)."""
    import asyncio
    import concurrent.futures as cf

    from docqa_amd.services.qa import ReplicaRouter, _ask_parts, ask_payload

    assert ask_payload("q", None, "dense", None) == "q"
    p = ask_payload("q", None, "dense", (0.25, 9))
    assert p["mmr"] == (0.25, 9)
    qs, scopes, modes, mmr = _ask_parts([("ask", "plain", None, 0.0), ("ask", p, None, 0.0)])
    assert qs == ["plain", "q"] and scopes is None and modes is None and mmr == [None, (0.25, 9)]
    assert _ask_parts([("ask", "plain", None, 0.0)])[3] is None

    sent = {}

    class Local:
        def submit(self, kind, payload):
            sent["local"] = payload
            f = cf.Future()
            f.set_result({"answer": "", "sources": []})
            return f

    class Client:
        async def post(self, url, json):
            sent["remote"] = json

            class R:
                status_code = 200

                def json(self):
                    return {"answer": "", "sources": []}
            return R()

    r = ReplicaRouter(Local(), ["http://other:8004"])
    r.client = Client()
    wire = {"question": "q", "search_type": "mmr", "lambda_mult": 0.25, "fetch_k": 9}

    async def both():
        await r.call("ask", "/ask/", dict(wire), "question")
        await r.call("ask", "/ask/", dict(wire), "question")
    asyncio.run(both())
    assert sent["remote"] == wire
    assert sent["local"]["mmr"] == (0.25, 9) and sent["local"]["question"] == "q"


def test_sharded_index_is_422(stack, monkeypatch):
    from fastapi.testclient import TestClient

    def refuse(*a, **k):
        raise NotImplementedError("sharded")
    monkeypatch.setattr(stack.indexer.index, "mmr_select", refuse, raising=False)
    r = TestClient(stack.indexer_app).post("/api/search", json={"query": "x", "search_type": "mmr"})
    assert r.status_code == 422
    monkeypatch.setattr(stack.pipeline.index, "check_gather", lambda: None, raising=False)
    r = TestClient(stack.qa_app).post("/ask/", json={"question": "x", "search_type": "mmr"})
    assert r.status_code == 422


@pytest.mark.parametrize("serving", ["batch", "continuous"])
def test_default_path_never_reaches_mmr(tmp_path, monkeypatch, serving):
    """With ``ops.mmr_select`` raising, a request without the fields is served through either
    batcher, with the hits of the plain search."""
    from fastapi.testclient import TestClient

    from docqa_amd import ops
    from docqa_amd.index.scope import scope_request

    for v in ("RETRIEVAL_SEARCH_TYPE", "MMR_LAMBDA", "MMR_FETCH_K"):
        monkeypatch.delenv(v, raising=False)
    s = _make_stack(tmp_path, serving=serving)
    try:
        def boom(*a, **k):
            raise AssertionError("mmr_select on the default path")
        monkeypatch.setattr(ops, "mmr_select", boom)
        q = {"question": NOTE, "patient_id": "A", "include_knowledge_base": False}
        r = TestClient(s.qa_app).post("/ask/", json=q)
        assert r.status_code == 200
        sc = [scope_request("A", None, None, False)]
        D, I = s.pipeline.retrieve([NOTE], scopes=sc)
        D2, I2 = s.pipeline.retrieve([NOTE], scopes=sc, mmr=[None])
        assert torch.equal(I, I2) and torch.equal(D, D2)
        assert r.json()["sources"] == [s.pipeline.metadata[i].get("source") for i in I[0].tolist() if i >= 0]
        body = {"query": NOTE, "k": 2}
        assert TestClient(s.indexer_app).post("/api/search", json=body).status_code == 200
        with pytest.raises(Exception):
            s.pipeline.retrieve([NOTE], mmr=[(0.5, 6)])                 # the patched op is what MMR reaches
    finally:
        s.close()
