"""Lexical (BM25) and hybrid retrieval on the CPU path: the analyzer, the term columns, the
fp32 references of ``ops.bm25_topk`` / ``ops.rank_fuse`` against fp64 / exact-rational
computations written out here, and the services with the tiny models."""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from docqa_amd.index.lexical import LexicalColumns
from docqa_amd.ops import reference as ref
from docqa_amd.text import lexical as lx

PAD = -1            # 0xFFFFFFFF as int32
FLT_MAX = 3.4028234663852886e38


# ------------------------------------------------------------------ analyzer
def test_analyzer_folds_accents_and_case():
    a, b, c = lx.analyze("Éphédra"), lx.analyze("ephedra"), lx.analyze("EPHEDRA")
    assert a == b == c and len(a) == 1 and a[0][1] == 1
    assert lx.analyze("Éphédra ephedra, EPHEDRA!") == [(a[0][0], 3)]


def test_analyzer_stop_words_digits_and_lengths():
    toks = lx.tokens("Le patient est sous 5 mg de warfarine et à jeun ; INR 2 x " + "z" * 65)
    assert toks == ["patient", "5", "mg", "warfarine", "jeun", "inr", "2"]
    assert lx.analyze("the of and le la les des") == []
    assert 120 <= len(lx.STOP_WORDS) <= 200
    pairs, dl = lx.analyze_full("aspirine " * 300)
    assert pairs == [(lx.term_of("aspirine"), 255)] and dl == 300      # tf capped, dl not


def test_analyzer_hashes_are_pinned():
    # FNV-1a 32-bit of the UTF-8 bytes: the on-device term format
    assert lx.fnv1a32(b"") == 0x811C9DC5
    assert lx.fnv1a32(b"a") == 0xE40C292C
    assert lx.fnv1a32(b"foobar") == 0xBF9CF968
    assert lx.term_of("ephedra") == lx.fnv1a32(b"ephedra") == lx.analyze("Éphédra")[0][0]
    pairs = lx.analyze("zeta alpha 42")
    assert [h for h, _ in pairs] == sorted(lx.term_of(t) for t in ("zeta", "alpha", "42"))


def test_analyzer_padding_key_is_remapped(monkeypatch):
    monkeypatch.setattr(lx, "fnv1a32", lambda data: 0xFFFFFFFF)
    assert lx.term_of("anything") == 0xFFFFFFFE
    assert lx.analyze("mot autre") == [(0xFFFFFFFE, 2)]


# ------------------------------------------------------------------ columns
def _meta(n, seed=0):
    rng = np.random.default_rng(seed)
    words = [f"mot{i}" for i in range(40)] + ["ginseng", "éphédra", "astragale"]
    out = []
    for i in range(n):
        k = int(rng.integers(0, 30))
        out.append({"text_content": " ".join(rng.choice(words, k)) if i % 7 else "", "type": "knowledge_base"})
    return out


def test_columns_extend_in_slices_equals_rebuild():
    meta = _meta(50)
    a = LexicalColumns("cpu", capacity=4, entry_capacity=8)
    for end in (13, 14, 50):
        a.extend(meta[:end])
    b = LexicalColumns("cpu")
    b.rebuild(meta)
    for name in ("row_ptr", "terms", "tfs", "dl"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.ndocs, a.total_len, a.entries, a.df) == (b.ndocs, b.total_len, b.entries, b.df)
    assert a.ndocs == 50 and a.row_ptr.dtype == torch.int64 and a.terms.dtype == torch.int32
    assert a.tfs.dtype == torch.uint8 and a.dl.dtype == torch.int32
    rp = a.row_ptr.tolist()
    assert rp[0] == 0 and rp[-1] == a.entries == a.terms.numel()
    for r in range(50):
        row = [t & 0xFFFFFFFF for t in a.terms[rp[r]:rp[r + 1]].tolist()]
        assert row == sorted(set(row))                                  # unique, ascending unsigned
        pairs, dl = lx.analyze_full(meta[r]["text_content"])
        assert row == [h for h, _ in pairs] and a.dl[r].item() == dl
    assert rp[1] == 0                                                   # an empty row has no entries
    assert a.stats() == {"rows": 50, "entries": a.entries, "distinct_terms": len(a.df)}


def test_columns_grow_one_row_at_a_time_through_doublings():
    """Every row count from a capacity of 2 up: row_ptr [c + 1] and dl [c] share one capacity,
    so no count falls between their sizes."""
    meta = _meta(70, seed=1)
    a = LexicalColumns("cpu", capacity=2, entry_capacity=2)
    for end in range(1, 71):
        a.extend(meta[:end])
        assert a.n == end and a._row_ptr.shape[0] == a._dl.shape[0] + 1
    b = LexicalColumns("cpu")
    b.rebuild(meta)
    for name in ("row_ptr", "terms", "tfs", "dl"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert (a.total_len, a.entries, a.df) == (b.total_len, b.entries, b.df)
    # the sizes at which the two buffers used to drift apart: 5 rows, then 9, from capacity 4
    c = LexicalColumns("cpu", capacity=4)
    c.extend(meta[:5])
    c.extend(meta[:9])
    assert torch.equal(c.row_ptr, b.row_ptr[:10]) and torch.equal(c.dl, b.dl[:9])


def test_columns_failed_extend_leaves_the_statistics(monkeypatch):
    meta = _meta(20, seed=2)
    a = LexicalColumns("cpu", capacity=4)
    a.extend(meta[:10])
    before = (a.n, a.total_len, a.entries, dict(a.df), a.row_ptr.clone())

    def boom():
        raise RuntimeError("copy failed")

    monkeypatch.setattr(a, "_sync", boom)
    with pytest.raises(RuntimeError):
        a.extend(meta)
    assert (a.n, a.total_len, a.entries, a.df) == before[:4] and torch.equal(a.row_ptr, before[4])
    monkeypatch.undo()
    a.extend(meta)
    b = LexicalColumns("cpu")
    b.rebuild(meta)
    assert a.df == b.df and torch.equal(a.terms, b.terms) and torch.equal(a.row_ptr, b.row_ptr)


def test_query_rows_drop_cap_and_padding():
    meta = [{"text_content": " ".join(f"w{j}" for j in range(i + 1))} for i in range(40)]
    cols = LexicalColumns("cpu")
    cols.rebuild(meta)
    qt, qw, avgdl = cols.query_rows(["w3 w3 inconnu w0", "inconnu", " ".join(f"w{j}" for j in range(40))])
    assert qt.shape == (3, 32) and qt.dtype == torch.int32 and qw.dtype == torch.float32
    assert avgdl == pytest.approx(sum(range(1, 41)) / 40)
    idf = lambda df: math.log(1 + (40 - df + 0.5) / (df + 0.5))  # noqa: E731
    h3, h0 = lx.term_of("w3"), lx.term_of("w0")
    got = {t & 0xFFFFFFFF: w for t, w in zip(qt[0].tolist(), qw[0].tolist()) if t != PAD}
    assert set(got) == {h3, h0}                                         # the unknown term is dropped
    assert got[h3] == np.float32(2 * idf(37)) and got[h0] == np.float32(idf(40))
    assert qt[0, 2:].eq(PAD).all() and qw[0, 2:].eq(0).all()
    assert qt[1].eq(PAD).all() and qw[1].eq(0).all()
    # 40 known terms: the 32 heaviest = the rarest (w8 .. w39), heaviest first
    kept = [t & 0xFFFFFFFF for t in qt[2].tolist()]
    assert set(kept) == {lx.term_of(f"w{j}") for j in range(8, 40)}
    assert qw[2].tolist() == sorted(qw[2].tolist(), reverse=True) and qw[2].min() > 0
    assert kept[0] == lx.term_of("w39")


# ------------------------------------------------------------------ reference ops
def make_columns(N, seed, lens=None, vocab=400):
    """Random CSR columns: Zipf-like terms (hash-like 32-bit values), tf 1..255."""
    rng = np.random.default_rng(seed)
    values = rng.choice(np.arange(1, 1 << 32, 977, dtype=np.int64), vocab, replace=False)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    rows = []
    for r in range(N):
        n = int(lens[r]) if lens is not None else int(rng.integers(0, 121))
        ts = np.unique(rng.choice(values, n, p=p)) if n else np.zeros(0, np.int64)
        rows.append((ts, rng.integers(1, 256, ts.size), int(ts.size + rng.integers(0, 50)) if ts.size else 0))
    return rows, values, p


def pack(rows):
    ptr = np.zeros(len(rows) + 1, np.int64)
    ptr[1:] = np.cumsum([r[0].size for r in rows])
    terms = np.concatenate([r[0] for r in rows] + [np.zeros(0, np.int64)]).astype(np.uint32).view(np.int32)
    tfs = np.concatenate([r[1] for r in rows] + [np.zeros(0, np.int64)]).astype(np.uint8)
    dl = np.array([r[2] for r in rows], np.int32)
    return (torch.from_numpy(ptr), torch.from_numpy(terms.copy()), torch.from_numpy(tfs),
            torch.from_numpy(dl))


def oracle(rows, qterms, qweights, avgdl, k1=1.2, b=0.75, allowed=None):
    """fp64 scores [nq, N] (NaN: the row does not compete) from the formula."""
    nq = len(qterms)
    out = np.full((nq, len(rows)), np.nan)
    for q in range(nq):
        w = {}
        for t, x in zip(qterms[q], qweights[q]):
            if t != 0xFFFFFFFF and t not in w:
                w[int(t)] = float(x)
        for r, (ts, tf, dl) in enumerate(rows):
            if allowed is not None and not allowed[q][r]:
                continue
            K = k1 * (1 - b + b * dl / avgdl)
            hit = [(w[int(t)], float(f)) for t, f in zip(ts, tf) if int(t) in w]
            if hit:
                out[q, r] = sum(wt * f / (f + K) for wt, f in hit)
    return out


def test_reference_bm25_against_fp64():
    rows, values, p = make_columns(137, 3)
    rows[0] = rows[-1] = (np.zeros(0, np.int64), np.zeros(0, np.int64), 0)
    rng = np.random.default_rng(4)
    nq = 9
    qt = np.full((nq, 32), 0xFFFFFFFF, np.int64)
    qw = np.zeros((nq, 32), np.float32)
    for q, T in enumerate((1, 32, 0, 5, 7, 12, 3, 20, 2)):
        qt[q, :T] = rng.choice(values, T, replace=False, p=p)
        qw[q, :T] = rng.uniform(0.1, 9.0, T)
    avgdl = float(np.mean([r[2] for r in rows]))
    want = oracle(rows, qt, qw, avgdl)
    cols = pack(rows)
    k = 10
    S, I = ref.bm25_topk(*cols, torch.from_numpy(qt.astype(np.uint32).view(np.int32)), torch.from_numpy(qw), k, avgdl)
    assert S.dtype == torch.float32 and I.dtype == torch.int64 and S.shape == I.shape == (nq, k)
    for q in range(nq):
        order = sorted((r for r in range(len(rows)) if not np.isnan(want[q, r])), key=lambda r: (-want[q, r], r))
        n = min(k, len(order))
        ids = I[q].tolist()
        assert ids[n:] == [-1] * (k - n) and all(s == -np.float32(FLT_MAX) for s in S[q, n:].tolist())
        assert len(set(ids[:n])) == n and all(not np.isnan(want[q, i]) for i in ids[:n])
        for j in range(n):
            assert abs(S[q, j].item() - want[q, order[j]]) <= 64 * 2.0 ** -24 * want[q, order[j]]
            assert want[q, ids[j]] >= want[q, order[n - 1]] * (1 - 64 * 2.0 ** -24)
    assert I[2].eq(-1).all()                                            # the padding-only query


def _fuse_oracle(a, b, mode, k, c=60):
    score = {}
    for use, ids in ((mode != 1, a), (mode != 0, b)):
        for pos, i in enumerate(ids if use else ()):
            if i >= 0:
                score[i] = score.get(i, Fraction(0)) + Fraction(1, c + pos + 1)
    top = sorted(score.items(), key=lambda kv: (-kv[1], kv[0]))[:k]
    return [i for i, _ in top] + [-1] * (k - len(top)), [s for _, s in top]


def rational_tie_lists():
    """Two 64-long lists in which id 900 sits at ranks (12, 30) and id 100 at (20, 20): both
    score 1/72 + 1/90 = 1/80 + 1/80 = 1/40 at c = 60."""
    a = list(range(1000, 1064))
    b = list(range(2000, 2064))
    a[11], b[29] = 900, 900
    a[19], b[19] = 100, 100
    return a, b


def test_reference_rank_fuse_against_fractions():
    assert Fraction(1, 72) + Fraction(1, 90) == Fraction(1, 80) + Fraction(1, 80) == Fraction(1, 40)
    a, b = rational_tie_lists()
    rng = np.random.default_rng(5)
    A, B = [a], [b]
    for _ in range(6):
        pool = rng.permutation(90)
        la, lb = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        A.append(list(pool[:la]) + [-1] * (64 - la))
        B.append(list(rng.permutation(pool)[:lb]) + [-1] * (64 - lb))
    modes = [2, 0, 1, 2, 2, 2, 2]
    k = 10
    F, I = ref.rank_fuse(torch.tensor(A), torch.tensor(B), torch.tensor(modes, dtype=torch.int32), k)
    for q in range(len(A)):
        ids, scores = _fuse_oracle([int(x) for x in A[q]], [int(x) for x in B[q]], modes[q], k)
        assert I[q].tolist() == ids
        for j, s in enumerate(scores):
            assert F[q, j].item() == np.float32(np.float32(s.numerator) / np.float32(s.denominator))
    top = I[0].tolist()
    assert top[:2] == [100, 900]                                        # the exact tie goes to the lower id
    assert I[1].tolist() == A[1][:k] and I[2].tolist()[:1] == B[2][:1]


def test_sharded_index_refuses():
    from docqa_amd.index.sharded import ShardedIndex

    with pytest.raises(NotImplementedError):
        ShardedIndex.search_lexical(object.__new__(ShardedIndex), None, None, None, 1.0, 3)


# ------------------------------------------------------------------ services (tiny models)
WORD = "zorglubine"


def _make_stack(d, monkeypatch=None):
    from docqa_amd.config import Settings
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = Settings()
    st.index_dir = str(d)
    st.default_data_dir = str(d / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 2
    s = DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu", max_batch=4,
                                max_context=1024, use_graphs=False, services=("indexer", "qa")), st)
    for pid in ("A", "B"):
        for j in range(6):
            extra = f" Traitement par {WORD} 5 mg." if (pid, j) == ("B", 4) else ""
            s.indexer.index_document(f"{pid}{j}", f"Note {j} du patient {pid} : tension stable, bilan normal.{extra}",
                                     {"patient_id": pid, "note_date": f"2024-01-{j + 1:02d}"})
    return s


@pytest.fixture(scope="module")
def stack(tmp_path_factory):
    s = _make_stack(tmp_path_factory.mktemp("lexstack"))
    yield s
    s.close()


def test_service_lexical_and_hybrid_find_the_word(stack):
    from fastapi.testclient import TestClient

    idx = TestClient(stack.indexer_app)
    assert idx.get("/api/index/stats").json()["lexical"] is None        # built lazily
    target = next(i for i, m in enumerate(stack.indexer.metadata) if WORD in m["text_content"])
    hits = idx.post("/api/search", json={"query": f"posologie {WORD}", "k": 3, "search_mode": "lexical"}).json()
    assert hits[0]["id"] == target and hits[0]["score"] > 0
    assert all(h["score"] <= hits[0]["score"] for h in hits)
    hyb = idx.post("/api/search", json={"query": f"posologie {WORD}", "k": 3, "search_mode": "hybrid"}).json()
    assert target in [h["id"] for h in hyb] and len(hyb) == 3
    assert all(0 < h["score"] <= 2 / 61 for h in hyb)
    lexstats = idx.get("/api/index/stats").json()["lexical"]
    assert lexstats["rows"] == len(stack.indexer.metadata) and lexstats["entries"] > 0 < lexstats["distinct_terms"]
    # the pipeline: lexical retrieval puts the chunk first, hybrid within k; a mixed batch
    qs = [f"posologie {WORD}"] * 3
    D, I = stack.pipeline.retrieve(qs, modes=["lexical", "hybrid", "dense"])
    Dd, Id = stack.pipeline.retrieve(qs[:1])
    assert I[0, 0].item() == target and target in I[1].tolist()
    # (the dense leg ran at the fetch depth: the same distances up to the GEMM's blocking)
    assert I[2].tolist() == Id[0].tolist() and torch.allclose(D[2], Dd[0], rtol=1e-5, atol=1e-6)
    qa = TestClient(stack.qa_app)
    r = qa.post("/ask/", json={"question": f"Quelle dose de {WORD} ?", "search_mode": "lexical"})
    assert r.status_code == 200 and r.json()["sources"][0] == "Dossier Patient B4"


def test_service_lexical_with_patient_scope(stack):
    from fastapi.testclient import TestClient

    idx = TestClient(stack.indexer_app)
    hits = idx.post("/api/search", json={"query": "note patient tension bilan", "k": 50, "search_mode": "lexical",
                                         "patient_id": "A"}).json()
    assert hits
    for h in hits:
        m = stack.indexer.metadata[h["id"]]
        assert m.get("type") != "patient_file" or m.get("patient_id") == "A"
    assert sum(stack.indexer.metadata[h["id"]].get("patient_id") == "A" for h in hits) == 6
    none = idx.post("/api/search", json={"query": WORD, "k": 5, "search_mode": "lexical", "patient_id": "A"}).json()
    assert none == []                                                   # the word is patient B's


def test_service_unknown_mode_is_422(stack):
    from fastapi.testclient import TestClient

    assert TestClient(stack.indexer_app).post(
        "/api/search", json={"query": "x", "search_mode": "fuzzy"}).status_code == 422
    assert TestClient(stack.qa_app).post("/ask/", json={"question": "x", "search_mode": "fuzzy"}).status_code == 422


def test_service_without_the_field_is_unchanged(stack, tmp_path, monkeypatch):
    from fastapi.testclient import TestClient

    monkeypatch.delenv("RETRIEVAL_MODE", raising=False)
    other = _make_stack(tmp_path)
    try:
        stack.indexer.ensure_lexical()          # the first stack has served lexical requests
        body = {"query": "tension stable du patient B", "k": 5}
        a = TestClient(stack.indexer_app).post("/api/search", json=body).json()
        b = TestClient(other.indexer_app).post("/api/search", json=body).json()
        assert a == b and len(a) == 5
        assert other.indexer.lexical is None and other.pipeline.lexical is None
        q = {"question": "Quelle est la tension du patient B ?"}
        ra = TestClient(stack.qa_app).post("/ask/", json=q).json()
        rb = TestClient(other.qa_app).post("/ask/", json=q).json()
        assert ra["sources"] == rb["sources"] and other.pipeline.lexical is None
        dense = TestClient(other.indexer_app).post("/api/search", json={**body, "search_mode": "dense"}).json()
        assert dense == b and other.indexer.lexical is None
    finally:
        other.close()


def test_service_columns_follow_later_adds(tmp_path):
    from fastapi.testclient import TestClient

    s = _make_stack(tmp_path)
    try:
        idx = TestClient(s.indexer_app)
        assert idx.post("/api/search", json={"query": "xylophane", "k": 2, "search_mode": "lexical"}).json() == []
        s.indexer.index_document("C0", "Nouvelle note avec du xylophane.", {"patient_id": "C"})
        assert idx.get("/api/index/stats").json()["lexical"]["rows"] == len(s.indexer.metadata)
        new = idx.post("/api/search", json={"query": "xylophane", "k": 2, "search_mode": "lexical"}).json()
        assert len(new) == 1 and "xylophane" in new[0]["text"]
    finally:
        s.close()


def test_index_follower_keeps_lexical_columns(tmp_path):
    """A follower builds the columns on the first request, extends them on every poll, rebuilds
    them on a snapshot reload, and builds them at start with LEXICAL_INDEX=1."""
    from docqa_amd.config import Settings
    from docqa_amd.index.follower import IndexFollower
    from docqa_amd.models.bert import BertConfig, BertEncoder
    from docqa_amd.services.indexer import SemanticIndexer
    from docqa_amd.text.tokenizer import WordPieceTokenizer

    st = Settings()
    st.index_dir = str(tmp_path)
    st.default_data_dir = str(tmp_path / "nodata")
    st.snapshot_every = 100
    enc = BertEncoder(BertConfig.preset("tiny-bert"), device="cpu")
    w = SemanticIndexer(enc, WordPieceTokenizer(), st, device="cpu").startup(build_if_missing=True)
    f = IndexFollower(str(tmp_path), d=enc.cfg.hidden, device="cpu")
    f.poll()
    assert f.lexical is None                                            # lazily

    def first_hit(fol, word):
        cols = fol.ensure_lexical()
        qt, qw, avgdl = cols.query_rows([word])
        _, I = fol.index.search_lexical(cols, qt, qw, avgdl, 3)
        return [fol.metadata[i]["source"] for i in I[0].tolist() if i >= 0]

    assert first_hit(f, WORD) == [] and f.lexical.n == len(f.metadata)
    w.index_document(7, f"Traitement par {WORD}.", {"patient_id": "P"})     # a WAL frame
    assert f.poll() == 1 and f.lexical.n == f.index.ntotal == len(f.metadata)
    assert first_hit(f, WORD) == ["Dossier Patient 7"]
    w.save_state()                                                      # snapshot: the follower reloads
    w.index_document(8, "Arrêt du xylophane.", {"patient_id": "P"})
    f.poll()
    ref_cols = LexicalColumns("cpu")
    ref_cols.rebuild(w.metadata)
    assert f.lexical.df == ref_cols.df and torch.equal(f.lexical.terms, ref_cols.terms)
    assert torch.equal(f.lexical.row_ptr, ref_cols.row_ptr) and first_hit(f, "xylophane") == ["Dossier Patient 8"]
    st.lexical_index = True
    g = IndexFollower(str(tmp_path), d=enc.cfg.hidden, device="cpu", settings=st).start()
    try:
        assert g.lexical is not None and g.lexical.n == len(g.metadata) and first_hit(g, WORD) == ["Dossier Patient 7"]
    finally:
        g.stop()
