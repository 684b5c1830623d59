"""The BM25 scan kernel (csrc/kernels/lexical.hip, ``ops.bm25_topk``) against an fp64
implementation of the formula written out here (``oracle``).

Inputs are made on the CPU with fixed seeds: row lengths 0..120 entries, terms Zipf-like from
400 values (most (query, row) pairs share a term, many share several), tf 1..255.  Row counts:
1, 31, 33, 129, 513, 1100 and the kernel's own seams -- 255 / 256 / 257 (the 256-row tile =
one row block; 1 once more with its row not empty), 262401 (over 1024 row blocks: 512-row blocks of two tile passes, the last
block half full, and blocks past the end that hold nothing); nq 1 / 33 / 70 (the 32-query
workgroup), k 1 / 3 / 10 / 64 (every padded K but 8 and 32, which 5 and 20 add).

Tolerance: 64 x 2^-24 relative -- every term is positive, so a relative bound holds; one
rounding each for w, the operations of K_r, the add, the divide and the multiply, plus T - 1
for the sum at T <= 32 terms is about 41 units of 2^-24.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMIN, IMAX = -(1 << 31), (1 << 31) - 1
FMAX = float(np.float32(3.4028234663852886e38))
PADKEY = 0xFFFFFFFF
TOL = 64 * 2.0 ** -24
VOCAB = 400


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops.native_loaded()
    return ops


def _vocab(rng):
    values = rng.choice(np.arange(1, PADKEY, 977, dtype=np.int64), VOCAB, replace=False)
    p = 1.0 / np.arange(1, VOCAB + 1)
    return values, p / p.sum()


def make_rows(N, seed, maxlen=120, long_row=None, twins=0):
    """CSR columns as numpy arrays (ptr, row_of, terms uint32-valued int64, tf, dl).  First and
    last row empty; ``long_row``: that row gets 300 entries; ``twins``: rows 3 i + 1 copy rows
    3 i (entries and dl) for i < twins."""
    rng = np.random.default_rng(seed)
    values, p = _vocab(rng)
    lens = rng.integers(0, maxlen + 1, N)
    lens[0] = lens[-1] = 0
    row = np.repeat(np.arange(N, dtype=np.int64), lens)
    t = rng.choice(values, row.size, p=p)
    if long_row is not None:
        keep = row != long_row
        row = np.concatenate([row[keep], np.full(300, long_row, np.int64)])
        t = np.concatenate([t[keep], rng.choice(values, 300, replace=False)])
    key = np.unique(row * (1 << 32) + t)           # by row, then by unsigned term; unique per row
    row, t = key >> 32, key & PADKEY
    tf = rng.integers(1, 256, row.size)
    counts = np.bincount(row, minlength=N)
    dl = np.where(counts > 0, counts + rng.integers(0, 50, N), 0)
    for i in range(twins):
        a, b = 3 * i, 3 * i + 1
        if b >= N:
            break
        ka, kb = row == a, row != b
        row = np.concatenate([row[kb], np.full(int(ka.sum()), b, np.int64)])
        t, tf = np.concatenate([t[kb], t[ka]]), np.concatenate([tf[kb], tf[ka]])
        dl[b] = dl[a]
        o = np.argsort(row * (1 << 32) + t, kind="stable")
        row, t, tf = row[o], t[o], tf[o]
    ptr = np.zeros(N + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(row, minlength=N))
    return {"N": N, "ptr": ptr, "row": row, "t": t, "tf": tf, "dl": dl, "values": values, "p": p}


def make_queries(c, nq, seed):
    """Query rows: 1 term, 32 terms, padding only, then random 2..31 terms; weights 0.05..9."""
    rng = np.random.default_rng(seed)
    qt = np.full((nq, 32), PADKEY, np.int64)
    qw = np.zeros((nq, 32), np.float32)
    for q in range(nq):
        T = (1, 32, 0)[(q + seed) % 3] if q < 3 else int(rng.integers(2, 32))
        qt[q, :T] = rng.choice(c["values"], T, replace=False, p=c["p"])
        qw[q, :T] = rng.uniform(0.05, 9.0, T)
    return qt, qw


def oracle(c, qt, qw, avgdl, k1=1.2, b=0.75, allowed=None):
    """fp64 BM25 from the formula: (scores [nq, N], competes bool [nq, N])."""
    N, nq = c["N"], qt.shape[0]
    K = k1 * (1 - b + b * c["dl"].astype(np.float64) / avgdl)
    x = c["tf"] / (c["tf"] + K[c["row"]])
    score = np.zeros((nq, N))
    comp = np.zeros((nq, N), bool)
    for q in range(nq):
        real = qt[q] != PADKEY
        if not real.any() or c["t"].size == 0:
            continue
        o = np.argsort(qt[q][real])
        st, sw = qt[q][real][o], qw[q][real][o].astype(np.float64)
        pos = np.minimum(np.searchsorted(st, c["t"]), st.size - 1)
        hit = st[pos] == c["t"]
        score[q] = np.bincount(c["row"][hit], weights=sw[pos[hit]] * x[hit], minlength=N)
        comp[q] = np.bincount(c["row"][hit], minlength=N) > 0
    if allowed is not None:
        comp &= allowed
    return score, comp


def to_device(c, qt, qw):
    i32 = lambda a: torch.from_numpy(a.astype(np.uint32).view(np.int32).copy())  # noqa: E731
    cols = (torch.from_numpy(c["ptr"]), i32(c["t"]), torch.from_numpy(c["tf"].astype(np.uint8)),
            torch.from_numpy(c["dl"].astype(np.int32)))
    return [x.cuda() for x in cols], i32(qt).reshape(-1, 32).cuda(), torch.from_numpy(qw).cuda()


def check(S, I, score, comp, k, id_offset=0):
    """Every property of a result against the oracle; prints the worst figures first."""
    S, I = S.cpu().numpy().astype(np.float64), I.cpu().numpy()
    nq, N = score.shape
    assert S.shape == I.shape == (nq, k)
    worst_rank = worst_row = 0.0
    for q in range(nq):
        order = sorted(np.flatnonzero(comp[q]), key=lambda r: (-score[q, r], r))
        n = min(k, len(order))
        ids = I[q, :n] - id_offset
        assert (I[q, n:] == -1).all() and (S[q, n:] == -FMAX).all(), (q, n, I[q], S[q])
        assert len(set(ids.tolist())) == n and ((0 <= ids) & (ids < N)).all(), (q, I[q])
        assert comp[q, ids].all(), (q, ids)                     # in scope and sharing a term
        assert (np.diff(S[q, :n]) <= 0).all()
        if n:
            want = score[q, order[:n]]
            worst_rank = max(worst_rank, float(np.max(np.abs(S[q, :n] - want) / want)))
            worst_row = max(worst_row, float(np.max((want[-1] - score[q, ids]) / want[-1])))
    print(f"worst rel. error at rank {worst_rank / 2.0 ** -24:.2f} x 2^-24, "
          f"worst returned-row deficit {worst_row / 2.0 ** -24:.2f} x 2^-24")
    assert worst_rank <= TOL and worst_row <= TOL


CASES = [(1, 1, 1), (31, 33, 3), (33, 70, 10), (129, 1, 64), (255, 33, 64), (256, 70, 3), (257, 1, 10),
         (513, 33, 1), (1100, 70, 64), (1100, 33, 5), (513, 70, 20)]


@pytest.mark.parametrize("N,nq,k", CASES)
def test_bm25_topk_matches_fp64(native, N, nq, k):
    c = make_rows(N, seed=N + nq, long_row=N // 2 if N >= 129 else None, twins=5)
    qt, qw = make_queries(c, nq, seed=k)
    avgdl = float(max(c["dl"].mean(), 1.0))
    score, comp = oracle(c, qt, qw, avgdl)
    assert PADKEY not in c["t"]
    cols, dqt, dqw = to_device(c, qt, qw)
    S, I = native.bm25_topk(*cols, dqt, dqw, k, avgdl)
    assert S.is_cuda and S.dtype == torch.float32 and I.dtype == torch.int64
    check(S, I, score, comp, k)
    if nq >= 3:
        pad = [(q + k) % 3 == 2 for q in range(3)].index(True)      # the padding-only query
        assert (I[pad] == -1).all()


def test_bm25_topk_over_1024_blocks_and_id_offset(native):
    N = 262144 + 257
    c = make_rows(N, seed=7, maxlen=6)
    qt, qw = make_queries(c, 4, seed=1)
    avgdl = float(c["dl"].mean())
    score, comp = oracle(c, qt, qw, avgdl)
    cols, dqt, dqw = to_device(c, qt, qw)
    off = 5_000_000_000
    S, I = native.bm25_topk(*cols, dqt, dqw, 10, avgdl, id_offset=off)
    check(S, I, score, comp, 10, id_offset=off)


def test_bm25_topk_exact_ties_go_to_the_lower_row(native):
    """Rows 3 i and 3 i + 1 are identical, so their scores are: with k cutting between them
    the lower row is returned and its twin is not."""
    c = make_rows(600, seed=11, twins=200)
    qt, qw = make_queries(c, 8, seed=1)
    avgdl = float(c["dl"].mean())
    score, comp = oracle(c, qt, qw, avgdl)
    cols, dqt, dqw = to_device(c, qt, qw)
    cut = 0
    for q in range(8):
        order = sorted(np.flatnonzero(comp[q]), key=lambda r: (-score[q, r], r))
        s = score[q, order]
        for j in range(1, min(63, len(order) - 2)):
            a, b = order[j], order[j + 1]
            # a twin pair clear of its neighbours by far more than the tolerance
            if a % 3 == 0 and b == a + 1 and s[j - 1] > s[j] * 1.001 and s[j + 1] > s[j + 2] * 1.001:
                k = j + 1
                S, I = native.bm25_topk(*cols, dqt[q:q + 1], dqw[q:q + 1], k, avgdl)
                ids = I[0].tolist()
                assert ids[-1] == a and b not in ids, (q, k, ids)
                S2, I2 = native.bm25_topk(*cols, dqt[q:q + 1], dqw[q:q + 1], k + 1, avgdl)
                assert I2[0].tolist()[-2:] == [a, b] and S2[0, -1] == S2[0, -2]     # bit-identical scores
                cut += 1
                break
    assert cut >= 3


def test_bm25_topk_single_row_with_a_hit(native):
    """N = 1 whose only row holds entries (the parametrised N = 1 case has it empty)."""
    rng = np.random.default_rng(41)
    values, p = _vocab(rng)
    t = np.sort(rng.choice(values, 7, replace=False))
    c = {"N": 1, "ptr": np.array([0, 7], np.int64), "row": np.zeros(7, np.int64), "t": t,
         "tf": rng.integers(1, 256, 7), "dl": np.array([9]), "values": values, "p": p}
    qt = np.full((2, 32), PADKEY, np.int64)
    qw = np.zeros((2, 32), np.float32)
    qt[0, :3], qw[0, :3] = t[[1, 4, 6]], (0.5, 2.0, 7.0)
    qt[1, :2], qw[1, :2] = np.setdiff1d(values, t)[:2], (1.0, 1.0)         # shares nothing
    score, comp = oracle(c, qt, qw, 9.0)
    assert comp.tolist() == [[True], [False]]
    cols, dqt, dqw = to_device(c, qt, qw)
    for k in (1, 3):
        S, I = native.bm25_topk(*cols, dqt, dqw, k, 9.0)
        check(S, I, score, comp, k)
        assert I[0, 0].item() == 0 and (I[1] == -1).all()


def test_bm25_topk_scoped_with_decoys(native):
    """Every row outside a query's scope holds all of that query's terms at tf 255 (a row
    outside several scopes holds the terms of each): unscoped, such rows fill the top of the
    list, and the scope must keep every one of them out.  Four kinds of scope: a tag, a tag
    plus the tag-0 rows, a date window over any tag, tag 0 with an upper bound only."""
    N, nq, k = 700, 8, 10
    c = make_rows(N, seed=21)
    qt, qw = make_queries(c, nq, seed=2)
    rng = np.random.default_rng(3)
    tags = rng.integers(0, 3, N).astype(np.int32)
    days = (737000 + rng.integers(0, 100, N)).astype(np.int32)
    days[rng.random(N) < 0.2] = IMIN
    scope = np.array([[(1, -1, IMIN, IMAX), (1, 0, IMIN, IMAX), (-1, -1, 737020, 737060),
                       (0, -1, IMIN + 1, 737050)][q % 4] for q in range(nq)], np.int32)
    tg, al, lo, hi = (scope[:, j:j + 1] for j in range(4))
    allowed = (tags[None] == al) | (((tg < 0) | (tags[None] == tg)) & (lo <= days[None]) & (days[None] <= hi))
    assert allowed.any(1).all() and (~allowed).sum(1).min() >= k
    decoy = [((np.flatnonzero(~allowed[q])[:, None] << 32) + qt[q][qt[q] != PADKEY][None]).ravel() for q in range(nq)]
    decoy = np.unique(np.concatenate(decoy))
    have = (c["row"] << 32) + c["t"]
    keys = np.union1d(have, decoy)
    tf = np.empty(keys.size, np.int64)
    tf[np.searchsorted(keys, have)] = c["tf"]
    tf[np.searchsorted(keys, decoy)] = 255
    c["row"], c["t"], c["tf"] = keys >> 32, keys & PADKEY, tf
    c["ptr"][1:] = np.cumsum(np.bincount(c["row"], minlength=N))
    avgdl = float(c["dl"].mean())
    score, comp = oracle(c, qt, qw, avgdl, allowed=allowed)
    unscoped, ucomp = oracle(c, qt, qw, avgdl)
    for q in range(nq):                 # a query with terms: every out-of-scope row competes unscoped,
        if (qt[q] != PADKEY).any():     # and for the 32-term queries they fill the whole top k
            assert ucomp[q, ~allowed[q]].all()
            if (qt[q] != PADKEY).all():
                assert not allowed[q, np.argsort(-unscoped[q])[:k]].any()
    cols, dqt, dqw = to_device(c, qt, qw)
    S, I = native.bm25_topk(*cols, dqt, dqw, k, avgdl, tags=torch.from_numpy(tags).cuda(),
                            days=torch.from_numpy(days).cuda(), scope=torch.from_numpy(scope).cuda())
    check(S, I, score, comp, k)
    ids = I.cpu().numpy()
    for q in range(nq):
        assert allowed[q, ids[q][ids[q] >= 0]].all()


def test_bm25_kill_switch_and_out_of_envelope_take_the_reference(native, monkeypatch):
    c = make_rows(300, seed=31)
    qt, qw = make_queries(c, 5, seed=0)
    avgdl = float(c["dl"].mean())
    score, comp = oracle(c, qt, qw, avgdl)
    cols, dqt, dqw = to_device(c, qt, qw)
    want = native.bm25_topk(*cols, dqt, dqw, 10, avgdl)

    def no_native():
        raise AssertionError("the native kernel was called")

    monkeypatch.setattr(native, "_native", no_native)
    S70, I70 = native.bm25_topk(*cols, dqt, dqw, 70, avgdl)            # k past the envelope
    assert S70.is_cuda and S70.shape == (5, 70)
    check(S70, I70, score, comp, 70)
    wide = [cols[0], cols[1], cols[2].int(), cols[3]]                  # tfs not uint8: the reference too
    check(*native.bm25_topk(*wide, dqt, dqw, 10, avgdl), score, comp, 10)
    monkeypatch.setenv("DOCQA_BM25", "0")
    S, I = native.bm25_topk(*cols, dqt, dqw, 10, avgdl)
    assert S.is_cuda
    check(S, I, score, comp, 10)
    assert torch.allclose(S, want[0], rtol=2 * TOL, atol=0)


def test_indexer_lexical_and_hybrid_on_the_device_match_the_cpu_path(native, tmp_path):
    from docqa_amd.config import Settings
    from docqa_amd.models.bert import BertConfig, BertEncoder
    from docqa_amd.services.indexer import SemanticIndexer
    from docqa_amd.text.tokenizer import WordPieceTokenizer

    rng = np.random.default_rng(5)
    words = [f"terme{i}" for i in range(60)] + ["warfarine", "éphédra", "INR", "K50"]
    notes = [" ".join(rng.choice(words, int(rng.integers(3, 40)))) for _ in range(300)]
    out = {}
    for dev in ("cpu", "cuda"):
        st = Settings()
        st.index_dir = str(tmp_path / dev)
        st.index_wal = False
        ix = SemanticIndexer(BertEncoder(BertConfig.preset("tiny-bert"), device=dev), WordPieceTokenizer(), st,
                             device=dev)
        ix.add_records([{"doc_id": str(i), "text_content": t, "source": f"n{i}", "type": "patient_file",
                         "patient_id": str(i % 3)} for i, t in enumerate(notes)])
        res = {}
        for query in ("warfarine INR", "ephedra terme3 terme7 terme11", "K50"):
            for mode in ("dense", "lexical", "hybrid"):
                res[query, mode] = ix.search(query, 5, mode=mode)
                res[query, mode + "@20"] = ix.search(query, 20, mode=mode)     # hybrid's legs at k = 5
            res[query, "scoped"] = ix.search(query, 5, {"patient_id": "1", "from_date": None, "to_date": None,
                                                        "include_knowledge_base": True}, "lexical")
        out[dev] = res
        assert ix.lexical.device.type == dev
    ids = lambda hits: [h["id"] for h in hits]  # noqa: E731
    checked = 0
    for key, cpu in out["cpu"].items():
        gpu = out["cuda"][key]
        sc = [h["score"] for h in cpu]
        if key[1] in ("lexical", "scoped"):
            assert len(cpu) == len(gpu) > 0
            assert np.allclose([h["score"] for h in gpu], sc, rtol=2 * TOL, atol=0)
            if all(a - b > 4 * TOL * a for a, b in zip(sc, sc[1:])):       # exact away from ties
                assert ids(gpu) == ids(cpu), key
                checked += 1
            if key[1] == "scoped":
                assert all(int(i) % 3 == 1 for i in ids(gpu))
        elif key[1] == "hybrid":
            assert len(gpu) == 5 and all(0 < h["score"] <= 2 / 61 for h in gpu)
            q = key[0]
            if all(ids(out["cpu"][q, leg]) == ids(out["cuda"][q, leg]) for leg in ("dense@20", "lexical@20")):
                assert ids(gpu) == ids(cpu) and [h["score"] for h in gpu] == sc, key
                checked += 1
    assert checked >= 2
