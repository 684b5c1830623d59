"""``ops.mmr_select`` on the GPU (csrc/kernels/mmr.hip, one workgroup per query) against an
fp64 numpy oracle written out here, computed from the stored values (bf16 widened exactly).

1. Replay on general data: given the kernel's own first t picks, its pick t scores within
   ``tol`` of the fp64 maximum over the remaining valid candidates, and S is within ``tol`` of
   that fp64 score.  ``tol = 4 * (d + 8) * 2^-24``: an fp32 dot of d terms in any order is off
   by at most d 2^-24 |a||b|, so a cosine is off by d 2^-24 from its dot and as much again
   from the fp32 norms; a score is a convex mix of two cosines and a comparison involves two
   scores; the + 8 covers the square root, the divide and the mix.
2. Exact arithmetic (rows of 16 entries +-1, lam a multiple of 1/4): P and I equal the fp64
   greedy pick bit for bit, ties to the earlier position.
3. Outside the envelope and with the kill switch: identical to ``ops.reference.mmr_select``.
4. ``FlatIndex`` / ``IVFPQRefineIndex.mmr_select`` and ``RAGPipeline.search(..., mmr=...)``.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LAMS = (0.0, 0.25, 0.5, 0.9, 1.0, -1.0)
EXACT_LAMS = (0.0, 0.25, 0.5, 0.75, 1.0)


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    return ops


# ------------------------------------------------------------------ fp64 oracle
def cosines64(rows, q):
    """rel [F] and sim [F, F] in fp64 from the stored values; 0 where a norm is 0."""
    rows, q = rows.astype(np.float64), q.astype(np.float64)
    n = (rows * rows).sum(1)
    qn = float(q @ q)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = np.sqrt(n * qn)
        rel = np.where(den > 0, (rows @ q) / np.where(den > 0, den, 1.0), 0.0)
        den = np.sqrt(n[:, None] * n[None, :])
        sim = np.where(den > 0, (rows @ rows.T) / np.where(den > 0, den, 1.0), 0.0)
    return rel, sim


def scores64(rel, sim, lam, picked):
    """The fp64 score of every position, given the picks so far."""
    if not picked:
        return rel.copy()
    return lam * rel - (1.0 - lam) * sim[:, picked].max(1)


def greedy64(rel, sim, lam, valid, k):
    """LangChain's loop: strict >, so ties go to the earlier position."""
    picked, scores = [], []
    left = np.zeros(len(rel), bool)
    left[valid] = True
    while len(picked) < min(k, len(valid)):
        s = np.where(left, scores64(rel, sim, lam, picked), -np.inf)
        p = int(np.argmax(s))                       # the first maximum
        picked.append(p)
        scores.append(float(s[p]))
        left[p] = False
    return picked, scores


def replay(xb64, xq, cand, ncand, lam, k, S, I, P, tol):
    """Every pick, given the picks before it, is within ``tol`` of the fp64 maximum over the
    remaining valid candidates; S within ``tol`` of its fp64 score; I == cand[P]; nothing
    invalid or past ncand, nothing twice; off rows are the untouched prefix."""
    N, F = xb64.shape[0], cand.shape[1]
    worst = 0.0
    for q in range(cand.shape[0]):
        lm = float(np.float32(lam[q]))
        if lm < 0:
            assert I[q].tolist() == cand[q, :k].tolist() and P[q].tolist() == list(range(k)) and (S[q] == 0).all()
            continue
        left = (np.arange(F) < ncand[q]) & (cand[q] >= 0) & (cand[q] < N)
        rel, sim = cosines64(xb64[np.clip(cand[q], 0, N - 1)], xq[q])
        picked = []
        npick = min(k, int(left.sum()))
        for t in range(npick):
            p = int(P[q, t])
            assert 0 <= p < F and left[p], (q, t, p)
            assert I[q, t] == cand[q, p]
            s = scores64(rel, sim, lm, picked)
            best = float(np.where(left, s, -np.inf).max())
            worst = max(worst, best - float(s[p]), abs(float(S[q, t]) - float(s[p])))
            assert s[p] >= best - tol, (q, t, float(s[p]), best)
            assert abs(float(S[q, t]) - s[p]) <= tol, (q, t, float(S[q, t]), float(s[p]))
            picked.append(p)
            left[p] = False
        assert (S[q, npick:] == 0).all() and (I[q, npick:] == -1).all() and (P[q, npick:] == -1).all()
    return worst


# ------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def cluster_rows(N, d, dtype):
    """8 Gaussian cluster centres + 0.3 noise -> (centres, stored rows, their fp64 image)."""
    g = np.random.default_rng(1000 + d)
    cent = g.standard_normal((8, d))
    xb = torch.from_numpy((cent[np.arange(N) % 8] + 0.3 * g.standard_normal((N, d))).astype(np.float32)).to(dtype)
    return cent, xb, xb.float().double().numpy()


def cluster_lists(cent, N, nq, F, seed):
    """Queries near a centre; candidate lists that repeat clusters, hold ids 0 and N - 1, rows
    with ncand < F and rows with -1 / >= N entries inside; lam cycling through LAMS."""
    g = np.random.default_rng(seed)
    d = cent.shape[1]
    xq = (cent[np.arange(nq) % 8] + 0.3 * g.standard_normal((nq, d))).astype(np.float32)
    cand = np.stack([g.choice(N, F, replace=False) for _ in range(nq)]).astype(np.int64)
    cand[0, 0], cand[-1, -1] = 0, N - 1
    ncand = np.full(nq, F, np.int32)
    for q in range(nq):
        if q % 4 == 1:
            ncand[q] = g.integers(0, F + 1)
        if q % 4 == 2:
            for p, v in zip(g.choice(F, min(F, 3), replace=False), (-1, N, (1 << 40) + 5)):
                cand[q, p] = v
    lam = np.array([LAMS[(q + seed) % len(LAMS)] for q in range(nq)], np.float32)
    return xq, cand, ncand, lam


def unit16(d, dims, signs=None):
    v = np.zeros(d, np.float32)
    v[list(dims)] = 1.0 if signs is None else signs
    assert np.count_nonzero(v) == 16
    return v


def exact_case(d, F, seed):
    """Rows with 16 entries of +-1 (|x|^2 = 16): every cosine is an integer / 16 and, with lam a
    multiple of 1/4, every score is exact in fp32.  -> rows, the query, candidate lists by kind."""
    g = np.random.default_rng(seed)
    N = 300
    xb = np.zeros((N, d), np.float32)
    for r in range(N):
        xb[r] = unit16(d, g.choice(40, 16, replace=False), g.choice([-1.0, 1.0], 16))
    q = unit16(d, range(16))
    xb[0] = unit16(d, list(range(8)) + list(range(16, 24)))           # u: q.u = 8
    xb[1] = unit16(d, list(range(8, 16)) + list(range(24, 32)))       # v: q.v = 8, u.v = 0
    xb[10] = xb[11] = xb[12] = unit16(d, list(range(12)) + list(range(16, 20)))   # one vector, three ids
    for j in range(4):                                                # q.e = 8, e.dup = 8, e.e' = 8
        xb[20 + j] = unit16(d, list(range(8)) + list(range(32 + 8 * j, 40 + 8 * j)))
    xb[30] = 0.0                                                      # a zero row: cosine 0, never NaN
    low = [r for r in range(40, N) if abs(float(xb[r] @ q)) <= 6]
    rest = lambda n: list(g.choice(low, n, replace=False))            # noqa: E731
    lists = {"tie_uv": [0, 1] + rest(F - 2),
             "dups": [10, 11, 12, 20, 21, 22, 23] + rest(F - 7),
             "zero": [30] + list(g.choice(np.arange(40, N), F - 1, replace=False)),
             "random": list(g.choice(np.arange(40, N), F, replace=False))}
    lists["tie_vu"] = [1, 0] + lists["tie_uv"][2:]                    # the tied pair in the other order
    return xb, q, {kd: np.array(v, np.int64) for kd, v in lists.items()}


def check_exact(select, d, F, k, device="cpu"):
    """``select(xb, norms, xq, cand, ncand, lam, k)`` equals the fp64 greedy pick: P, I and S
    bit for bit, on every list kind at every lam."""
    xb, q, lists = exact_case(d, F, seed=d + F)
    kinds = list(lists)
    cand = np.stack([lists[kd] for kd in kinds for _ in EXACT_LAMS])
    lam = np.array([lm for _ in kinds for lm in EXACT_LAMS], np.float32)
    nq = len(lam)
    t = lambda a: torch.from_numpy(a).to(device)                      # noqa: E731
    xbt = t(xb)
    S, I, P = select(xbt, (xbt * xbt).sum(1), t(np.tile(q, (nq, 1))), t(cand),
                     torch.full((nq,), F, dtype=torch.int32, device=device), t(lam), k)
    S, I, P = S.cpu().numpy(), I.cpu().numpy(), P.cpu().numpy()
    assert not np.isnan(S).any()
    for r in range(nq):
        kind = kinds[r // len(EXACT_LAMS)]
        rel, sim = cosines64(xb[cand[r]], q)
        picked, scores = greedy64(rel, sim, float(lam[r]), list(range(F)), k)
        assert P[r].tolist() == picked, (kind, lam[r], P[r].tolist(), picked)
        assert I[r].tolist() == cand[r][picked].tolist()
        assert S[r].tolist() == [float(np.float32(s)) for s in scores]
        if kind in ("tie_uv", "tie_vu"):
            assert P[r, 0] == 0                                       # the earlier of the tied pair
        if kind == "dups" and k >= 3:
            if lam[r] == 0.5:
                assert P[r, 0] == 0 and all(p >= 3 for p in P[r, 1:3])
            if lam[r] == 1.0:
                assert P[r, :3].tolist() == [0, 1, 2]


# ------------------------------------------------------------------ 1. replay
N_ROWS = 3000


@pytest.mark.parametrize("nq", [1, 5, 70])
@pytest.mark.parametrize("dtype,d", [(torch.float32, 8), (torch.float32, 384), (torch.float32, 776),
                                     (torch.float32, 1024), (torch.bfloat16, 16), (torch.bfloat16, 384),
                                     (torch.bfloat16, 784)])
def test_mmr_replays_against_fp64(native, dtype, d, nq):
    cent, xb, xb64 = cluster_rows(N_ROWS, d, dtype)
    xbg = xb.cuda()
    nm = (xbg.float() ** 2).sum(1)
    tol = 4 * (d + 8) * 2.0 ** -24
    worst = 0.0
    for F in (1, 3, 20, 64):
        xq, cand, ncand, lam = cluster_lists(cent, N_ROWS, nq, F, seed=F)
        args = [torch.from_numpy(a).cuda() for a in (xq, cand, ncand, lam)]
        for k in sorted({kk for kk in (1, 3, 10, F) if kk <= F}):
            S, I, P = native.mmr_select(xbg, nm, *args, k)
            assert S.is_cuda and S.dtype == torch.float32 and I.dtype == torch.int64 and P.dtype == torch.int32
            assert S.shape == I.shape == P.shape == (nq, k)
            worst = max(worst, replay(xb64, xq, cand, ncand, lam, k, S.cpu().numpy(), I.cpu().numpy(),
                                      P.cpu().numpy(), tol))
    print(f"mmr replay d={d} {dtype} nq={nq}: worst gap {worst:.3e} (tol {tol:.3e})")


# ------------------------------------------------------------------ 2. exact arithmetic and ties
@pytest.mark.parametrize("d", [64, 384])
@pytest.mark.parametrize("F,k", [(64, 64), (20, 3)])
def test_mmr_exact_arithmetic_and_ties(native, d, F, k):
    check_exact(native.mmr_select, d, F, k, device="cuda")


# ------------------------------------------------------------------ 3. envelope
def _same(a, b):
    return all(torch.equal(x, y) and x.device == y.device and x.dtype == y.dtype for x, y in zip(a, b))


def test_mmr_outside_the_envelope_is_the_reference(native, monkeypatch):
    from docqa_amd.ops import reference as ref

    g = torch.Generator().manual_seed(5)

    def case(d, F, dtype=torch.float32, nq=6, N=200):
        xb = torch.randn(N, d, generator=g).to(dtype).cuda()
        return (xb, (xb.float() ** 2).sum(1), torch.randn(nq, d, generator=g).cuda(),
                torch.stack([torch.randperm(N, generator=g)[:F] for _ in range(nq)]).cuda(),
                torch.full((nq,), F, dtype=torch.int32).cuda(),
                torch.tensor([0.5, 0.0, 1.0, -1.0, 0.25, 0.9])[:nq].cuda())

    for args, k in ((case(12, 20), 3), (case(64, 65), 10), (case(64, 20, torch.float16), 3)):
        out = native.mmr_select(*args, k)
        assert out[0].is_cuda and _same(out, ref.mmr_select(*args, k))
    args = case(64, 20)
    inside = native.mmr_select(*args, 3)
    monkeypatch.setenv("DOCQA_MMR", "0")
    off = native.mmr_select(*args, 3)
    assert _same(off, ref.mmr_select(*args, 3))
    assert torch.equal(inside[2], off[2]) and torch.equal(inside[1], off[1])    # and the kernel agrees
    monkeypatch.delenv("DOCQA_MMR")
    # no questions, and rows without candidates
    xb, nm, xq, cand, ncand, lam = args
    S, I, P = native.mmr_select(xb, nm, xq[:0], cand[:0], ncand[:0], lam[:0], 3)
    assert S.shape == I.shape == P.shape == (0, 3) and S.is_cuda
    lam = torch.full_like(lam, 0.5)
    S, I, P = native.mmr_select(xb, nm, xq, cand, torch.tensor([0, 2, 20, 0, 1, 3], dtype=torch.int32).cuda(), lam, 3)
    assert (I[0] == -1).all() and (P[0] == -1).all() and (S[0] == 0).all() and (I[3] == -1).all()
    assert (I[1, :2] >= 0).all() and I[1, 2] == -1 and P[1, 2] == -1 and S[1, 2] == 0
    assert (I[4, 0] == cand[4, 0]) and (I[4, 1:] == -1).all() and (I[2] >= 0).all() and (I[5] >= 0).all()


# ------------------------------------------------------------------ 4. index and pipeline
@pytest.mark.parametrize("kind", ["flat_fp32", "flat_bf16", "ivfpq_untrained"])
def test_index_mmr_select_is_the_op_on_its_rows(native, kind):
    from docqa_amd.index.flat import FlatIndex
    from docqa_amd.index.hybrid import IVFPQRefineIndex

    g = torch.Generator().manual_seed(11)
    d, N, nq = 64, 500, 7
    x = torch.randn(N, d, generator=g)
    x[100:110] = x[0]                                     # near-copies compete
    if kind == "ivfpq_untrained":
        idx = IVFPQRefineIndex(d, device="cuda")
    else:
        idx = FlatIndex(d, device="cuda", storage_dtype=torch.bfloat16 if kind == "flat_bf16" else torch.float32)
    idx.add(x)
    if kind == "ivfpq_untrained":
        assert idx.ivf is None
    xq = torch.randn(nq, d, generator=g).cuda()
    _, C = idx.search(xq, 20)
    ncand = torch.full((nq,), 20, dtype=torch.int32).cuda()
    lam = torch.tensor([LAMS[q % len(LAMS)] for q in range(nq)]).cuda()
    got = idx.mmr_select(xq, C, ncand, lam, 3)
    want = native.mmr_select(idx.xb, idx.norms, xq, C, ncand, lam, 3)
    assert _same(got, want) and (got[1] >= 0).all()
    # host inputs are moved to the index's device
    assert _same(idx.mmr_select(xq.cpu(), C.cpu(), ncand.cpu(), lam.cpu(), 3), want)


def mixed_pipeline_case(device):
    """A 400-row store of 40 distinct unit vectors x 10 exact copies (row r holds vector r % 40;
    copies 0..4 are patient A's, 5..9 patient B's) behind a RAGPipeline, and a batch mixing
    dense / hybrid / lexical, scoped / unscoped, MMR on / off."""
    from docqa_amd.index.flat import FlatIndex
    from docqa_amd.index.scope import scope_request
    from docqa_amd.pipeline.rag import RAGPipeline

    g = torch.Generator().manual_seed(3)
    d = 128
    base = torch.nn.functional.normalize(torch.randn(40, d, generator=g), dim=1)
    x = base[torch.arange(400) % 40]
    meta = [{"text_content": f"mot{r % 40} commun", "source": f"s{r}", "type": "patient_file",
             "patient_id": "A" if r // 40 < 5 else "B", "note_date": "2024-01-01"} for r in range(400)]
    idx = FlatIndex(d, device=device)
    idx.add(x)

    class _Eng:
        pass
    _Eng.device = torch.device(device)
    pipe = RAGPipeline(None, None, idx, meta, _Eng(), object(), k=3)
    A, B = scope_request("A", None, None, False), scope_request("B", None, None, False)
    on = (0.5, 30)
    rows = [("dense", None, None), ("dense", None, on), ("dense", A, on), ("hybrid", None, None),
            ("hybrid", None, on), ("hybrid", B, on), ("dense", A, None), ("lexical", None, on),
            ("dense", B, (1.0, 30))]
    nq = len(rows)
    qemb = torch.nn.functional.normalize(torch.randn(nq, d, generator=g), dim=1).to(device)
    texts = [f"mot{3 * q} commun" for q in range(nq)]
    return pipe, x, meta, rows, qemb, texts


def check_mixed_pipeline(device):
    from docqa_amd import ops

    pipe, x, meta, rows, qemb, texts = mixed_pipeline_case(device)
    modes, scopes, mmr = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    D, I = pipe.search(qemb, scopes, modes, texts, mmr)
    assert D.shape == I.shape == (len(rows), 3) and (I >= 0).all()
    D, I = D.cpu(), I.cpu()
    off = [q for q, m in enumerate(mmr) if m is None]
    D0, I0 = pipe.search(qemb[off], [scopes[q] for q in off], [modes[q] for q in off], [texts[q] for q in off])
    # MMR off: today's output.  The kNN kernel orders exact copies by id at every depth; the CPU
    # reference's order among them is unspecified, so there the vectors (id % 40) are compared
    if device == "cuda":
        assert torch.equal(I[off], I0.cpu())
    else:
        assert torch.equal(I[off] % 40, I0.cpu() % 40)
    assert torch.allclose(D[off], D0.cpu(), rtol=1e-5, atol=1e-6)
    # the plain search of the same questions returns three copies of one vector
    Dp, Ip = pipe.search(qemb, scopes, ["dense"] * len(rows), texts)
    assert all(len({i % 40 for i in Ip[q].tolist()}) == 1 for q in range(len(rows)))
    depth = 30
    Dd, Id = pipe.index.search(qemb, 64)
    l2 = [dict(zip(Id[q].tolist(), Dd[q].tolist())) for q in range(len(rows))]
    for q, (mode, scope, m) in enumerate(rows):
        ids = I[q].tolist()
        if scope is not None:
            assert all(meta[i]["patient_id"] == scope["patient_id"] for i in ids), q
        if m is None:
            continue
        if m[0] == 1.0:                                                # relevance alone: the copies again
            assert len({i % 40 for i in ids}) == 1 and ids[0] % 40 == Ip[q, 0].item() % 40
        else:
            assert len({i % 40 for i in ids}) == 3, (q, ids)           # three distinct vectors
        # D is the leg's own score of every returned id
        if mode == "dense":
            want = [float(((x[i].double() - qemb[q].cpu().double()) ** 2).sum()) for i in ids]
            assert np.allclose(D[q].numpy(), want, rtol=1e-4, atol=1e-5), q
            if scope is None:
                assert np.allclose(D[q].numpy(), [l2[q][i] for i in ids], rtol=1e-5, atol=1e-6)
        else:
            cols = pipe._scope_cols(qemb.device) if scope is not None else None
            srow = cols.scope_rows([scope]) if scope is not None else None
            lex = pipe._lexical_cols(qemb.device)
            qt, qw, avgdl = lex.query_rows([texts[q]])
            Sl, Il = pipe.index.search_lexical(lex, qt, qw, avgdl, depth, scope_cols=cols, scope=srow)
            if mode == "lexical":
                leg = dict(zip(Il[0].tolist(), Sl[0].tolist()))
            else:
                _, Idq = (pipe.index.search(qemb[q:q + 1], depth) if scope is None
                          else pipe.index.search_scoped(qemb[q:q + 1], depth, cols, srow))
                Fv, C = ops.rank_fuse(Idq, Il, torch.full((1,), 2, dtype=torch.int32, device=Il.device), depth)
                leg = dict(zip(C[0].tolist(), Fv[0].tolist()))
            assert np.allclose(D[q].numpy(), [leg[i] for i in ids], rtol=1e-6, atol=0), q


def test_pipeline_mixed_batch(native):
    check_mixed_pipeline("cuda")
