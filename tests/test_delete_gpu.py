"""Row deletion on the GPU: ``FlatIndex.remove_ids`` / ``IVFPQRefineIndex.remove_ids`` and the
columns kept beside the vectors, against an index built from the surviving rows.

A delete is copying (csrc/kernels/compact.hip), so the compacted index holds identical bits at
identical positions: every comparison is exact equality -- buffers, and the D and I of every
search mode.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N, D = 2600, 128          # more than two scan tiles
WORDS = ("fever", "cough", "aspirin", "renal", "cardiac", "biopsy", "insulin", "fracture", "asthma", "sepsis",
         "anemia", "stroke")


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    return ops


def make_metadata(n: int) -> list[dict]:
    rng = np.random.default_rng(3)
    meta = []
    for i in range(n):
        if i % 9 == 0:
            meta.append({"type": "knowledge_base", "doc_id": "KB", "text_content": f"guideline {WORDS[i % 12]} dose"})
            continue
        words = " ".join(WORDS[j] for j in rng.integers(0, 12, size=int(rng.integers(0, 9))))
        meta.append({"type": "patient_file", "patient_id": f"P{i % 41}", "doc_id": str(i // 8),
                     "text_content": words,            # some rows have no kept token at all
                     "note_date": f"2021-{1 + i % 12:02d}-{1 + i % 28:02d}" if i % 5 else None})
    return meta


@pytest.fixture(scope="module")
def corpus():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(N, D, generator=g)
    meta = make_metadata(N)
    rng = np.random.default_rng(9)
    gone = np.unique(np.concatenate([np.arange(0, 8), np.arange(1020, 1030), np.arange(N - 8, N),
                                     rng.choice(N, size=N // 100, replace=False)]))
    return x, meta, gone


def build(x, meta, dtype):
    from docqa_amd.index.flat import FlatIndex
    from docqa_amd.index.lexical import LexicalColumns
    from docqa_amd.index.scope import ScopeColumns

    idx = FlatIndex(D, "l2", DEV, storage_dtype=dtype)
    idx.add(x)
    sc = ScopeColumns(DEV)
    sc.rebuild(meta)
    lx = LexicalColumns(DEV)
    lx.rebuild(meta)
    return idx, sc, lx


def lexical_state(lx):
    return {"row_ptr": lx.row_ptr, "terms": lx.terms, "tfs": lx.tfs, "dl": lx.dl}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_flat_remove_ids_equals_a_fresh_index(corpus, dtype):
    from docqa_amd.index.flat import removal_mask

    x, meta, gone = corpus
    sel = np.ones(N, dtype=bool)
    sel[gone] = False
    surv = [m for m, s in zip(meta, sel) if s]
    idx, sc, lx = build(x, meta, dtype)
    fresh, fsc, flx = build(x[torch.from_numpy(sel)], surv, dtype)
    before = (idx.xb.clone(), idx.norms.clone())

    ids = np.concatenate([gone, gone[:5], [-3, N, N + 77]])          # duplicates and out-of-range ids are ignored
    keep, pos, removed = removal_mask(ids, N, DEV)
    ran = []

    def swap():
        ran.append(idx.ntotal)
        sc.remove(keep, pos, N - removed)
        lx.remove(keep, pos, N - removed, [meta[i] for i in gone])

    assert idx.remove_ids(ids, before_swap=swap) == gone.size == removed
    assert ran == [N]                                   # once, before the swap
    assert idx.ntotal == fresh.ntotal == N - gone.size
    assert torch.equal(idx.xb, before[0][torch.from_numpy(sel).to(DEV)])
    assert torch.equal(idx.xb, fresh.xb) and idx.xb.dtype == dtype
    assert torch.equal(idx.norms, before[1][torch.from_numpy(sel).to(DEV)])
    assert torch.equal(idx.norms, fresh.norms)
    assert idx.remove_ids([N + 5, -1]) == 0 and idx.ntotal == N - gone.size

    # the columns equal a rebuild over the surviving metadata
    for name, t in lexical_state(flx).items():
        assert torch.equal(lexical_state(lx)[name], t), name
    assert (lx.entries, lx.n, lx.total_len, lx.df) == (flx.entries, flx.n, flx.total_len, flx.df)
    assert sc.n == fsc.n and torch.equal(sc.days, fsc.days)
    assert torch.equal(sc.tags == 0, fsc.tags == 0)

    # every search mode: identical bits at identical positions -> identical D and I
    g = torch.Generator().manual_seed(2)
    xq = torch.randn(9, D, generator=g).to(DEV)
    for k in (3, 16):
        Da, Ia = idx.search(xq, k)
        Db, Ib = fresh.search(xq, k)
        assert torch.equal(Ia, Ib) and torch.equal(Da, Db)
    reqs = [{"patient_id": "P7"}, {"patient_id": "P12", "from_date": "2021-03-01", "to_date": "2021-09-30"},
            None, {"patient_id": "P40", "include_knowledge_base": False}, {"from_date": "2021-06-01"},
            {"patient_id": "nobody"}, {"patient_id": "P1"}, {"patient_id": "P2"}, {"patient_id": "P3"}]
    Da, Ia = idx.search_scoped(xq, 5, sc, sc.scope_rows(reqs))
    Db, Ib = fresh.search_scoped(xq, 5, fsc, fsc.scope_rows(reqs))
    assert torch.equal(Ia, Ib) and torch.equal(Da, Db)
    texts = ["fever cough", "renal biopsy insulin", "guideline dose", "sepsis", "nothing matches this"]
    Sa, Ja = idx.search_lexical(lx, *lx.query_rows(texts), 8)
    Sb, Jb = fresh.search_lexical(flx, *flx.query_rows(texts), 8)
    assert torch.equal(Ja, Jb) and torch.equal(Sa, Sb)
    Sa, Ja = idx.search_lexical(lx, *lx.query_rows(texts), 8, scope_cols=sc, scope=sc.scope_rows(reqs[:5]))
    Sb, Jb = fresh.search_lexical(flx, *flx.query_rows(texts), 8, scope_cols=fsc, scope=fsc.scope_rows(reqs[:5]))
    assert torch.equal(Ja, Jb) and torch.equal(Sa, Sb)

    # the columns keep following adds after a delete
    more = make_metadata(40)
    idx.add(x[:40]); fresh.add(x[:40])
    sc.extend(surv + more); fsc.extend(surv + more)
    lx.extend(surv + more); flx.extend(surv + more)
    for name, t in lexical_state(flx).items():
        assert torch.equal(lexical_state(lx)[name], t), name
    assert lx.df == flx.df and torch.equal(idx.xb, fresh.xb)


def test_lexical_remove_everything_and_nothing_left_behind(corpus):
    from docqa_amd.index.flat import removal_mask
    from docqa_amd.index.lexical import LexicalColumns

    _, meta, _ = corpus
    meta = meta[:70]
    lx = LexicalColumns(DEV)
    lx.rebuild(meta)
    keep, pos, removed = removal_mask(np.arange(70), 70, DEV)
    lx.remove(keep, pos, 0, meta)
    assert (lx.n, lx.entries, lx.total_len, lx.df) == (0, 0, 0, {})
    assert lx.row_ptr.tolist() == [0]
    lx.extend(meta[:10])                                 # and grows again from empty
    again = LexicalColumns(DEV)
    again.rebuild(meta[:10])
    for name, t in lexical_state(again).items():
        assert torch.equal(lexical_state(lx)[name], t), name


def test_trained_ivfpq_remove_ids(corpus):
    from docqa_amd.index.hybrid import IVFPQRefineIndex

    x, _, gone = corpus
    nlist = 8
    idx = IVFPQRefineIndex(D, nlist=nlist, M=16, nprobe=nlist, k_factor=4, train_min=N, device=DEV, rotation="none")
    idx.add(x)
    assert idx.trained
    _ = idx.ivf._norms()
    ivf = idx.ivf
    old = {k: getattr(ivf, k).cpu().numpy().copy() for k in ("codes", "ids", "norms", "list_off")}
    cent, pq = ivf.centroids, ivf.pq

    assert idx.remove_ids(gone) == gone.size
    sel = np.ones(N, dtype=bool)
    sel[gone] = False
    new_row = np.cumsum(sel) - 1
    lk = sel[old["ids"]]
    assert idx.ivf is ivf and ivf.centroids is cent and ivf.pq is pq          # no retraining
    assert idx.ntotal == ivf.ntotal == N - gone.size < idx.train_min
    assert np.array_equal(ivf.codes.cpu().numpy(), old["codes"][lk])
    assert np.array_equal(ivf.ids.cpu().numpy(), new_row[old["ids"][lk]])
    assert np.array_equal(ivf.norms.cpu().numpy(), old["norms"][lk])
    counts = np.array([lk[old["list_off"][l]:old["list_off"][l + 1]].sum() for l in range(nlist)])
    assert np.array_equal(ivf.list_off.cpu().numpy(), np.concatenate([[0], np.cumsum(counts)]))
    assert torch.equal(idx.xb, x.to(DEV)[torch.from_numpy(sel).to(DEV)])

    # a search names surviving rows only, and finds the survivors themselves
    probe = np.nonzero(sel)[0][:32]
    Dd, I = idx.search(x[probe].to(DEV), 4)
    assert int(I.max()) < idx.ntotal and int(I.min()) >= 0
    found = (Dd[:, 0] < 1e-3).cpu().numpy()                # the PQ stage proposed the row itself
    assert found.sum() >= 16
    assert np.array_equal(I[:, 0].cpu().numpy()[found], new_row[probe][found])
    # the removed vectors are no longer their own nearest neighbour at distance 0
    Dg, _ = idx.search(x[gone[:16]].to(DEV), 1)
    assert float(Dg.min()) > 0

    # the snapshot is an ordinary IxRF file and loads back
    from docqa_amd.index import faiss_io

    data = faiss_io.read_index_from(faiss_io.Reader(idx.to_bytes()))
    back = IVFPQRefineIndex.from_data(data, device=DEV)
    assert back.trained and back.ntotal == idx.ntotal
    assert torch.equal(back.ivf.ids, ivf.ids) and torch.equal(back.ivf.codes, ivf.codes)
    assert torch.equal(back.ivf.list_off, ivf.list_off) and torch.equal(back.xb, idx.xb)


def test_untrained_ivfpq_removes_from_the_flat_store(corpus):
    from docqa_amd.index.hybrid import IVFPQRefineIndex

    x, _, gone = corpus
    idx = IVFPQRefineIndex(D, nlist=8, M=16, train_min=10 * N, device=DEV)
    idx.add(x)
    assert not idx.trained and idx.remove_ids(gone) == gone.size
    sel = torch.ones(N, dtype=torch.bool)
    sel[torch.from_numpy(gone)] = False
    assert torch.equal(idx.xb, x[sel].to(DEV))


def test_search_launched_before_a_delete_on_a_side_stream(corpus):
    from docqa_amd.index.flat import FlatIndex

    x, _, gone = corpus
    idx = FlatIndex(D, "l2", DEV)
    idx.add(x)
    xq = x[:64].to(DEV)
    want_d, want_i = idx.search(xq, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        outs = [idx.search(xq, 3) for _ in range(8)]      # queued on the side stream, old generation
    assert idx.remove_ids(gone) == gone.size              # swaps while they may still be running
    filler = [torch.empty(N, D, device=DEV).normal_() for _ in range(4)]     # the allocator may reuse freed blocks
    side.synchronize()
    for d, i in outs:
        assert torch.equal(i, want_i) and torch.equal(d, want_d)
        assert int(i.max()) < N
    del filler
    assert idx.ntotal == N - gone.size
