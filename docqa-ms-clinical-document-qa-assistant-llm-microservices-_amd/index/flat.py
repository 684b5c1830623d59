"""Exact flat vector index (IndexFlatL2 / IndexFlatIP semantics), HBM-resident.

The database lives on the GPU in a capacity-doubling buffer (``add`` is an async
device copy, amortised O(1); no host round trip), together with its fp32 squared norms
for the ``||x||^2 + ||y||^2 - 2 x.y`` decomposition.  ``search`` is one launch of the
fused MFMA distance + top-k kernel (``ops.knn``) plus its merge pass.  Storage dtype:
fp32 (exact, the FAISS format and the default) or bf16 (half the HBM bytes per scan,
for multi-million-vector shards).

Reference parity: ``faiss.IndexFlatL2(384)`` created/added at
semantic-indexer/indexer.py:39-41, written at :27, read back at llm-qa/main.py:35, and
searched with k=3 through the LangChain retriever (llm-qa/main.py:101).  Unlike the
reference, the QA side sees new vectors without a restart.
"""
from __future__ import annotations

import threading

import numpy as np
import torch

from .. import ops
from . import faiss_io


def removal_mask(ids, n: int, device):
    """(``keep`` uint8 [n], ``pos`` int64 [n+1], removed) for deleting the row ids ``ids`` from
    ``n`` rows: ids outside ``[0, n)`` and duplicates are ignored (FAISS ``remove_ids``), ``pos``
    is ``ops.masked_scan(keep)`` -- the new position of every surviving row.  The count comes
    from the host-side id list, so nothing here waits for the device."""
    host = np.unique(np.asarray(torch.as_tensor(ids).cpu(), dtype=np.int64).reshape(-1))
    host = host[(host >= 0) & (host < n)]
    keep = torch.ones(n, dtype=torch.uint8, device=device)
    if host.size:
        keep[torch.from_numpy(host).to(device)] = 0
    return keep, ops.masked_scan(keep), int(host.size)


class FlatIndex:
    def __init__(self, d: int, metric: str = "l2", device="cuda", storage_dtype=torch.float32,
                 capacity: int = 1024):
        if metric not in ("l2", "ip"):
            raise ValueError("metric must be 'l2' or 'ip'")
        self.d = d
        self.metric = metric
        self.device = torch.device(device)
        self.storage_dtype = storage_dtype
        self._xb = torch.empty(capacity, d, device=self.device, dtype=storage_dtype)
        self._norms = torch.empty(capacity, device=self.device, dtype=torch.float32)
        self.ntotal = 0
        self._lock = threading.RLock()

    # ------------------------------------------------------------------ mutation
    def _grow(self, need: int) -> None:
        cap = self._xb.shape[0]
        if need <= cap:
            return
        new = max(need, cap * 2)
        xb = torch.empty(new, self.d, device=self.device, dtype=self.storage_dtype)
        nm = torch.empty(new, device=self.device, dtype=torch.float32)
        xb[: self.ntotal] = self._xb[: self.ntotal]
        nm[: self.ntotal] = self._norms[: self.ntotal]
        self._xb, self._norms = xb, nm

    def add(self, x) -> None:
        x = torch.as_tensor(x)
        if x.dim() == 1:
            x = x[None]
        if x.shape[1] != self.d:
            raise ValueError(f"dimension mismatch: {x.shape[1]} != {self.d}")
        x = x.to(self.device, dtype=torch.float32, non_blocking=True)
        with self._lock:
            n = x.shape[0]
            self._grow(self.ntotal + n)
            stored = x.to(self.storage_dtype)
            self._xb[self.ntotal:self.ntotal + n] = stored
            self._norms[self.ntotal:self.ntotal + n] = (stored.float() ** 2).sum(1)
            self.ntotal += n

    def reset(self) -> None:
        with self._lock:
            self.ntotal = 0

    def replace(self, x, before_swap=None, after_swap=None) -> None:
        """Replace the whole content with ``x`` [n, d] without an empty or partial
        intermediate state: the new storage is built off to the side, then swapped in
        under the lock (``before_swap()``, e.g. a metadata swap, runs under the same
        lock, ``after_swap()`` as its last statement), so a concurrent search sees either the
        old or the new index."""
        x = torch.as_tensor(x)
        if x.dim() == 1:
            x = x[None]
        if x.numel() and x.shape[1] != self.d:
            raise ValueError(f"dimension mismatch: {x.shape[1]} != {self.d}")
        n = x.shape[0] if x.numel() else 0
        cap = max(1024, n)
        xb = torch.empty(cap, self.d, device=self.device, dtype=self.storage_dtype)
        nm = torch.empty(cap, device=self.device, dtype=torch.float32)
        if n:
            stored = x.to(self.device, dtype=torch.float32).to(self.storage_dtype)
            xb[:n] = stored
            nm[:n] = (stored.float() ** 2).sum(1)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        with self._lock:
            if before_swap is not None:
                before_swap()
            self._xb, self._norms, self.ntotal = xb, nm, n
            if after_swap is not None:
                after_swap()

    def remove_ids(self, ids, before_swap=None, after_swap=None, mask=None) -> int:
        """Remove the rows ``ids`` (FAISS ``IndexFlat::remove_ids``): surviving rows keep their
        order and later ids shift down; ids outside ``[0, ntotal)`` and duplicates are ignored.
        Returns the number of rows removed (0: nothing changes, ``before_swap`` is not called).

        Same discipline as :meth:`replace`: the compacted vectors and norms are built off to
        the side (``ops.gather_rows``, out of place), the stream is synchronised, then they are
        swapped in under the lock with ``before_swap()`` -- the metadata and column swap --
        running under the same lock.  A search in flight on another stream keeps reading the old
        buffers (``search`` recorded its stream on them).  Transient memory: one extra copy of
        the store (the surviving rows) until the old buffers are released.  ``after_swap()``
        runs as the last statement under the lock, once the new buffers are in place.  ``mask``:
        the ``removal_mask(ids, ntotal, device)`` a caller already made for its own columns."""
        with self._lock:
            n, xb, nm = self.ntotal, self._xb, self._norms
        keep, pos, removed = mask if mask is not None else removal_mask(ids, n, self.device)
        if keep.numel() != n:
            raise ValueError(f"remove_ids: the mask covers {keep.numel()} rows, the index holds {n}")
        if removed == 0:
            return 0
        left = n - removed
        cap = max(1024, left)
        new_xb = torch.empty(cap, self.d, device=self.device, dtype=self.storage_dtype)
        new_nm = torch.empty(cap, device=self.device, dtype=torch.float32)
        ops.gather_rows(xb[:n], keep, pos, out=new_xb)
        ops.gather_rows(nm[:n], keep, pos, out=new_nm)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()
        with self._lock:
            if self.ntotal != n or self._xb is not xb:
                raise RuntimeError("remove_ids: the index changed during the delete (writers must be serialised)")
            if before_swap is not None:
                before_swap()
            self._xb, self._norms, self.ntotal = new_xb, new_nm, left
            if after_swap is not None:
                after_swap()
        return removed

    # ------------------------------------------------------------------ query
    @property
    def xb(self) -> torch.Tensor:
        return self._xb[: self.ntotal]

    @property
    def norms(self) -> torch.Tensor:
        return self._norms[: self.ntotal]

    def search(self, xq, k: int, id_offset: int = 0):
        """xq [nq, d] -> (D [nq, k] fp32, I [nq, k] int64), FAISS conventions."""
        xq = torch.as_tensor(xq)
        if xq.dim() == 1:
            xq = xq[None]
        xq = xq.to(self.device, dtype=torch.float32)
        with self._lock:
            xb, nm = self._xb, self._norms
            if xb.is_cuda:
                # the kernel may run on a side stream (the RAG prep stream) while a
                # concurrent replace()/_grow() drops these buffers: keep the caching
                # allocator from handing them out until this stream's work is done
                s = torch.cuda.current_stream(self.device)
                xb.record_stream(s)
                nm.record_stream(s)
            return ops.knn(xb[: self.ntotal], nm[: self.ntotal], xq, k, self.metric == "ip", id_offset)

    def search_scoped(self, xq, k: int, cols, scope, id_offset: int = 0):
        """``search`` among the rows inside each query's scope: ``cols`` the rows'
        :class:`~docqa_amd.index.scope.ScopeColumns`, ``scope`` int32 [nq, 4] (its
        ``scope_rows``).  Exact; covers rows ``[0, min(ntotal, cols.n))``."""
        xq = torch.as_tensor(xq)
        if xq.dim() == 1:
            xq = xq[None]
        xq = xq.to(self.device, dtype=torch.float32)
        scope = torch.as_tensor(scope).to(self.device, dtype=torch.int32)
        with self._lock:
            # a delete swaps vectors and columns together under this lock, an add extends the
            # columns first: min() is a row count every buffer read below covers
            n = min(self.ntotal, cols.n)
            xb, nm, tags, days = self._xb, self._norms, cols._tags, cols._days
            if xb.is_cuda:
                # as in search(): the kernel may run on a side stream while these are dropped
                s = torch.cuda.current_stream(self.device)
                for t in (xb, nm, tags, days):
                    t.record_stream(s)
            return ops.knn_scoped(xb[:n], nm[:n], tags[:n], days[:n], xq, scope, k, self.metric == "ip",
                                  id_offset)

    def search_lexical(self, cols, qterms, qweights, avgdl: float, k: int, scope_cols=None, scope=None,
                       id_offset: int = 0):
        """BM25 top-k over the rows' :class:`~docqa_amd.index.lexical.LexicalColumns`
        (``qterms``, ``qweights``, ``avgdl``: its ``query_rows``); ``scope_cols`` + ``scope``
        restrict every query as in :meth:`search_scoped`.  -> (S descending, I), -1 past the
        matching rows.  Exact (the columns do not depend on the vectors); covers rows
        ``[0, min(ntotal, cols.n[, scope_cols.n]))``."""
        with self._lock:
            n = min(self.ntotal, cols.n)      # as in search_scoped()
            if scope is not None:
                n = min(n, scope_cols.n)
            bufs = [cols._row_ptr, cols._terms, cols._tfs, cols._dl]
            tags = days = None
            if scope is not None:
                scope = torch.as_tensor(scope).to(self.device, dtype=torch.int32)
                tags, days = scope_cols._tags, scope_cols._days
                bufs += [tags, days]
                tags, days = tags[:n], days[:n]
            if self.device.type == "cuda":
                # as in search(): the kernel may run on a side stream while these are dropped
                s = torch.cuda.current_stream(self.device)
                for t in bufs:
                    t.record_stream(s)
            return ops.bm25_topk(bufs[0][: n + 1], bufs[1], bufs[2], bufs[3][:n], qterms, qweights, k, avgdl,
                                 tags=tags, days=days, scope=scope, id_offset=id_offset)

    def mmr_select(self, xq, cand, ncand, lam, k: int):
        """Maximal marginal relevance re-selection (``ops.mmr_select``) of ranked row ids
        ``cand`` int64 [nq, F] -- a search's hits over these rows -- against the stored vectors:
        -> (S, I, P) [nq, k].  Ids outside ``[0, ntotal)`` are no candidates."""
        xq = torch.as_tensor(xq)
        if xq.dim() == 1:
            xq = xq[None]
        xq = xq.to(self.device, dtype=torch.float32)
        cand = torch.as_tensor(cand).to(self.device, dtype=torch.long)
        ncand = torch.as_tensor(ncand).to(self.device, dtype=torch.int32)
        lam = torch.as_tensor(lam).to(self.device, dtype=torch.float32)
        with self._lock:
            xb, nm = self._xb, self._norms
            if xb.is_cuda:
                # as in search(): the kernel may run on a side stream while these are dropped
                s = torch.cuda.current_stream(self.device)
                xb.record_stream(s)
                nm.record_stream(s)
            return ops.mmr_select(xb[: self.ntotal], nm[: self.ntotal], xq, cand, ncand, lam, k)

    def reconstruct(self, i: int) -> np.ndarray:
        return self._xb[i].float().cpu().numpy()

    # ------------------------------------------------------------------ persistence
    def to_numpy(self) -> np.ndarray:
        return self.xb.float().cpu().numpy()

    def save(self, path) -> None:
        metric = faiss_io.METRIC_L2 if self.metric == "l2" else faiss_io.METRIC_INNER_PRODUCT
        faiss_io.write_flat(path, self.to_numpy(), metric)

    @classmethod
    def load(cls, path, device="cuda", storage_dtype=torch.float32) -> "FlatIndex":
        data = faiss_io.read_index(path)
        if not isinstance(data, faiss_io.FlatIndexData):
            raise ValueError("not a flat index")
        idx = cls(data.d, "l2" if data.metric == faiss_io.METRIC_L2 else "ip", device,
                  storage_dtype, capacity=max(1024, data.ntotal))
        if data.ntotal:
            idx.add(torch.from_numpy(data.xb))
        return idx
