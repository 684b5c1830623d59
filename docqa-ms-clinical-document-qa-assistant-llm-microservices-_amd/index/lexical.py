"""Row columns and query rows of the lexical (BM25) search (``ops.bm25_topk``).

Every index row carries the analysed terms of its ``text_content`` (text/lexical.py), held
beside the vectors like the scope columns (index/scope.py): derived from the metadata list,
never written to the FAISS file or the write-ahead log.  On the index's device, CSR:

* ``row_ptr`` int64 [n+1]: entries of row r are ``row_ptr[r] .. row_ptr[r+1]``;
* ``terms``   int32 [E]:   the 32-bit term hash's bit pattern, unique within a row and
  ascending by unsigned value;
* ``tfs``     uint8 [E]:   term frequency, capped at 255;
* ``dl``      int32 [n]:   document length (kept tokens, uncapped).

A row without a kept token has no entries.  Host statistics for the idf: ``ndocs`` (empty
rows count), ``total_len`` and ``df`` per term.
"""
from __future__ import annotations

import math
import os

import torch

from ..text.lexical import PAD_TERM, analyze, analyze_full

QUERY_TERMS = 32     # slots of a query row (the kernel's envelope)


def _i32(h: int) -> int:
    return h - (1 << 32) if h >= (1 << 31) else h


class LexicalColumns:
    """Capacity-doubling CSR term columns on the index's device for the first ``n`` rows of a
    metadata list, plus the host document-frequency table.

    ``df`` is a Python dict term -> count: about 100 B per distinct term.  A 10M-row clinical
    corpus has a few million distinct terms (identifiers and typos dominate), so a few
    hundred MB of host memory and, at ~20 us per analysed chunk, minutes of start-up; a
    device-side or array-backed table is the step after this one."""

    # the buffers are updated in place for the columns' whole life: never inference tensors,
    # though the first lexical request builds them inside a service's inference_mode block
    @torch.inference_mode(False)
    def __init__(self, device="cuda", capacity: int = 1024, entry_capacity: int = 1 << 16):
        self.device = torch.device(device)
        self._row_ptr = torch.zeros(capacity + 1, dtype=torch.int64, device=self.device)
        self._dl = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self._terms = torch.zeros(entry_capacity, dtype=torch.int32, device=self.device)
        self._tfs = torch.zeros(entry_capacity, dtype=torch.uint8, device=self.device)
        self.df: dict[int, int] = {}
        self.total_len = 0
        self.entries = 0
        self.n = 0          # metadata rows covered so far (= ndocs)

    # ------------------------------------------------------------------ rows
    @property
    def ndocs(self) -> int:
        return self.n

    @property
    def row_ptr(self) -> torch.Tensor:
        return self._row_ptr[: self.n + 1]

    @property
    def terms(self) -> torch.Tensor:
        return self._terms[: self.entries]

    @property
    def tfs(self) -> torch.Tensor:
        return self._tfs[: self.entries]

    @property
    def dl(self) -> torch.Tensor:
        return self._dl[: self.n]

    def stats(self) -> dict:
        return {"rows": self.n, "entries": self.entries, "distinct_terms": len(self.df)}

    def _sync(self) -> None:
        # searches may run on another stream (the QA prep stream): rows are complete on the
        # device before ``n`` makes them visible
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()

    @staticmethod
    def _grown(old: torch.Tensor, keep: int, size: int) -> torch.Tensor:
        new = torch.zeros(size, dtype=old.dtype, device=old.device)
        new[:keep] = old[:keep]
        return new

    @torch.inference_mode(False)
    def extend(self, metadata: list[dict]) -> None:
        """Cover rows ``n..len(metadata)`` (one small host-to-device copy per column).  The
        state changes only at the end: the buffers (grown ones included) are complete on the
        device before they and ``n`` become visible, and a failure leaves every statistic as
        it was."""
        start, end = self.n, len(metadata)
        if end <= start:
            return
        terms, tfs, dls, ptr = [], [], [], []
        df_add: dict[int, int] = {}
        e, total = self.entries, self.total_len
        for i in range(start, end):
            pairs, dl = analyze_full(metadata[i].get("text_content", "") or "")
            for h, tf in pairs:
                terms.append(_i32(h))
                tfs.append(tf)
                df_add[h] = df_add.get(h, 0) + 1
            e += len(pairs)
            total += dl
            ptr.append(e)
            dls.append(min(dl, (1 << 31) - 1))
        if e >= (1 << 31):
            raise OverflowError("lexical columns: 2^31 entries")
        row_ptr, dls_t, terms_t, tfs_t = self._row_ptr, self._dl, self._terms, self._tfs
        cap = dls_t.shape[0]                     # one row capacity c: dl [c], row_ptr [c + 1]
        if end > cap:
            cap = max(end, cap * 2)
            row_ptr = self._grown(row_ptr, start + 1, cap + 1)
            dls_t = self._grown(dls_t, start, cap)
        if e > terms_t.shape[0]:
            ecap = max(e, terms_t.shape[0] * 2)
            terms_t = self._grown(terms_t, self.entries, ecap)
            tfs_t = self._grown(tfs_t, self.entries, ecap)
        row_ptr[start + 1:end + 1] = torch.tensor(ptr, dtype=torch.int64).to(self.device)
        dls_t[start:end] = torch.tensor(dls, dtype=torch.int32).to(self.device)
        if terms:
            terms_t[self.entries:e] = torch.tensor(terms, dtype=torch.int32).to(self.device)
            tfs_t[self.entries:e] = torch.tensor(tfs, dtype=torch.uint8).to(self.device)
        self._sync()
        self._row_ptr, self._dl, self._terms, self._tfs = row_ptr, dls_t, terms_t, tfs_t
        for h, c in df_add.items():
            self.df[h] = self.df.get(h, 0) + c
        self.total_len, self.entries = total, e
        self.n = end

    def rebuild(self, metadata: list[dict]) -> None:
        self.df, self.total_len, self.entries, self.n = {}, 0, 0, 0
        self.extend(metadata)

    @torch.inference_mode(False)
    def remove(self, keep: torch.Tensor, pos: torch.Tensor, n_out: int, removed: list[dict]) -> None:
        self.prepare_remove(keep, pos, n_out, removed)()

    @torch.inference_mode(False)
    def prepare_remove(self, keep: torch.Tensor, pos: torch.Tensor, n_out: int, removed: list[dict]):
        """Two-step :meth:`remove`: the validation and every new device buffer are made here and
        change nothing; the returned ``commit()`` only swaps references and updates statistics.

        Drop the rows a delete removes: ``keep`` uint8 [n], ``pos`` its ``ops.masked_scan``,
        ``n_out`` the surviving count, ``removed`` the removed rows' records (their text is
        analysed again for the statistics: ``df`` is decremented and a term that reaches 0 is
        dropped, ``total_len`` and ``entries`` shrink by what the rows held -- so no count is
        read back from the device).  Same rule as :meth:`extend`: the new buffers are complete
        on the device before they and ``n`` become visible."""
        from .. import ops

        if keep.numel() != self.n or self.n - n_out != len(removed):
            raise ValueError(f"lexical columns cover {self.n} rows: mask {keep.numel()}, {n_out} left, "
                             f"{len(removed)} records")
        df_sub: dict[int, int] = {}
        gone_entries = gone_len = 0
        for m in removed:
            pairs, dl = analyze_full(m.get("text_content", "") or "")
            for h, _ in pairs:
                df_sub[h] = df_sub.get(h, 0) + 1
            gone_entries += len(pairs)
            gone_len += dl
        e_out = self.entries - gone_entries
        if e_out < 0 or any(self.df.get(h, 0) < c for h, c in df_sub.items()):
            raise ValueError("lexical columns: the removed records do not match the rows they name")
        row_ptr = self._row_ptr[: self.n + 1]
        epos = ops.masked_scan(keep, row_ptr[1:] - row_ptr[:-1])
        new_ptr, terms, tfs = ops.csr_gather(row_ptr, keep, pos, epos, self._terms[: self.entries],
                                             self._tfs[: self.entries], n_out, e_out)
        dl_t = ops.gather_rows(self._dl[: self.n], keep, pos, n_out)
        if e_out == 0:       # the scan kernel is never handed an empty buffer
            terms, tfs = self._grown(terms, 0, 1), self._grown(tfs, 0, 1)
        if n_out == 0:
            new_ptr, dl_t = self._grown(new_ptr, 1, 2), self._grown(dl_t, 0, 1)
        self._sync()

        def commit() -> None:
            self._row_ptr, self._dl, self._terms, self._tfs = new_ptr, dl_t, terms, tfs
            for h, c in df_sub.items():
                left = self.df[h] - c
                if left:
                    self.df[h] = left
                else:
                    del self.df[h]
            self.total_len -= gone_len
            self.entries = e_out
            self.n = n_out

        return commit

    # ------------------------------------------------------------------ queries
    @property
    def avgdl(self) -> float:
        return self.total_len / self.n if self.n and self.total_len else 1.0

    def query_row(self, text: str) -> tuple[list[int], list[float]]:
        """(terms as unsigned hashes, fp64 weights) of one query, at most ``QUERY_TERMS``:
        the analysed terms some row holds, weight = qtf x Lucene's idf; over the cap the
        heaviest stay, ties towards the lower hash."""
        n = self.n
        cand = []
        for h, qtf in analyze(text):
            df = self.df.get(h, 0)
            if df > 0:
                cand.append((qtf * math.log(1.0 + (n - df + 0.5) / (df + 0.5)), h))
        cand.sort(key=lambda wh: (-wh[0], wh[1]))
        cand = cand[:QUERY_TERMS]
        return [h for _, h in cand], [w for w, _ in cand]

    def query_rows(self, texts: list[str]):
        """(qterms int32 [nq, 32], qweights fp32 [nq, 32]) on the device and ``avgdl``; unused
        slots hold the padding key and weight 0.  Weights are formed in fp64 and rounded
        once to fp32."""
        nq = len(texts)
        qt = torch.full((nq, QUERY_TERMS), _i32(PAD_TERM), dtype=torch.int32)
        qw = torch.zeros((nq, QUERY_TERMS), dtype=torch.float64)
        for i, t in enumerate(texts):
            hs, ws = self.query_row(t)
            if hs:
                qt[i, : len(hs)] = torch.tensor([_i32(h) for h in hs], dtype=torch.int32)
                qw[i, : len(ws)] = torch.tensor(ws, dtype=torch.float64)
        return qt.to(self.device), qw.to(torch.float32).to(self.device), self.avgdl


def fetch_depth(k: int) -> int:
    """Depth of the dense and the lexical leg in front of the rank fusion: ``HYBRID_FETCH_K``,
    default min(64, max(16, 4 k)), clamped to k..64."""
    return max(k, min(64, int(os.environ.get("HYBRID_FETCH_K") or max(16, 4 * k))))
