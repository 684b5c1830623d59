"""Retrieval-augmented QA: question -> embed -> kNN top-k -> "stuff" prompt -> generate.

Batched and device-resident end to end: a batch of questions is embedded in one packed
varlen encoder forward, searched in one fused distance+top-k launch (or the sharded
all-gather search across GPUs), and all prompts are generated together by the HIP-graph
decode engine.  Per-stage wall times are recorded for the latency breakdown.

Reference parity (llm-qa/main.py:71-122): ``RetrievalQA.from_chain_type(chain_type=
"stuff", k=3, return_source_documents=True)`` -> contexts joined with a blank line into
the prompt's ``{context}``, the user question into ``{question}``; the response carries
``answer`` and the ``source`` metadata of the k retrieved chunks (duplicates allowed).
The reference serves one request at a time; here every stage is batched.
"""
from __future__ import annotations

import math
import os
import time
from dataclasses import dataclass, field

import torch

# safety factor of the adaptive pipeline lead (answer_pipelined): preparation cost x this,
# over the decode step time
_LEAD_MARGIN = float(os.environ.get("DOCQA_PIPELINE_LEAD_MARGIN", "1.5"))

from .. import ops
from ..utils import tracing
from ..engine.llm_engine import LLMEngine, SamplingParams
from ..prompts import CACHE_FRIENDLY_QA_TEMPLATE, REFERENCE_QA_TEMPLATE, qa_template

# QA prompt: the verbatim reference QA_CHAIN_PROMPT (llm-qa/main.py:71-93) by default, the
# cache-friendly reordering with QA_TEMPLATE=cache_friendly (docqa_amd/prompts.py)
DEFAULT_TEMPLATE = REFERENCE_QA_TEMPLATE

# retrieval modes of a question, in ops.rank_fuse's numbering: the dense kNN hits, the BM25
# hits, or their reciprocal rank fusion
SEARCH_MODES = ("dense", "lexical", "hybrid")


@dataclass
class StageTimes:
    embed_s: float = 0.0
    search_s: float = 0.0
    prompt_s: float = 0.0
    generate_s: float = 0.0

    def total(self) -> float:
        return self.embed_s + self.search_s + self.prompt_s + self.generate_s


@dataclass
class Answer:
    answer: str
    sources: list
    token_ids: list = field(default_factory=list)
    chunk_ids: list = field(default_factory=list)   # index rows retrieved for the prompt


class RAGPipeline:
    def __init__(self, encoder, enc_tokenizer, index, metadata: list[dict], engine: LLMEngine,
                 chat_tokenizer, k: int = 3, template: str | None = None,
                 max_prompt_tokens: int | None = None, context_order: str | None = None):
        template = template if template is not None else qa_template()
        # order of the retrieved chunks inside the prompt: "relevance" (nearest first, as
        # the reference's stuff chain), "shared" (the batch's most-retrieved chunks first,
        # ties by id: prompts retrieving a common chunk then share its KV blocks in the
        # prefix cache) or "trie" (the order whose leading chunks an earlier prompt already
        # used -- this batch or an earlier one, whose KV the prefix cache still holds --
        # else "shared").  Same chunks either way; Answer.sources keep relevance order.
        # Default: trie with the cache-friendly template (the prompt arranged for the prefix
        # cache: 0.72 -> 0.75 -> 0.77 of prompt tokens cached, +5 % then +2.5 % q/s same box,
        # profiles/r4_context_order_ab.log), relevance with the reference's verbatim template
        context_order = context_order or os.environ.get("DOCQA_CONTEXT_ORDER") or (
            "trie" if template == CACHE_FRIENDLY_QA_TEMPLATE else "relevance")
        if context_order not in ("relevance", "shared", "trie"):
            raise ValueError(f"context_order must be relevance, shared or trie, got {context_order!r}")
        self.context_order = context_order
        self._seen: set[tuple[int, ...]] = set()
        self.encoder = encoder
        self.enc_tok = enc_tokenizer
        self.index = index
        self.metadata = metadata
        self.engine = engine
        self.chat_tok = chat_tokenizer
        # format: "json" -- the engine masks tokens by their bytes (LLMEngine.set_vocab_bytes); a
        # tokenizer without all 256 single-byte tokens leaves it unset and such requests refused
        if (hasattr(engine, "set_vocab_bytes") and engine.vocab_bytes is None
                and hasattr(chat_tokenizer, "token_bytes")):
            try:
                engine.set_vocab_bytes(chat_tokenizer.token_bytes(engine.cfg.vocab_size))
            except ValueError:
                pass
        self.k = k
        self.template = template
        self.max_prompt_tokens = max_prompt_tokens
        self.last_times = StageTimes()
        # row tags / days of the scoped search (index/scope.py): an IndexFollower's or the
        # indexer's when one owns the (index, metadata) pair, else built lazily from metadata
        self.scopes = None
        self._own_scopes = None
        # term columns of the lexical / hybrid search (index/lexical.py), built on the first
        # such request: the owner's (``lexical_owner.ensure_lexical()``) when one keeps the
        # (index, metadata) pair, else built from metadata here
        self.lexical = None
        self.lexical_owner = None
        self._own_lexical = None
        # token ids of every retrieved chunk, tokenised once: a prompt is then assembled
        # from cached pieces split at paragraph boundaries (the byte-level BPE never merges
        # across a newline pre-token), so only the question is tokenised per request
        self._chunk_ids: dict[int, list[int]] = {}
        # the owner of the (index, metadata) pair (SemanticIndexer / IndexFollower), handed over
        # like its columns (services/stack.py).  Row ids are positions and a delete shifts them:
        # ``owner.generation`` is odd while a delete swaps the pair and changes with every one,
        # so :meth:`resolve` reads it before the search and again once ids are resolved to
        # records and prompts, and redoes the batch's retrieval when it moved.  Deletes are
        # rare: no lock on the hot path.  None: nobody deletes, nothing is checked
        self.owner = None
        self._generation = 0
        self._after_search = None        # test hook: called between the search and the resolve
        self._pieces = None
        if hasattr(chat_tokenizer, "special") and template.count("{context}") == 1 \
                and template.count("{question}") == 1 and template.index("{context}") < template.index("{question}"):
            head, _, rest = template.partition("{context}")
            mid, _, tail = rest.partition("{question}")
            self._pieces = (head, mid, tail)

    def _sync(self):
        if self.engine.device.type == "cuda":
            torch.cuda.synchronize()

    def embed(self, texts: list[str]) -> torch.Tensor:
        return self.encoder.encode(self.enc_tok.encode_batch(texts))

    def _host_ids(self, I: torch.Tensor) -> list[list[int]]:
        """Hits to the host (the batch's one sync on the search stream), then surface a
        failed cross-rank gather of a sharded index (index/sharded.py) as an exception
        instead of serving stale peer rows."""
        ids = I.tolist()
        check = getattr(self.index, "check_gather", None)
        if check is not None:
            check()
        return ids

    def _scope_cols(self, device):
        if self.scopes is None:
            from ..index.scope import ScopeColumns

            self._own_scopes = self.scopes = ScopeColumns(getattr(self.index, "device", device))
        if self._own_scopes is self.scopes:     # no follower / indexer keeps it in step
            if self.scopes.n > len(self.metadata):
                self.scopes.rebuild(self.metadata)
            self.scopes.extend(self.metadata)
        return self.scopes

    def _lexical_cols(self, device):
        """The term columns, built on the first lexical / hybrid request: the (index, metadata)
        owner's (``lexical_owner.ensure_lexical()``, kept in step by it from then on), else
        this pipeline's own, extended from the metadata list on every such request."""
        if self.lexical is None:
            if self.lexical_owner is not None:
                self.lexical = self.lexical_owner.ensure_lexical()
            else:
                from ..index.lexical import LexicalColumns

                self._own_lexical = self.lexical = LexicalColumns(getattr(self.index, "device", device))
        if self._own_lexical is self.lexical:
            if self.lexical.n > len(self.metadata):
                self.lexical.rebuild(self.metadata)
            self.lexical.extend(self.metadata)
        return self.lexical

    def search(self, qemb: torch.Tensor, scopes: list | None = None, modes: list | None = None,
               texts: list | None = None, mmr: list | None = None):
        """(D, I) of the embedded questions' top-k.  ``scopes``: per question ``None`` or a
        scope request (index/scope.py: patient_id, from_date, to_date,
        include_knowledge_base); a batch without any takes the unscoped search, a mixed
        batch is one scoped launch (``None`` = the any-scope row).  ``modes``: per question
        ``"dense"``, ``"lexical"`` or ``"hybrid"`` (``texts``: the questions, needed by the last
        two); ``None`` or all dense is the dense search alone.  ``mmr``: per question ``None`` or
        ``(lambda_mult, fetch_k)`` -- the k hits are then re-selected for diversity out of the
        question's first ``fetch_k`` (:meth:`_search_mmr`); ``None`` or all ``None`` runs exactly
        the launches above."""
        if mmr is not None and any(m is not None for m in mmr):
            return self._search_mmr(qemb, scopes, modes, texts, mmr)
        if modes is not None and any(m != "dense" for m in modes):
            return self._search_modes(qemb, scopes, modes, texts)
        if scopes is None or all(s is None for s in scopes):
            return self.index.search(qemb, self.k)
        if len(scopes) != qemb.shape[0]:
            raise ValueError("one scope per question")
        cols = self._scope_cols(qemb.device)
        return self.index.search_scoped(qemb, self.k, cols, cols.scope_rows(scopes))

    def _search_modes(self, qemb, scopes, modes, texts):
        """A batch with a lexical or hybrid question: the dense leg and the BM25 leg for the
        whole batch at depth ``HYBRID_FETCH_K`` (default min(64, max(16, 4 k))), then
        ``ops.rank_fuse`` picks per question the dense hits, the lexical hits or their
        reciprocal rank fusion -- three launches, no host sync between them.  D is the
        leg's own score: L2 distance, BM25 score or RRF value."""
        nq, k = qemb.shape[0], self.k
        if texts is None or len(texts) != nq or len(modes) != nq:
            raise ValueError("one mode and one question text per question")
        bad = [m for m in modes if m not in SEARCH_MODES]
        if bad:
            raise ValueError(f"search mode must be one of {SEARCH_MODES}, got {bad[0]!r}")
        if k > 64:
            raise ValueError("lexical / hybrid search serves k <= 64")
        from ..index.lexical import fetch_depth

        depth = fetch_depth(k)
        lex = self._lexical_cols(qemb.device)
        scoped = scopes is not None and any(s is not None for s in scopes)
        if scoped and len(scopes) != nq:
            raise ValueError("one scope per question")
        cols = rows = None
        if scoped:
            cols = self._scope_cols(qemb.device)
            rows = cols.scope_rows(scopes)
            Dd, Id = self.index.search_scoped(qemb, depth, cols, rows)
        else:
            Dd, Id = self.index.search(qemb, depth)
        qt, qw, avgdl = lex.query_rows(list(texts))
        Sl, Il = self.index.search_lexical(lex, qt, qw, avgdl, depth, scope_cols=cols, scope=rows)
        mode = torch.tensor([SEARCH_MODES.index(m) for m in modes], dtype=torch.int32).to(Id.device)
        F, I = ops.rank_fuse(Id, Il, mode, k)
        m = mode[:, None]
        return torch.where(m == 0, Dd[:, :k], torch.where(m == 1, Sl[:, :k], F)), I

    def _search_mmr(self, qemb, scopes, modes, texts, mmr):
        """A batch with a maximal-marginal-relevance question (LangChain's
        ``search_type="mmr"``): the legs run at depth ``max(k, max fetch_k)`` (with a lexical or
        hybrid question both legs at ``max(fetch_depth(k), that)`` and ``ops.rank_fuse`` returns
        that many ids), then one ``mmr_select`` launch re-selects k per question out of its own
        first ``fetch_k`` candidates by ``lambda_mult * cos(q, c) - (1 - lambda_mult) * max
        cos(c, picked)``.  Questions without MMR carry ``lam = -1`` and keep their first k; their
        rank fusion sees the leg depth it sees without MMR in the batch.  The relevance term is
        the cosine to the question's embedding in every mode; scopes apply to the candidates.
        D is the leg's own score of each picked row (gathered by position on the device), in
        pick order; no host sync."""
        nq, k = qemb.shape[0], self.k
        if len(mmr) != nq:
            raise ValueError("one mmr entry per question")
        if k > 64:
            raise ValueError("mmr search serves k <= 64")
        lam_h, fk_h = [], []
        for m in mmr:
            if m is None:
                lam_h.append(-1.0)
                fk_h.append(k)
                continue
            lm, fk = float(m[0]), int(m[1])
            if not 0.0 <= lm <= 1.0:
                raise ValueError(f"lambda_mult must be in [0, 1], got {m[0]!r}")
            if fk < 1:
                raise ValueError(f"fetch_k must be >= 1, got {m[1]!r}")
            lam_h.append(lm)
            fk_h.append(min(64, max(k, fk)))
        F = max(fk_h)
        scoped = scopes is not None and any(s is not None for s in scopes)
        if scoped and len(scopes) != nq:
            raise ValueError("one scope per question")
        cols = rows = None
        if scoped:
            cols = self._scope_cols(qemb.device)
            rows = cols.scope_rows(scopes)
        if modes is not None and any(m != "dense" for m in modes):
            if texts is None or len(texts) != nq or len(modes) != nq:
                raise ValueError("one mode and one question text per question")
            bad = [m for m in modes if m not in SEARCH_MODES]
            if bad:
                raise ValueError(f"search mode must be one of {SEARCH_MODES}, got {bad[0]!r}")
            from ..index.lexical import fetch_depth

            base = fetch_depth(k)
            depth = max(base, F)
            lex = self._lexical_cols(qemb.device)
            Dd, Id = (self.index.search_scoped(qemb, depth, cols, rows) if scoped
                      else self.index.search(qemb, depth))
            qt, qw, avgdl = lex.query_rows(list(texts))
            Sl, Il = self.index.search_lexical(lex, qt, qw, avgdl, depth, scope_cols=cols, scope=rows)
            dev = Id.device
            mode = torch.tensor([SEARCH_MODES.index(m) for m in modes], dtype=torch.int32).to(dev)
            # every question fuses the leg depth it asked for: fetch_depth(k) without MMR
            own = torch.tensor([base if m is None else max(base, f) for m, f in zip(mmr, fk_h)]).to(dev)
            past = torch.arange(depth, device=dev)[None, :] >= own[:, None]
            Fv, C = ops.rank_fuse(Id.masked_fill(past, -1), Il.masked_fill(past, -1), mode, F)
            m = mode[:, None]
            Dc = torch.where(m == 0, Dd[:, :F], torch.where(m == 1, Sl[:, :F], Fv))
            miss = torch.tensor([(3.4028234663852886e38, -3.4028234663852886e38, 0.0)[SEARCH_MODES.index(md)]
                                 for md in modes], dtype=torch.float32).to(dev)
        else:
            Dc, C = (self.index.search_scoped(qemb, F, cols, rows) if scoped else self.index.search(qemb, F))
            dev = C.device
            miss = torch.full((nq,), 3.4028234663852886e38, dtype=torch.float32, device=dev)
        lam = torch.tensor(lam_h, dtype=torch.float32).to(dev)
        ncand = torch.tensor(fk_h, dtype=torch.int32).to(dev)
        _, I, P = self.index.mmr_select(qemb, C, ncand, lam, k)
        D = torch.gather(Dc, 1, P.clamp(min=0).long())
        return torch.where(P >= 0, D, miss[:, None]), I

    def retrieve(self, questions: list[str], scopes: list | None = None, modes: list | None = None,
                 mmr: list | None = None):
        """(D, I) of the questions' top-k.  On a sharded index the hits are checked for a
        failed cross-rank gather here (one host sync on the search's ids) so no caller can
        use stale peer rows unchecked."""
        q = self.embed(questions)
        D, I = self.search(q, scopes, modes, questions, mmr)
        if getattr(self.index, "check_gather", None) is not None:
            self._host_ids(I)
        return D, I

    def _new_generation(self, gen: int) -> None:
        """Row ids changed meaning: everything cached by id goes, and columns this pipeline
        built itself are rebuilt from the metadata list (an owner's are compacted by it)."""
        self._chunk_ids.clear()
        self._seen.clear()
        if self._own_scopes is not None and self._own_scopes is self.scopes:
            self.scopes.rebuild(self.metadata)
        if self._own_lexical is not None and self._own_lexical is self.lexical:
            self.lexical.rebuild(self.metadata)
        self._generation = gen

    def _resolve_ids(self, questions: list[str], I, span: str | None):
        if span is None:
            return self.build_prompts(questions, I), self._sources(I)
        with tracing.span(span, n=len(questions)):
            return self.build_prompts(questions, I), self._sources(I)

    def _even_generation(self) -> int:
        """The owner's generation once no delete is swapping.  The counter is odd only inside
        the swap's critical section under the index lock, so an odd value is waited out on that
        lock -- however long the swap takes, no retry is counted for it."""
        owner = self.owner
        g = owner.generation
        while g & 1:
            lock = getattr(self.index, "_lock", None)
            if lock is not None:
                with lock:
                    pass
            else:
                time.sleep(0)
            g = owner.generation
        return g

    def resolve(self, questions: list[str], search, span: str | None = None):
        """One batch's retrieval, safe against a concurrent delete: ``search()`` -> the hits as
        host id lists; -> (I, prompts, sources) with the ids resolved to prompts (inside the
        tracing span ``span``, if any) and to each question's sources while they still name the rows the
        search saw.  Without an owner this is search + :meth:`build_prompts` and nothing else."""
        owner = self.owner
        if owner is None:
            I = search()
            return (I, *self._resolve_ids(questions, I, span))
        for _ in range(16):                   # one round per delete that lands inside a retrieval
            g0 = self._even_generation()
            if g0 != self._generation:
                self._new_generation(g0)
            try:
                I = search()
                if self._after_search is not None:
                    self._after_search()
                prompts, sources = self._resolve_ids(questions, I, span)
            except (IndexError, KeyError):    # a list that shrank under the resolve
                if owner.generation == g0:
                    raise
                continue
            if owner.generation == g0:
                return I, prompts, sources
        raise RuntimeError("retrieval raced 16 deletes in a row")

    def _sources(self, I: list[list[int]]) -> list[list]:
        meta = self.metadata
        return [[meta[i].get("source") for i in ids if 0 <= i < len(meta)] for ids in I]

    def _piece_prompt(self, qtext: str, ids: list[int], qids: list[int] | None = None) -> list[int]:
        ct = self.chat_tok
        if not hasattr(self, "_frame"):
            s = ct.special
            head, mid, tail = self._pieces
            self._frame = ([s("<|begin_of_text|>"), s("<|start_header_id|>")] + ct.encode("user")
                           + [s("<|end_header_id|>")] + ct.encode("\n\n" + head),
                           ct.encode("\n\n"), ct.encode(mid),
                           ct.encode(tail) + [s("<|eot_id|>"), s("<|start_header_id|>")] + ct.encode("assistant")
                           + [s("<|end_header_id|>")] + ct.encode("\n\n"))
        pre, sep, mid_ids, post = self._frame
        out = list(pre)
        first = True
        for i in ids:
            if not 0 <= i < len(self.metadata):
                continue
            c = self._chunk_ids.get(i)
            if c is None:
                c = self._chunk_ids[i] = ct.encode(self.metadata[i]["text_content"])
            if not first:
                out += sep
            out += c
            first = False
        return out + mid_ids + (qids if qids is not None else ct.encode(qtext)) + post

    def _ordered(self, I: list[list[int]]) -> list[list[int]]:
        if self.context_order == "relevance":
            return I
        cnt: dict[int, int] = {}
        for ids in I:
            for i in ids:
                cnt[i] = cnt.get(i, 0) + 1
        if self.context_order == "shared":
            return [sorted(ids, key=lambda i: (-cnt[i], i)) for ids in I]
        # "trie": the permutation whose leading chunks an earlier prompt (this batch or an
        # earlier one) already used, longest match first, then batch popularity
        import itertools

        seen = self._seen
        out = []
        for ids in I:
            base = sorted(ids, key=lambda i: (-cnt[i], i))
            best, best_m = base, -1
            if len(ids) <= 4:
                for perm in itertools.permutations(base):
                    m = 0
                    while m < len(perm) and perm[:m + 1] in seen:
                        m += 1
                    if m > best_m:
                        best, best_m = list(perm), m
            for m in range(1, len(best) + 1):
                seen.add(tuple(best[:m]))
            out.append(best)
        if len(seen) > 1_000_000:
            seen.clear()
        return out

    def build_prompts(self, questions: list[str], I: list[list[int]]) -> list[list[int]]:
        I = self._ordered(I)
        if self._pieces is not None and os.environ.get("DOCQA_PROMPT_PIECES", "1") == "1":
            many = getattr(self.chat_tok, "encode_many", None)
            qids = many(questions) if many else [None] * len(questions)
            prompts = [self._piece_prompt(q, ids, qi) for q, ids, qi in zip(questions, I, qids)]
            lim = self.max_prompt_tokens
            if lim:
                prompts = [p if len(p) <= lim else p[: lim // 2] + p[-lim // 2:] for p in prompts]
            return prompts
        texts = []
        for qtext, ids in zip(questions, I):
            ctx = "\n\n".join(self.metadata[i]["text_content"] for i in ids if 0 <= i < len(self.metadata))
            texts.append(self.template.format(context=ctx, question=qtext))
        enc = getattr(self.chat_tok, "encode_batch_chat", None)
        prompts = enc(texts) if enc else [self.chat_tok.chat_prompt(t) for t in texts]
        lim = self.max_prompt_tokens
        if lim:
            prompts = [p if len(p) <= lim else p[: lim // 2] + p[-lim // 2:] for p in prompts]
        return prompts

    @torch.inference_mode()
    def answer_batch(self, questions: list[str], params: SamplingParams | None = None,
                     scopes: list | None = None, modes: list | None = None,
                     mmr: list | None = None) -> list[Answer]:
        params = params or SamplingParams(stop_on_eos=True)
        t = StageTimes()
        t0 = time.perf_counter()
        with tracing.span("rag.embed", n=len(questions)):
            qemb = self.embed(questions)
            self._sync()
        t1 = time.perf_counter()
        tm = {}

        def hits():
            with tracing.span("rag.search", n=len(questions), k=self.k):
                D, I = self.search(qemb, scopes, modes, questions, mmr)
                I = self._host_ids(I)  # host needs ids to assemble the prompts
            tm["t2"] = time.perf_counter()
            return I

        I, prompts, sources = self.resolve(questions, hits, "rag.prompt")
        t2 = tm["t2"]
        t3 = time.perf_counter()
        with tracing.span("rag.generate", n=len(prompts)):
            outs = self.engine.generate(prompts, params)
        t4 = time.perf_counter()
        t.embed_s, t.search_s, t.prompt_s, t.generate_s = t1 - t0, t2 - t1, t3 - t2, t4 - t3
        self.last_times = t
        res = []
        for ids, toks, srcs in zip(I, outs, sources):
            res.append(Answer(answer=self.chat_tok.decode(toks), sources=srcs, token_ids=toks,
                              chunk_ids=list(ids)))
        return res

    def answer(self, question: str, params: SamplingParams | None = None, scope: dict | None = None,
               mode: str | None = None, mmr: tuple | None = None) -> Answer:
        return self.answer_batch([question], params, None if scope is None else [scope],
                                 None if mode is None else [mode], None if mmr is None else [mmr])[0]

    # ------------------------------------------------------------------ pipelined
    @torch.inference_mode()
    def _prepare(self, questions: list[str], stream, gate, params=None, scopes=None, mmr=None):
        """embed + kNN on a side HIP stream (held back by ``gate`` until the running
        generation is ``lead_steps`` from its end), then host-side prompt assembly and
        (``params`` given) the batch's KV-block reservation."""
        t0 = time.perf_counter()
        evs = None
        sp = tracing.span("rag.prepare", n=len(questions))
        sp.__enter__()
        if stream is not None:
            with torch.cuda.stream(stream):
                if gate is not None:
                    stream.wait_event(gate)
                # GPU-clock stage times: embed = [e0, e1), kNN search = [e1, e2)
                evs = tuple(torch.cuda.Event(enable_timing=True) for _ in range(3))
                evs[0].record(stream)
                qemb = self.embed(questions)
                evs[1].record(stream)
        else:
            qemb = self.embed(questions)
            tm = time.perf_counter()
        stamp = {}

        def hits():
            if stream is not None:
                with torch.cuda.stream(stream):
                    _, I = self.search(qemb, scopes, mmr=mmr)
                    if "t1" not in stamp:       # a retry after a delete is not timed again
                        evs[2].record(stream)
                    I = self._host_ids(I)       # waits for this side stream only
            else:
                _, I = self.search(qemb, scopes, mmr=mmr)
                I = self._host_ids(I)
            stamp.setdefault("t1", time.perf_counter())
            return I

        I, prompts, sources = self.resolve(questions, hits, "rag.prompts")
        t1 = stamp["t1"]
        host = None if stream is not None else (tm - t0, t1 - tm)
        reserved = None
        if params is not None and len(prompts) <= self.engine.max_batch:
            try:
                reserved = self.engine.reserve(prompts, params)
            except MemoryError:
                # the batches still in flight hold the pool: the main loop collects them
                # first and reserves this batch itself (reserved=None)
                reserved = None
        sp.__exit__(None, None, None)
        return questions, I, prompts, reserved, (evs, host), t0, t1, time.perf_counter(), sources

    @torch.inference_mode()
    def answer_pipelined(self, batches: list[list[str]], params: SamplingParams | None = None,
                         lead_steps: int | None = None, scopes: list | None = None,
                         mmr: list | None = None):
        """Yield (answers, StageTimes, latency_s) per batch.  Batch i+1's embedding and
        kNN search run on a side HIP stream and its prompt assembly + KV reservation on a
        helper thread, released when batch i's decode is ``lead_steps`` steps from its
        end, so they overlap the tail of batch i's generation; batch i+1 is then launched
        (prefill + decode graphs queued behind batch i) before batch i is collected and
        detokenised on a second helper thread, so the GPU never waits on host work between
        batches.  Latency is measured on the GPU clock from the moment batch i+1's
        embedding may start to its answers being ready.  ``scopes``: per batch ``None`` or the
        list of per-question scope requests, ``mmr``: per batch ``None`` or the list of per-question
        ``(lambda_mult, fetch_k)`` entries (see :meth:`search`)."""
        import concurrent.futures as cf

        params = params or SamplingParams(stop_on_eos=True)
        # embed + kNN (side stream) + prompt assembly + KV reservation of batch i+1 should
        # finish before batch i's last decode step, so batch i+1's prefill is queued right
        # behind it (launch-before-collect below); an earlier start only adds latency
        # (measured: lead 4 / 8 / 16 steps -> 205.1 / 204.8 / 204.4 q/s, p50 1264 / 1301 /
        # 1370 ms; profiles/r2_ab_pipeline_lead.log).  Adaptive (no argument, no env): after
        # the first batch the lead is the measured preparation time over the measured decode
        # step time, x1.5 -- 1 step at batch 1 (1.5 ms of preparation vs 3.6 ms steps; a
        # fixed 4 put 11 ms of waiting into every answer's latency), 4 at batch 256
        env_lead = os.environ.get("DOCQA_PIPELINE_LEAD")
        # data-parallel ranks keep the fixed lead: their batch preparation meets in the
        # sharded index's all-gather, so every rank must release it at the same step
        dp = torch.distributed.is_available() and torch.distributed.is_initialized() and \
            torch.distributed.get_world_size() > 1
        adaptive = lead_steps is None and env_lead is None and not dp
        lead = [lead_steps if lead_steps is not None else int(env_lead or 4)]
        est = {"prep": None, "step": None}

        def adapt():
            if adaptive and est["prep"] is not None and est["step"]:
                lead[0] = max(1, min(16, math.ceil(_LEAD_MARGIN * est["prep"] / est["step"])))
        eng = self.engine
        cuda = eng.device.type == "cuda"
        stream = torch.cuda.Stream() if cuda else None
        pending = None   # (Launched, questions, I, sources, stage timers, t0, t1, t2, t3) of the batch in flight

        def stage_times(tm, t0, t1, t2, gen_s):
            evs, host = tm
            if evs is not None:
                emb, srch = evs[0].elapsed_time(evs[1]) / 1e3, evs[1].elapsed_time(evs[2]) / 1e3
            else:
                emb, srch = host if host is not None else (t1 - t0, 0.0)
            return StageTimes(embed_s=emb, search_s=srch, prompt_s=t2 - t1, generate_s=gen_s)

        def finish(p):
            h, questions, I, sources, tm, t0, t1, t2, t3 = p
            outs = eng.collect(h)
            t4 = time.perf_counter()
            if cuda:
                latency = tm[0][0].elapsed_time(h.done_event) / 1e3
                gen_s = h.start_event.elapsed_time(h.done_event) / 1e3
            else:
                latency, gen_s = t4 - t0, t4 - t3
            est["step"] = gen_s / max(1, params.max_new_tokens)
            adapt()
            st = stage_times(tm, t0, t1, t2, gen_s)
            self.last_times = st
            with tracing.span("rag.detokenise", n=len(outs)):
                res = [Answer(answer=self.chat_tok.decode(toks), sources=srcs,
                              token_ids=toks, chunk_ids=list(ids)) for ids, toks, srcs in zip(I, outs, sources)]
            return res, st, latency

        # batch i-1 is collected and detokenised on a helper thread as soon as batch i's
        # decode starts being enqueued (its prefill is queued by then): enqueueing the
        # decode graphs blocks the host on the stream's queue depth until about the end of
        # the batch, so collecting after launch() returned left the GPU idle meanwhile
        with cf.ThreadPoolExecutor(1, thread_name_prefix="rag-prep") as ex, \
                cf.ThreadPoolExecutor(1, thread_name_prefix="rag-collect") as col:
            sc = (lambda i: scopes[i]) if scopes is not None else (lambda i: None)
            mm = (lambda i: mmr[i]) if mmr is not None else (lambda i: None)
            fut = ex.submit(self._prepare, batches[0], stream, None, params, sc(0), mm(0)) if batches else None
            fin = None
            try:
                for i in range(len(batches)):
                    questions, I, prompts, reserved, tm, t0, t1, t2, sources = fut.result()
                    fut = None
                    # preparation cost, not the wait for the gate: GPU embed + search time (side
                    # stream events, complete once the host has the hits) + host prompt assembly
                    evs = tm[0] if tm is not None else None
                    est["prep"] = ((evs[0].elapsed_time(evs[2]) / 1e3 + (t2 - t1)) if evs is not None
                                   else t2 - t0)
                    adapt()
                    nxt = batches[i + 1] if i + 1 < len(batches) else None

                    nxt_sc = sc(i + 1) if nxt is not None else None
                    nxt_mm = mm(i + 1) if nxt is not None else None

                    def on_step(step, total, nxt=nxt, nxt_sc=nxt_sc, nxt_mm=nxt_mm):
                        nonlocal fut, fin, pending
                        if pending is not None and fin is None:
                            p, pending = pending, None
                            fin = col.submit(finish, p)
                        if nxt is not None and fut is None and step >= max(1, total - lead[0]):
                            gate = None
                            if cuda:
                                gate = torch.cuda.Event()
                                gate.record()
                            fut = ex.submit(self._prepare, nxt, stream, gate, params, nxt_sc, nxt_mm)

                    if reserved is None and pending is not None and len(prompts) <= eng.max_batch:
                        # no KV reservation (pool held by the batch in flight): collect that
                        # batch first so launch() can reserve this one
                        p, pending = pending, None
                        yield finish(p)
                    t3 = time.perf_counter()
                    if len(prompts) <= eng.max_batch:
                        h = eng.launch(prompts, params, on_step=on_step, reserved=reserved)
                    else:   # larger than one engine batch: plain blocking generation
                        h = None
                        outs = eng.generate(prompts, params, on_step=on_step)
                    if nxt is not None and fut is None:   # single-step generations
                        fut = ex.submit(self._prepare, nxt, stream, None, params, nxt_sc, nxt_mm)
                    if pending is not None:   # no decode step enqueued: collect batch i-1 now
                        p, pending = pending, None
                        fin = col.submit(finish, p)
                    if fin is not None:
                        f, fin = fin, None
                        yield f.result()
                    if h is not None:
                        pending = (h, questions, I, sources, tm, t0, t1, t2, t3)
                    else:
                        t4 = time.perf_counter()
                        st = stage_times(tm, t0, t1, t2, t4 - t3)
                        self.last_times = st
                        yield ([Answer(answer=self.chat_tok.decode(toks), sources=srcs, token_ids=toks,
                                       chunk_ids=list(ids))
                                for ids, toks, srcs in zip(I, outs, sources)], st, t4 - t0)
                if pending is not None:
                    p, pending = pending, None
                    yield finish(p)
            finally:
                if fin is not None:
                    try:
                        fin.result()
                    except Exception:
                        pass
                if pending is not None:   # abandoned generator: wait, free the blocks
                    eng.collect(pending[0])
                if fut is not None:
                    try:
                        r = fut.result()[3]
                        if r is not None:
                            eng.release(r)
                    except Exception:
                        pass


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
