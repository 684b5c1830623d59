"""format: a JSON schema, on the GPU: the schema kernels against the CPU reference (exact) over
every DFA state of a small schema and of one near the size cap, and the HIP-graph scheduler end to
end with rows on two schemas, plain-JSON rows and free rows."""
from __future__ import annotations

import functools
import json

import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import grammar as G
from docqa_amd.ops import json_schema as J
from docqa_amd.ops import reference as ref
from tests.format_json_common import EOS_SYN
from tests.format_schema_common import (SERVICE_SCHEMA, SMALL_SCHEMA, big_schema, cases, coverage_words,
                                        schema_engine_vocab, schema_vocab)

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
NEG = -float("inf")
N_SLOTS = 4


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True), "native extension missing"


@functools.lru_cache(maxsize=3)
def _vocab(kind: str):
    """(token bytes, eos id, n_valid, ld) of the vocabularies: the synthetic one tiled over three
    of the kernel's 4096-column chunks with a ragged last one ("syn1": one tile of it, every
    distinct token once), and the shipped tokenizer."""
    if kind.startswith("syn"):
        toks = list(schema_vocab(tiles=1 if kind == "syn1" else 3))
        assert kind == "syn1" or 2 * 4096 < len(toks) < 3 * 4096
        assert len(toks) % 64 != 0 and {48, 64} <= {len(t) for t in toks}
        return toks, EOS_SYN, len(toks), len(toks) + 24
    from docqa_amd.text.tokenizer import ChatTokenizer

    tok = ChatTokenizer()
    return tok.token_bytes(32000), tok.tok.token_to_id("<|eot_id|>"), 32000, 32768


@functools.lru_cache(maxsize=1)
def _pool():
    """Slots 0, 1 and 3 hold the service schema, the Answer model's and the near-cap one; slot 2
    holds nothing.  -> (pool on the CPU, {slot: compiled schema})."""
    by_slot = {0: J.compile_schema(SERVICE_SCHEMA), 1: J.compile_schema(cases()["Answer"][0]),
               3: J.compile_schema(big_schema())}
    pool = J.pool_new(N_SLOTS)
    for slot, cs in by_slot.items():
        J.pool_put(pool, slot, cs)
    return pool, by_slot


@functools.lru_cache(maxsize=1)
def _all_words() -> tuple:
    _, by_slot = _pool()
    return tuple(w for slot, cs in by_slot.items() for w in coverage_words(cs, slot))


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _rows(R: int):
    """Words and valid flags of an R-row bucket: states of the three slots in turn (a stride that
    walks through all of them); the 256-row bucket mixes in word-0 rows, valid-0 rows, DONE rows
    and rows whose slot holds nothing."""
    words = _all_words()
    pick = [words[(i * 7919) % len(words)] for i in range(R)]
    valid = [1] * R
    if R >= 256:
        for i in range(0, R, 5):
            pick[i] = 0
        for i in range(3, R, 7):
            valid[i] = 0
        for i in range(4, R, 11):
            pick[i] = J.pack(J.DONE, 0, (0, 1, 3)[i % 3])
        pick[9] = J.pack(J.START, 0, 2)
        assert {J.unpack(w)[2] for w in pick if w} == {0, 1, 2, 3}
    return pick, valid


def _check_mask(kind, words, valid, dt, use_valid):
    toks, eos, n_valid, ld = _vocab(kind)
    pool, _ = _pool()
    off, data = G.vocab_tensors(toks)
    R = len(words)
    g = torch.Generator().manual_seed(R)
    x0 = (torch.randn(R, ld, generator=g) * 4).to(DTYPES[dt])
    want = x0.clone()
    st, vl = torch.tensor(words, dtype=torch.int64), torch.tensor(valid, dtype=torch.int32)
    ref.schema_mask(want, n_valid, st, off, data, pool, eos, vl)
    got = x0.to(DEV)
    ops.schema_mask(got, n_valid, st.to(DEV), off.to(DEV), data.to(DEV), pool.to(DEV), eos,
                    vl.to(DEV) if use_valid else None)
    got = got.cpu()
    # the set of -inf columns is the reference's and every other element is the input's, bit for bit
    assert torch.equal(_bits(got), _bits(want))
    masked = want.float() == NEG
    assert torch.equal(_bits(got)[~masked], _bits(x0)[~masked])
    for r, (w, v) in enumerate(zip(words, valid)):
        if w == 0 or v == 0:
            assert not masked[r].any()
        elif J.unpack(w)[2] == 2:
            assert masked[r, :n_valid].all() and not masked[r, n_valid:].any()     # an empty slot allows nothing
        else:
            assert masked[r, :n_valid].any() and not masked[r, :n_valid].all() and not masked[r, n_valid:].any()
            assert bool(masked[r, eos]) != J.is_done(w)


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("R", (1, 3, 33, 256))
@pytest.mark.parametrize("kind", ("syn", "chat"))
def test_schema_mask_matches_reference(native, kind, R, dt):
    words, valid = _rows(R)
    _check_mask(kind, words, valid, dt, use_valid=R >= 256)


@pytest.mark.parametrize("slot,dt", [(0, "bf16"), (0, "fp32"), (1, "fp32"), (3, "bf16")])
def test_schema_mask_and_advance_every_state(native, slot, dt):
    """Every DFA state of the small schemas and of the one near the cap, at whitespace runs 0 and
    WS_CAP: one mask row each, and the word after every token (the 11000 rows of the large one
    over one tile of the vocabulary, which has every distinct token)."""
    _, by_slot = _pool()
    words = coverage_words(by_slot[slot], slot)
    assert len(words) == 2 * (by_slot[slot].n_states - 1)
    toks, eos, n_valid, ld = _vocab("syn" if slot == 0 else "syn1")
    pool, _ = _pool()
    off, data = G.vocab_tensors(toks)
    st = torch.tensor(words, dtype=torch.int64)
    # the reference over this many rows as one boolean matrix: no [R, ld] float reference copy
    off_np, data_np, pool_np = off.numpy(), data.numpy(), pool.numpy()
    tables = J.pool_tables(pool_np, slot)
    dev = [t.to(DEV) for t in (off, data, pool)]
    x = torch.zeros(len(words), ld, dtype=DTYPES[dt], device=DEV)
    ops.schema_mask(x, n_valid, st.to(DEV), *dev, eos)
    got = (x == NEG).cpu()
    assert not got[:, n_valid:].any() and bool((x[~got.to(DEV)] == 0).all())
    V = len(_vocab("syn1")[0])                   # advance: every distinct token, EOS and empty ones included
    after = st.to(DEV).repeat_interleave(V)
    ops.schema_advance(after, torch.arange(V, device=DEV).repeat(len(words)), *dev, eos)
    after = after.view(len(words), V).cpu()
    moved = 0
    for r, w in enumerate(words):
        allowed, nxt = ref._schema_walk(w, n_valid, off_np, data_np, tables, eos)
        assert torch.equal(got[r, :n_valid], torch.from_numpy(~allowed)), J.unpack(w)
        assert torch.equal(after[r], torch.from_numpy(nxt[:V])), J.unpack(w)
        moved += int((nxt[:V] != w).sum())
    assert moved > len(words)


def test_schema_advance_matches_reference(native):
    toks, eos, n_valid, _ = _vocab("syn")
    V = len(toks) // 3 + 40                      # one tile of the vocabulary: every distinct token
    pool, by_slot = _pool()
    off, data = G.vocab_tensors(toks)
    # (every state against the vectorised walk: test_schema_mask_and_advance_every_state; here the
    # reference op itself on a sample of each slot's states)
    words = coverage_words(by_slot[0], 0)[::2] + coverage_words(by_slot[1], 1)[::31] + coverage_words(by_slot[3], 3)[::997]
    st = torch.tensor(words, dtype=torch.int64).repeat_interleave(V)
    nxt = torch.arange(V).repeat(len(words))
    want = st.clone()
    ref.schema_advance(want, nxt, off, data, pool, eos)
    got = st.to(DEV)
    ops.schema_advance(got, nxt.to(DEV), off.to(DEV), data.to(DEV), pool.to(DEV), eos)
    assert torch.equal(got.cpu(), want)
    moved = want != st
    assert int(moved.sum()) > len(words)
    assert bool(((want >> 21) == (st >> 21)).all())               # the slot stays in the word
    empty = torch.tensor([len(toks[t]) == 0 for t in range(V)]).repeat(len(words))
    assert not moved[empty].any() and not moved[nxt == eos].any()
    # word 0, valid 0, DONE, out-of-table ids, an empty slot and a slot past the pool stay
    w0 = words[0]
    z0 = [0, w0, w0, w0, J.pack(J.DONE, 0, 1), J.pack(J.START, 0, 2), J.pack(J.START, 0, 77)]
    z = torch.tensor(z0, dtype=torch.int64, device=DEV)
    ops.schema_advance(z, torch.tensor([300, 3 + 0x7B, len(toks) + 5, -1, 3 + 0x7B, 3 + 0x7B, 3 + 0x7B], device=DEV),
                       off.to(DEV), data.to(DEV), pool.to(DEV), eos,
                       torch.tensor([1, 0, 1, 1, 1, 1, 1], dtype=torch.int32, device=DEV))
    assert z.tolist() == z0


# ------------------------------------------------------------------ HIP-graph scheduler
@pytest.fixture(scope="module")
def model(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    return LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=23)


def test_scheduler_graphs_run_the_schema_pair_for_the_rows_that_ask(model, monkeypatch):
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.engine.scheduler import ContinuousEngine
    from tests.native_trace import record

    vocab, eos = schema_engine_vocab(32000), 2
    oracle = cases()["service"][1]
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(3, 32000, (n,), generator=g).tolist() for n in (40, 23, 77, 5, 30, 51, 18, 64)]
    A, B = SERVICE_SCHEMA, SMALL_SCHEMA
    # fixed lengths (no EOS stop: a closed document goes on picking EOS, the one token DONE allows), so
    # the batch has the same rows at every step whether or not requests 0..3 carry a schema
    kw = dict(format="json", stop_on_eos=False)
    seeded = SamplingParams(max_new_tokens=16, json_schema=A, temperature=0.8, top_k=4, seed=99, **kw)
    sch = {0: SamplingParams(max_new_tokens=14, json_schema=A, **kw),
           1: seeded,
           2: SamplingParams(max_new_tokens=12, json_schema=B, repeat_penalty=1.3, presence_penalty=0.4,
                             repeat_last_n=32, logprobs=True, top_logprobs=2, **kw),
           3: SamplingParams(max_new_tokens=J.compile_schema(B).max_document_len() + 1, json_schema=B,
                             logprobs=True, top_logprobs=3, **kw)}
    which = {0: A, 1: A, 2: B, 3: B}
    rest = {4: SamplingParams(max_new_tokens=12, **kw),
            5: SamplingParams(max_new_tokens=10, temperature=0.7, seed=5, **kw),
            6: SamplingParams(max_new_tokens=12, stop_on_eos=False),
            7: SamplingParams(max_new_tokens=9, stop_on_eos=False, logprobs=True, top_logprobs=2)}

    def serve(reqs: dict):
        eng = LLMEngine(model, max_batch=8, max_context=256, use_graphs=True, prefix_cache=False)
        eng.set_vocab_bytes(vocab)
        ce = ContinuousEngine(eng)
        trace: list = []
        steps = []                       # per scheduler step: (schema rows in it, native ops launched)

        def step():
            n0 = len(trace)
            had = any(r.params.schema_constrained for r in list(ce.running) + list(ce.waiting))
            ce.step()
            steps.append((had, {t[0] for t in trace[n0:]}))

        with record(trace):
            futs = {}
            for i, sp in reqs.items():
                futs[i] = ce.submit(prompts[i], sp)
                for _ in range(i % 3):
                    step()
            while ce.has_work():
                step()
        names = {t[0] for t in trace}
        return ce, {i: f.result() for i, f in futs.items()}, {i: f.request.logprobs for i, f in futs.items()}, \
            names, steps

    ce, out, lps, names, steps = serve({**sch, **rest})
    assert {"schema_mask", "schema_advance", "grammar_mask", "grammar_advance"} <= names
    assert any(k[-1] == "schema" and gr.graph is not None for k, gr in ce._graphs.items())
    # the schema kernels only in steps that have (or admit) schema rows; request 3 outlives the
    # others, so the batch also runs steps with schema rows alone
    assert all(had for had, ops_ in steps if ops_ & {"schema_mask", "schema_advance"})
    assert any(ops_ and not ops_ & {"schema_mask", "schema_advance"} for _, ops_ in steps)
    for i, sp in sch.items():
        cs = J.compile_schema(which[i])
        w = J.start_state()
        for t in out[i]:
            assert J.token_allowed(cs, w, t, vocab, eos), (i, t, vocab[t], J.unpack(w))
            w = J.advance_token(cs, w, t, vocab, eos)
        assert len(out[i]) == sp.max_new_tokens
        if eos in out[i]:
            assert J.is_done(w) and set(out[i][out[i].index(eos):]) == {eos}
            doc = b"".join(vocab[t] for t in out[i])
            assert J.accepts(cs, doc) and isinstance(json.loads(doc.decode()), dict)
            assert which[i] is not A or oracle(doc)
        assert len(lps[i]) == (len(out[i]) if sp.logprobs else 0)
    # its token budget covers the longest document of schema B: request 3 closed its object
    assert eos in out[3]
    for i in (4, 5):
        s = G.START_STATE
        for t in out[i]:
            assert G.token_allowed(s, t, vocab, eos)
            s = G.advance_token(s, t, vocab, eos)
    # free and plain-JSON rows: what they get without the schema requests; such a batch creates no
    # schema-flavour graph and launches neither schema kernel
    plain = {i: SamplingParams(max_new_tokens=sp.max_new_tokens, stop_on_eos=False) for i, sp in sch.items()}
    ce0, out0, lps0, names0, _ = serve({**plain, **rest})
    assert not names0 & {"schema_mask", "schema_advance"} and {"grammar_mask", "grammar_advance"} <= names0
    assert all(len(k) == 6 or k[-1] == "json" for k in ce0._graphs) and ce0.eng.schema_slots.uploads == 0
    assert {i: out0[i] for i in rest} == {i: out[i] for i in rest} and lps0[7] == lps[7]
    assert any(out0[i] != out[i] for i in sch)
    # a seeded schema request alone
    _, alone, _, _, _ = serve({1: seeded})
    assert alone[1] == out[1]
