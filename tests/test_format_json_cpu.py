"""format: "json" without a GPU: the automaton against Python's json module, the reference ops
against a brute-force walk, ChatTokenizer.token_bytes, the engine (static batcher and the
scheduler with the GPU's lagged readback) on the tiny CPU preset, and the Ollama routes.

All comparisons are exact: sets of allowed ids, int64 states, token ids."""
from __future__ import annotations

import json
import random

import pytest
import torch

from docqa_amd import ops
from docqa_amd.config import Settings
from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
from docqa_amd.engine.scheduler import ContinuousEngine
from docqa_amd.models.llama import LlamaConfig, LlamaModel
from docqa_amd.ops import grammar as G
from tests.format_json_common import (EOS_SYN, SAMPLE_DOCS, brute_allowed, coverage_states, engine_vocab,
                                      gen_documents, max_ws_run, mutate, states_tensor, synthetic_vocab, vocab_on)


# ------------------------------------------------------------------ the automaton
def test_automaton_accepts_json_dumps_documents():
    docs = gen_documents(6000)
    over = [d for d in docs if max_ws_run(d) > G.WS_CAP]
    assert 0 < len(over) <= 0.02 * len(docs), len(over)           # a condition of the test: at most 2 %
    for d in docs:
        s = G.walk(G.START_STATE, d)
        if max_ws_run(d) <= G.WS_CAP:
            assert s >= 0 and G.is_done(s), d
        else:
            assert s < 0, d
    for d in SAMPLE_DOCS:
        assert G.accepts(d), d


def test_automaton_is_sound_under_mutations():
    rng = random.Random(3)
    n = accepted = 0
    for d in gen_documents(4000, seed=1):
        for _ in range(10):
            m = mutate(d, rng)
            n += 1
            if G.accepts(m):
                accepted += 1
                assert isinstance(json.loads(m.decode("utf-8")), dict), m
    assert n >= 40000 and accepted >= 0.05 * n, (n, accepted)


@pytest.mark.parametrize("bad", [b'[]', b'{"a":NaN}', b'{"a":Infinity}', b'{"a":01}', b'{"a":1,}', b'{"a" 1}', b'{} ',
                                 b' {}', b'{"a":"\x01"}', b'{"a":"\xed\xa0\x80"}', b'{"a":"\xc0\xaf"}', b'{"a":[1}',
                                 b'{"a":1.}', b'{"a":-}', b'{"a":1e}', b'{"\\x":1}', b'{"a":"\\u12g4"}', b'{"a":tru}',
                                 b'{"a":"\xf4\x90\x80\x80"}', b'{,}', b'{"a":1}}', b'"a"', b'{"a":+1}', b'{"a":.5}'])
def test_automaton_rejects(bad):
    assert not G.accepts(bad)


def test_caps():
    assert G.accepts(b'{' + b' ' * G.WS_CAP + b'}') and not G.accepts(b'{' + b' ' * (G.WS_CAP + 1) + b'}')
    assert G.accepts(b'{"s":"' + b' ' * 40 + b'"}')                # inside a string it is no whitespace run
    deep = lambda n: b'{"a":' + b'[' * (n - 1) + b']' * (n - 1) + b'}'   # noqa: E731
    assert G.accepts(deep(G.DEPTH_CAP)) and not G.accepts(deep(G.DEPTH_CAP + 1))
    # a number's delimiter is processed in the same step
    assert G.accepts(b'{"a":[1,2 ,3]}') and G.accepts(b'{"a":1}') and G.accepts(b'{"a":1\n}')
    assert G.is_done(G.walk(G.START_STATE, b'{}')) and G.walk(G.walk(G.START_STATE, b'{}'), b' ') < 0


def test_no_dead_state():
    """Every lexer state but DONE accepts some byte, at whitespace run 0 and at the cap, depth 1
    and at the cap, top object and array.  START exists only at depth 0 and is checked there."""
    assert G.N_STATES <= G.MAX_STATES
    assert any(G.step(G.START_STATE, b) >= 0 for b in range(256))
    for lex in range(1, G.N_STATES):
        if lex in (G.DONE, G.START):
            continue
        for ws in (0, G.WS_CAP):
            for depth in (1, G.DEPTH_CAP):
                for top in (0, 1):
                    s = G.pack(lex, ws, depth, top << (depth - 1))
                    assert any(G.step(s, b) >= 0 for b in range(256)), (G.STATE_NAMES[lex], ws, depth, top)
    assert all(G.step(G.pack(G.DONE), b) < 0 for b in range(256))


def test_table_is_shared_shape():
    t = G.table()
    assert t.dtype == torch.int16 and tuple(t.shape) == (G.N_STATES, 256)
    assert bool((t[0] >> 8 == G.OP_REJECT).all()) and bool((t[G.DONE] >> 8 == G.OP_REJECT).all())


# ------------------------------------------------------------------ reference ops
def test_reference_mask_and_advance_match_brute_force():
    toks = list(synthetic_vocab())
    V = len(toks)
    assert 2000 <= V <= 4000 and V % 64 != 0
    off, data, table = vocab_on("cpu")
    states = list(coverage_states())
    assert {s & 0xFF for s in states} == set(range(1, G.N_STATES))
    x0 = torch.randn(len(states) + 2, V + 5)
    x = x0.clone()
    st = states_tensor(states + [0, states[3]], "cpu")
    valid = torch.ones(len(states) + 2, dtype=torch.int32)
    valid[-1] = 0
    ops.grammar_mask(x, V, st, off, data, table, EOS_SYN, valid)
    for r, s in enumerate(states):
        want = brute_allowed(s, toks, EOS_SYN, V)
        assert (x[r, :V] != -float("inf")).tolist() == want, G.STATE_NAMES[s & 0xFF]
        assert any(want)                                          # no state is left without a token
        assert want[EOS_SYN] == G.is_done(s)
    keep = x != -float("inf")
    assert torch.equal(x[keep], x0[keep]) and torch.equal(x[-2:], x0[-2:]) and torch.equal(x[:, V:], x0[:, V:])
    # advance: every (state, token) pair
    for s in states:
        got = torch.full((V,), s, dtype=torch.int64)
        ops.grammar_advance(got, torch.arange(V), off, data, table, EOS_SYN)
        assert got.tolist() == [G.advance_token(s, t, toks, EOS_SYN) for t in range(V)]
    z = torch.tensor([0, states[0], G.pack(G.DONE)], dtype=torch.int64)
    ops.grammar_advance(z, torch.tensor([300, 300, EOS_SYN]), off, data, table, EOS_SYN,
                        torch.tensor([1, 0, 1], dtype=torch.int32))
    assert z.tolist() == [0, states[0], G.pack(G.DONE)]


def test_vocab_tensors_need_every_single_byte():
    toks = list(synthetic_vocab())
    toks[3 + 0x41] = b""
    with pytest.raises(ValueError):
        G.vocab_tensors(toks)


# ------------------------------------------------------------------ token bytes
def test_token_bytes_invert_the_byte_level_alphabet():
    from docqa_amd.text.tokenizer import ChatTokenizer

    tok = ChatTokenizer()
    tb = tok.token_bytes()
    assert len(tb) == tok.model_vocab
    assert {bytes([i]) for i in range(256)} <= set(tb)
    checked = 0
    for i, b in enumerate(tb):
        if not b:
            continue
        try:
            text = b.decode("utf-8")
        except UnicodeDecodeError:
            continue
        assert text == tok.decode([i]), i
        checked += 1
    assert checked > 1000
    for name in ("<|begin_of_text|>", "<|eot_id|>", "<|end_of_text|>", "<|start_header_id|>"):
        assert tb[tok.special(name)] == b""
    assert tb[-1] == b"" and len(tok.token_bytes(512)) == 512


# ------------------------------------------------------------------ engine
def _model(seed=7):
    cfg = LlamaConfig(name="tiny-gqa4", vocab_size=4096, hidden=256, intermediate=512, layers=2,
                      heads=8, kv_heads=2, head_dim=128, max_position=2048, bos_token_id=1, eos_token_id=2)
    return LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=seed)


VOCAB = engine_vocab(4096)
EOS = 2


def _prompts(lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, 4096, (int(n),), generator=g).tolist() for n in lens]


def _engine(m, vocab=True, **kw):
    e = LLMEngine(m, max_batch=8, max_context=256, block_size=16, use_graphs=False, prefix_cache=False, **kw)
    if vocab:
        e.set_vocab_bytes(VOCAB)
    return e


def check_constrained(out: list, max_new: int) -> bool:
    """Replay a constrained output: every token allowed at its step, EOS only in DONE; an output
    that ended on EOS parses.  Returns whether it finished on EOS."""
    s = G.START_STATE
    for t in out:
        assert G.token_allowed(s, t, VOCAB, EOS), (t, VOCAB[t], G.STATE_NAMES[s & 0xFF])
        s = G.advance_token(s, t, VOCAB, EOS)
    if out[-1] == EOS:
        assert G.is_done(s)
        assert isinstance(json.loads(b"".join(VOCAB[t] for t in out).decode("utf-8")), dict)
        return True
    assert len(out) == max_new
    return False


FLAVOURS = {
    "greedy": dict(),
    "penalised": dict(repeat_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2, repeat_last_n=32),
    "sampled": dict(temperature=4.0, seed=11),
    "logprobs": dict(logprobs=True, top_logprobs=3),
}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_static_batcher_constrains_every_row(flavour):
    m = _model()
    sp = SamplingParams(max_new_tokens=24, format="json", **FLAVOURS[flavour])
    eng = _engine(m)
    prompts = _prompts((20, 31, 12))
    if sp.logprobs:
        outs, lps = eng.generate_with_logprobs(prompts, sp)
        assert all(len(o) == len(l) for o, l in zip(outs, lps))
    else:
        outs = eng.generate(prompts, sp)
    assert eng._graphs_json and not eng._graphs and not eng._graphs_min_p
    for o in outs:
        check_constrained(o, sp.max_new_tokens)


def _run_mixed(m, with_constrained: bool, **kw):
    """Six requests through one scheduler with the GPU's lagged readback: constrained greedy,
    penalised, sampled, greedy with logprobs -- and two unconstrained greedy ones (one with
    logprobs) in the same batch."""
    pr = _prompts((20, 31, 12, 25, 18, 9))
    specs = [SamplingParams(max_new_tokens=24, format="json", **FLAVOURS[f])
             for f in ("greedy", "penalised", "sampled", "logprobs")]
    free = [SamplingParams(max_new_tokens=24, stop_on_eos=False),
            SamplingParams(max_new_tokens=24, stop_on_eos=False, logprobs=True, top_logprobs=2)]
    ce = ContinuousEngine(_engine(m, **kw))
    ce.lag_cpu = True
    futs = []
    if with_constrained:
        futs = [ce.submit(p, sp) for p, sp in zip(pr[:4], specs)]
        ce.step()
    ffree = [ce.submit(p, sp) for p, sp in zip(pr[4:], free)]
    while ce.has_work():
        ce.step()
    return ce, futs, ffree, specs


def test_scheduler_mixed_batch():
    m = _model()
    ce, futs, ffree, specs = _run_mixed(m, True)
    assert any(len(k) == 7 and k[-1] == "json" for k in ce._graphs)
    for f, sp in zip(futs, specs):
        check_constrained(f.result(), sp.max_new_tokens)
    # the unconstrained rows are what they are without constrained neighbours
    ce0, _, ffree0, _ = _run_mixed(m, False)
    assert all(len(k) == 6 for k in ce0._graphs)                  # no constrained flavour was created
    assert [f.result() for f in ffree] == [f.result() for f in ffree0]
    assert ffree[1].request.logprobs == ffree0[1].request.logprobs


def test_scheduler_logprobs_come_from_the_unmasked_logits(monkeypatch):
    """A constrained request's logprobs are ops.token_logprobs of the very logits each step
    masks, taken before the mask: exact."""
    m = _model()
    sp = SamplingParams(max_new_tokens=10, format="json", logprobs=True, top_logprobs=4)
    p = _prompts((22,), seed=4)[0]
    seen, real = [], ops.grammar_mask

    def spy(logits, *a, **k):
        seen.append(logits.clone())                               # as the LM head wrote them
        return real(logits, *a, **k)

    monkeypatch.setattr(ops, "grammar_mask", spy)
    ce = ContinuousEngine(_engine(m))
    ce.lag_cpu = True
    f = ce.submit(p, sp)
    while ce.has_work():
        ce.step()
    out, lps = f.result(), f.request.logprobs
    assert len(lps) == len(out) <= len(seen)                      # + the extra lagged step
    for t, (lp, top), x in zip(out, lps, seen):
        assert bool(torch.isfinite(x).all())
        wlp, wid, wtop = ops.token_logprobs(x[:1], 4096, torch.tensor([t]), torch.tensor([4], dtype=torch.int32))
        assert lp == float(wlp[0])
        assert top == [(int(i), float(v)) for i, v in zip(wid[0, :4], wtop[0, :4])]
    # the model's own favourite is usually not a JSON token: the logprobs were not renormalised
    assert any(top[0][0] != t for t, (_, top) in zip(out, lps))


def test_sampled_constrained_requests_finish_on_eos():
    m = _model()
    ce = ContinuousEngine(_engine(m))
    ce.lag_cpu = True
    p = _prompts((16,), seed=2)[0]
    futs = [ce.submit(p, SamplingParams(max_new_tokens=48, format="json", temperature=4.0, seed=s))
            for s in range(1, 9)]
    while ce.has_work():
        ce.step()
    done = [check_constrained(f.result(), 48) for f in futs]
    assert sum(done) * 4 >= len(done), done


def test_preempted_constrained_request_resumes_its_state():
    m = _model()
    pr = _prompts((28, 20, 35, 9, 50, 17))
    a = SamplingParams(max_new_tokens=40, format="json", stop_on_eos=False)
    others = [SamplingParams(max_new_tokens=n, stop_on_eos=False) for n in (30, 40, 25, 40, 35)]
    alone = ContinuousEngine(_engine(m)).generate([pr[0]], a)[0]
    ce = ContinuousEngine(_engine(m, num_blocks=20), max_running=8)
    ce.lag_cpu = True
    for p, sp in zip(pr[1:], others):
        ce.submit(p, sp)
    fa = ce.submit(pr[0], a)                      # the latest arrival: the first to be preempted
    while ce.has_work():
        ce.step()
    assert ce.preempted > 0 and fa.request.preemptions > 0
    assert fa.result() == alone


def test_constrained_request_needs_vocab_bytes_and_plain_steps(monkeypatch):
    m = _model()
    sp = SamplingParams(max_new_tokens=4, format="json")
    p = _prompts((10,))[0]
    with pytest.raises(ValueError):
        _engine(m, vocab=False).generate([p], sp)
    with pytest.raises(ValueError):
        ContinuousEngine(_engine(m, vocab=False)).submit(p, sp)
    monkeypatch.setenv("DOCQA_MIXED_PREFILL", "1")
    ce = ContinuousEngine(_engine(m))
    assert ce.mixed
    with pytest.raises(ValueError):
        ce.submit(p, sp)
    with pytest.raises(ValueError):
        SamplingParams(format="yaml")


# ------------------------------------------------------------------ service
def _stack(tmp_path):
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = Settings()
    st.index_dir = str(tmp_path)
    st.default_data_dir = str(tmp_path / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 6
    st.serving_mode = "continuous"
    return DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu",
                                   max_batch=4, max_context=1024, use_graphs=False), st)


def test_service_format(tmp_path):
    from fastapi.testclient import TestClient

    s = _stack(tmp_path)
    try:
        qa = TestClient(s.qa_app)
        eng, tok = s.pipeline.engine, s.pipeline.chat_tok
        assert eng.vocab_bytes is not None
        stops = 0
        for seed in range(1, 7):
            opts = {"temperature": 3.0, "seed": seed, "num_predict": 40}
            r = qa.post("/api/chat", json={"model": "mistral", "format": "json", "stream": False, "options": opts,
                                           "messages": [{"role": "user", "content": "Rate ?"}]})
            assert r.status_code == 200
            d = r.json()
            assert d["done_reason"] in ("stop", "length")
            if d["done_reason"] == "stop":
                stops += 1
                assert isinstance(json.loads(d["message"]["content"]), dict)
            else:
                assert d["eval_count"] == 40
            r = qa.post("/api/generate", json={"prompt": "Rate ?", "format": "json", "stream": True, "options": opts})
            assert r.status_code == 200
            lines = [json.loads(x) for x in r.text.splitlines() if x]
            text = "".join(x.get("response", "") for x in lines)
            if lines[-1]["done_reason"] == "stop":
                stops += 1
                assert isinstance(json.loads(text), dict)
        assert stops > 0
        ok = qa.post("/api/chat", json={"format": {"type": "object", "properties": {"a": {"type": "string"}}},
                                        "stream": False, "options": {"num_predict": 4},
                                        "messages": [{"role": "user", "content": "x"}]})
        assert ok.status_code == 200 and ok.json()["message"]["content"].lstrip().startswith("{")
        for bad in ("yaml", 3):
            for route, body in (("/api/chat", {"messages": [{"role": "user", "content": "x"}]}),
                                ("/api/generate", {"prompt": "x"})):
                r = qa.post(route, json={**body, "format": bad, "stream": False})
                assert r.status_code == 400 and "format" in r.json()["error"]
        # no format: the completion of the engine itself (greedy)
        for fmt in ({}, {"format": None}, {"format": ""}):
            r = qa.post("/api/generate", json={"prompt": "Vide de Qi ?", "stream": False,
                                               "options": {"num_predict": 8}, **fmt})
            ids = tok.chat_prompt("Vide de Qi ?")
            want = eng.generate([ids], SamplingParams(max_new_tokens=8))[0]
            assert r.status_code == 200 and r.json()["response"] == tok.decode(want)
    finally:
        s.close()
