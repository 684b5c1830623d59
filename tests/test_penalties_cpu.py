"""Repeat / presence / frequency penalties and stop strings, CPU side: the engine against a
plain Python loop (full-logit forward, llama.cpp's penalty formula in fp32, argmax or the
reference sampler), neutrality of the defaults, tensor parallelism (2 gloo ranks), the
Ollama options / stop-string handling of the llm-qa routes and the scheduler's stop_check."""
import collections
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from docqa_amd import ops
from docqa_amd.config import Settings
from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
from docqa_amd.engine.scheduler import ContinuousEngine
from docqa_amd.models.llama import LlamaConfig, LlamaModel
from docqa_amd.ops import reference as ref


def _model(seed=3):
    return LlamaModel(LlamaConfig.preset("tiny"), device="cpu", dtype=torch.float32, seed=seed)


def _prompt(seed, n=40, vocab=4096):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(3, vocab, (n,), generator=g).tolist()


def _engine(m, **kw):
    return LLMEngine(m, max_batch=4, max_context=512, block_size=16, use_graphs=False, prefix_cache=False, **kw)


def _last_logits(eng, seq):
    """fp32 logits [V] of the token after ``seq``: a full prefill of the sequence."""
    r = eng.reserve([seq], SamplingParams(max_new_tokens=1))
    try:
        with torch.inference_mode():
            lg = eng._prefill([seq], r.tables, r.cached)
            return eng.model.full_logits(lg)[0].float().clone()
    finally:
        eng.release(r)


def _penalize(x, window, rp, pp, fp):
    """The issue's formula on the fp32 numpy row ``x``, every operation rounded to fp32."""
    rp, pp, fp = np.float32(rp), np.float32(pp), np.float32(fp)
    for t, c in collections.Counter(window).items():
        if not 0 <= t < x.shape[0]:
            continue
        l = x[t]
        l = l * rp if l <= 0 else l / rp
        x[t] = l - (np.float32(c) * fp + pp)
    return x


def _loop(m, prompt, sp: SamplingParams):
    eng = _engine(m)
    seq, out = list(prompt), []
    if sp.temperature > 0 and sp.seed:
        torch.manual_seed(sp.seed)
    for _ in range(sp.max_new_tokens):
        x = _last_logits(eng, seq).numpy().astype(np.float32)
        n = sp.repeat_last_n if 0 <= sp.repeat_last_n <= ops.PENALTY_WINDOW else ops.PENALTY_WINDOW
        window = seq[len(seq) - min(n, len(seq)):] if n else []
        x = torch.from_numpy(_penalize(x, window, sp.repeat_penalty, sp.presence_penalty, sp.frequency_penalty))
        if sp.temperature > 0:
            u = torch.rand(1)
            t = int(ref.sample(x[None], torch.tensor([1.0 / sp.temperature]), torch.tensor([sp.top_k], dtype=torch.int32),
                               torch.tensor([sp.top_p]), u)[0])
        else:
            t = int(x.argmax())
        seq.append(t)
        out.append(t)
    return out


def test_sampling_params_default_is_neutral():
    assert SamplingParams().neutral and SamplingParams().fused_greedy_ok
    assert not SamplingParams(repeat_penalty=1.1).neutral
    assert not SamplingParams(presence_penalty=0.5).neutral and not SamplingParams(frequency_penalty=0.1).neutral
    assert SamplingParams(repeat_penalty=1.3, presence_penalty=1.0, repeat_last_n=0).neutral
    assert not SamplingParams(temperature=0.7).fused_greedy_ok
    assert ops.PENALTY_WINDOW == 256


@pytest.mark.parametrize("seed", [0, 1])
def test_engine_penalised_greedy_equals_python_loop(seed):
    m = _model()
    sp = SamplingParams(max_new_tokens=24, stop_on_eos=False, repeat_penalty=1.3, frequency_penalty=0.2,
                        repeat_last_n=16)
    p = _prompt(seed)
    got = _engine(m).generate([p], sp)[0]
    assert got == _loop(m, p, sp)
    # the penalties matter on this prompt: the unpenalised greedy decode differs
    assert got != _engine(m).generate([p], SamplingParams(max_new_tokens=24, stop_on_eos=False))[0]


def test_engine_penalised_sampling_equals_python_loop():
    m = _model()
    sp = SamplingParams(max_new_tokens=16, stop_on_eos=False, temperature=0.8, top_k=50, top_p=0.95, seed=11,
                        repeat_penalty=1.3, frequency_penalty=0.2, repeat_last_n=16)
    p = _prompt(2)
    assert _engine(m).generate([p], sp)[0] == _loop(m, p, sp)


def test_neutral_run_equals_run_without_the_fields():
    m = _model()
    prompts = [_prompt(s, n) for s, n in ((0, 40), (1, 23), (2, 31))]
    base = _engine(m).generate(prompts, SamplingParams(max_new_tokens=12, stop_on_eos=False))
    eng = _engine(m)
    same = eng.generate(prompts, SamplingParams(max_new_tokens=12, stop_on_eos=False, repeat_penalty=1.0,
                                                repeat_last_n=64, presence_penalty=0.0, frequency_penalty=0.0))
    off = eng.generate(prompts, SamplingParams(max_new_tokens=12, stop_on_eos=False, repeat_penalty=1.5,
                                               presence_penalty=2.0, repeat_last_n=0))
    assert same == base and off == base
    assert all(not g.penalized for g in eng._graphs.values())     # the unpenalised flavour served both
    ce = ContinuousEngine(_engine(m))
    assert ce.generate(prompts, SamplingParams(max_new_tokens=12, stop_on_eos=False)) == base
    assert all(not g.penalized for g in ce._graphs.values())


def test_scheduler_penalised_matches_static_engine_and_moves_rings():
    """Requests join and leave (``_place`` / ``_compact`` move the rings), neutral ones mixed
    in: every request gets the tokens of running it alone."""
    m = _model()
    pen = dict(stop_on_eos=False, repeat_penalty=1.3, frequency_penalty=0.2, repeat_last_n=16)
    specs = [(0, 40, 6, True), (1, 33, 14, True), (2, 20, 3, False), (3, 50, 9, True), (4, 12, 11, False),
             (5, 28, 5, True)]
    ce = ContinuousEngine(_engine(m))
    futs, want = [], []
    for i, (seed, n, new, penalised) in enumerate(specs):
        sp = SamplingParams(max_new_tokens=new, **(pen if penalised else {"stop_on_eos": False}))
        p = _prompt(seed, n)
        want.append(_engine(m).generate([p], sp)[0])
        futs.append(ce.submit(p, sp))
        for _ in range(i % 3):
            ce.step()
    while ce.has_work():
        ce.step()
    assert [f.result() for f in futs] == want


def test_scheduler_stop_check_retires_early_and_frees_blocks():
    m = _model()
    eng = _engine(m)
    ce = ContinuousEngine(eng)
    free0 = eng.kv.allocator.num_free()
    p = _prompt(0)
    full = ce.generate([p], SamplingParams(max_new_tokens=12, stop_on_eos=False))[0]
    seen = []

    def check(out):
        seen.append(list(out))
        return len(out) >= 4

    f = ce.submit(p, SamplingParams(max_new_tokens=12, stop_on_eos=False), stop_check=check)
    g = ce.submit(_prompt(1), SamplingParams(max_new_tokens=12, stop_on_eos=False))
    while ce.has_work():
        ce.step()
    assert f.result() == full[:4] and len(g.result()) == 12
    assert seen == [full[:k] for k in range(1, 5)]
    assert eng.kv.allocator.num_free() == free0 and not ce.running

    def broken(out):
        raise RuntimeError("client bug")

    f = ce.submit(p, SamplingParams(max_new_tokens=12, stop_on_eos=False), stop_check=broken)
    while ce.has_work():
        ce.step()
    assert f.result() == full          # a check that raises is dropped, the request runs on
    assert eng.kv.allocator.num_free() == free0


# ------------------------------------------------------------------ tensor parallelism
TP_PROMPTS = [[1, 2, 3, 4, 5], list(range(7, 40)), [9] * 12 + [10, 11]]
TP_PARAMS = dict(max_new_tokens=8, stop_on_eos=False, repeat_penalty=1.3, frequency_penalty=0.2, repeat_last_n=16)


def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _tp_worker(rank, world, port, sd_path, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    torch.set_num_threads(1)
    from docqa_amd.parallel import comm

    comm.init_distributed(tp_size=world, backend="gloo")
    m = LlamaModel(LlamaConfig.preset("test-tp8"), device="cpu", dtype=torch.float32, init=False)
    m.load_state_dict_hf(torch.load(sd_path, weights_only=True))
    eng = LLMEngine(m, max_batch=4, max_context=256, block_size=16, use_graphs=False)
    out = eng.generate(TP_PROMPTS, SamplingParams(**TP_PARAMS))
    if rank == 0:
        torch.save(out, out_path)
    comm.destroy()


def test_tp2_penalised_greedy_matches_single_process(tmp_path):
    from docqa_amd.parallel import comm

    comm.destroy()
    one = LlamaModel(LlamaConfig.preset("test-tp8"), device="cpu", dtype=torch.float32, seed=5)
    sd_path = tmp_path / "sd.pt"
    torch.save(one.export_state_dict_hf(), sd_path)
    eng = LLMEngine(one, max_batch=4, max_context=256, block_size=16, use_graphs=False)
    expect = eng.generate(TP_PROMPTS, SamplingParams(**TP_PARAMS))
    plain = eng.generate(TP_PROMPTS, SamplingParams(max_new_tokens=8, stop_on_eos=False))
    assert expect != plain                     # the penalties change these decodes
    out = tmp_path / "out.pt"
    mp.start_processes(_tp_worker, args=(2, _free_port(), str(sd_path), str(out)), nprocs=2, join=True,
                       start_method="spawn")
    assert torch.load(out, weights_only=True) == expect


# ------------------------------------------------------------------ Ollama options / stop
def test_ollama_options_reach_sampling_params(monkeypatch):
    from docqa_amd.services.ollama_api import sampling_from_options

    for k in ("REPEAT_PENALTY", "REPEAT_LAST_N", "PRESENCE_PENALTY", "FREQUENCY_PENALTY"):
        monkeypatch.delenv(k, raising=False)
    st = Settings()
    assert (st.repeat_penalty, st.repeat_last_n, st.presence_penalty, st.frequency_penalty) == (1.0, 64, 0.0, 0.0)
    assert sampling_from_options(None, st, 1024, 100).neutral
    p = sampling_from_options({"repeat_penalty": 1.1, "repeat_last_n": 32, "presence_penalty": 0.5,
                               "frequency_penalty": 0.25}, st, 1024, 100)
    assert (p.repeat_penalty, p.repeat_last_n, p.presence_penalty, p.frequency_penalty) == (1.1, 32, 0.5, 0.25)
    assert sampling_from_options({"repeat_penalty": 1.1, "repeat_last_n": 0}, st, 1024, 100).neutral
    # the environment sets the service-wide defaults (Ollama's own: 1.1 over 64 tokens)
    monkeypatch.setenv("REPEAT_PENALTY", "1.1")
    monkeypatch.setenv("REPEAT_LAST_N", "48")
    monkeypatch.setenv("PRESENCE_PENALTY", "0.3")
    monkeypatch.setenv("FREQUENCY_PENALTY", "0.2")
    st = Settings()
    p = sampling_from_options({}, st, 1024, 100)
    assert (p.repeat_penalty, p.repeat_last_n, p.presence_penalty, p.frequency_penalty) == (1.1, 48, 0.3, 0.2)
    assert sampling_from_options({"repeat_penalty": 1.0, "presence_penalty": 0, "frequency_penalty": 0},
                                 st, 1024, 100).neutral


def test_stop_string_helpers():
    from docqa_amd.services.ollama_api import find_stop, held_back, stop_strings

    assert stop_strings(None) == [] and stop_strings({"stop": "a"}) == ["a"]
    assert stop_strings({"stop": ["x", "", "yz"]}) == ["x", "yz"]
    assert find_stop("hello END x", ["x", "END"]) == 6 and find_stop("abc", ["zz"]) == -1
    assert held_back("abc<|e", ["<|end|>", "xyz"]) == 3 and held_back("abc", ["<|end|>"]) == 0
    assert held_back("xa", ["ab"]) == 1 and held_back("ab", ["ab"]) == 0   # proper prefixes only
    assert held_back("", ["ab"]) == 0


def _stack(tmp_path, mode):
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = Settings()
    st.index_dir = str(tmp_path)
    st.default_data_dir = str(tmp_path / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 6
    st.serving_mode = mode
    return DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu",
                                   max_batch=4, max_context=1024, use_graphs=False), st)


def _post_generate(qa, options):
    return qa.post("/api/generate", json={"prompt": "Vide de Qi ?", "stream": False, "options": options}).json()


def _pieces(resp, key="response"):
    lines = [json.loads(x) for x in resp.text.splitlines() if x.strip()]
    assert lines[-1]["done"] is True and all(not x["done"] for x in lines[:-1])
    return [x[key] for x in lines[:-1]], lines[-1]


@pytest.mark.parametrize("mode", ["continuous", "batch"])
def test_ollama_stop_truncates_streaming_and_not(tmp_path, mode):
    from fastapi.testclient import TestClient

    s = _stack(tmp_path, mode)
    try:
        qa = TestClient(s.qa_app)
        N = 24
        req = {"prompt": "Vide de Qi ?", "stream": False, "options": {"num_predict": N, "temperature": 0}}
        full = qa.post("/api/generate", json=req).json()
        text = full["response"]
        assert full["done_reason"] == "length" and full["eval_count"] == N and len(text) >= 8, full
        # streamed without a stop string: the pieces the stop strings below are cut from
        pieces, _ = _pieces(qa.post("/api/generate", json={**req, "stream": True}))
        assert "".join(pieces) == text
        # (a) a stop string from the middle of the text
        k = len(text) // 2
        stop = text[k:k + 2]
        want = text[:text.find(stop)]
        opts = {**req["options"], "stop": [stop, "\x00never\x00"]}
        j = qa.post("/api/generate", json={**req, "options": opts}).json()
        assert j["response"] == want and stop not in j["response"] and j["done_reason"] == "stop"
        got, last = _pieces(qa.post("/api/generate", json={**req, "stream": True, "options": opts}))
        assert "".join(got) == want and last["done_reason"] == "stop"
        if mode == "continuous":
            # the scheduler retired the request at the token completing the stop string
            assert j["eval_count"] < N and last["eval_count"] == j["eval_count"]
            assert stop in s.pipeline.chat_tok.decode(
                s.pipeline.engine.generate([s.pipeline.chat_tok.chat_prompt("Vide de Qi ?")],
                                           SamplingParams(max_new_tokens=j["eval_count"], stop_on_eos=False))[0])
        else:
            assert j["eval_count"] == N           # no per-token hook: the text alone is cut
        # (b) a stop string split across two streamed pieces is never partly emitted
        if mode == "continuous":
            b = next(i for i in range(len(pieces) - 1) if pieces[i] and pieces[i + 1] and i >= 1)
            split = pieces[b][-1] + pieces[b + 1][0]
            want = text[:text.find(split)]
            got, last = _pieces(qa.post("/api/generate", json={**req, "stream": True,
                                                               "options": {**req["options"], "stop": split}}))
            assert "".join(got) == want and last["done_reason"] == "stop"
            assert not any(split in "".join(got[:i + 1]) for i in range(len(got)))
        # chat route, a plain string for ``stop``
        msgs = [{"role": "user", "content": "Vide de Qi ?"}]
        c = qa.post("/api/chat", json={"messages": msgs, "stream": False,
                                       "options": {"num_predict": N, "temperature": 0}}).json()
        ctext = c["message"]["content"]
        cstop = ctext[len(ctext) // 2:len(ctext) // 2 + 2]
        c2 = qa.post("/api/chat", json={"messages": msgs, "stream": False,
                                        "options": {"num_predict": N, "temperature": 0, "stop": cstop}}).json()
        assert c2["message"]["content"] == ctext[:ctext.find(cstop)] and c2["done_reason"] == "stop"
    finally:
        s.close()


def test_ollama_penalty_options_change_the_decode(tmp_path):
    """The options reach the engine: a presence penalty that forbids every repeat changes a
    greedy decode that repeats, and the route returns the engine's tokens for those params."""
    from fastapi.testclient import TestClient

    s = _stack(tmp_path, "continuous")
    try:
        qa = TestClient(s.qa_app)
        opts = {"num_predict": 48, "temperature": 0}
        a = _post_generate(qa, opts)
        b = _post_generate(qa, {**opts, "presence_penalty": 1e4, "repeat_last_n": -1})
        assert a["eval_count"] == b["eval_count"] == 48
        ids = s.pipeline.chat_tok.chat_prompt("Vide de Qi ?")
        sp = SamplingParams(max_new_tokens=48, presence_penalty=1e4, repeat_last_n=-1)
        out = s.pipeline.engine.generate([ids], sp)[0]
        assert len(set(out)) == len(out) and not set(out) & set(ids)       # nothing repeats
        assert b["response"] == s.pipeline.chat_tok.decode(out)
        assert a["response"] != b["response"]
    finally:
        s.close()


def test_env_penalty_defaults_serve_ask_and_ollama_routes(tmp_path, monkeypatch):
    """PRESENCE_PENALTY / REPEAT_LAST_N from the environment are the defaults of /ask/ (the
    batcher's params) and of Ollama requests that send no such option; an option overrides."""
    from fastapi.testclient import TestClient

    opts = {"num_predict": 48, "temperature": 0}
    plain = _stack(tmp_path / "a", "continuous")
    try:
        want_plain = _post_generate(TestClient(plain.qa_app), opts)["response"]
        want_pen = _post_generate(TestClient(plain.qa_app), {**opts, "presence_penalty": 1e4,
                                                             "repeat_last_n": -1})["response"]
    finally:
        plain.close()
    assert want_plain != want_pen
    monkeypatch.setenv("PRESENCE_PENALTY", "1e4")
    monkeypatch.setenv("REPEAT_LAST_N", "-1")
    s = _stack(tmp_path / "b", "continuous")
    try:
        qa = TestClient(s.qa_app)
        p = s.qa_app.state.batcher._params()           # what /ask/ and /api/llm/summarize decode with
        assert (p.presence_penalty, p.repeat_last_n, p.repeat_penalty, p.frequency_penalty) == (1e4, -1, 1.0, 0.0)
        assert not p.neutral
        assert _post_generate(qa, opts)["response"] == want_pen
        assert _post_generate(qa, {**opts, "presence_penalty": 0})["response"] == want_plain
        r = qa.post("/ask/", json={"question": "Quelle plante pour un Vide de Qi ?"})
        assert r.status_code == 200 and isinstance(r.json()["answer"], str)
    finally:
        s.close()
