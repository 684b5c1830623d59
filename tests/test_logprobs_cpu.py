"""Per-token log-probabilities without a GPU: the fp32 reference op against a float64 oracle, the
engine and the continuous scheduler on the ``tiny`` preset, the Ollama routes in both serving
modes, and the vocab-parallel path on two gloo ranks."""
import json
import math
import os

import pytest
import torch
import torch.multiprocessing as mp

from docqa_amd import ops
from docqa_amd.config import Settings
from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
from docqa_amd.engine.scheduler import ContinuousEngine
from docqa_amd.models.llama import LlamaConfig, LlamaModel
from tests.test_logprobs_gpu import TOL, T, check

SENT = (777.0, -7, 555.0)


def _case(R, n_valid, ld, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.full((R, ld), 100.0)                                # padding beats every valid logit
    x[:, :n_valid] = (torch.randn(R, n_valid, generator=g) * 8).clamp(-64, 64)
    x = x.to(dtype)
    chosen = torch.randint(0, n_valid, (R,), generator=g)
    chosen[0] = int(x[0, :n_valid].float().argmin())              # a token outside the top 20
    return x, chosen, torch.tensor([[20, 0, -1, 1][r % 4] for r in range(R)], dtype=torch.int32)


def _run(x, n_valid, chosen, top_n):
    R = x.shape[0]
    lp = torch.full((R,), SENT[0])
    ti = torch.full((R, T), SENT[1], dtype=torch.int32)
    tl = torch.full((R, T), SENT[2])
    out = ops.token_logprobs(x, n_valid, chosen, top_n, lp, ti, tl)
    assert out[0] is lp and out[1] is ti and out[2] is tl
    check(x, n_valid, chosen, top_n, lp, ti, tl, SENT)
    return lp, ti, tl


# ----------------------------------------------------------------------------- the reference op
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("R", [1, 3, 33])
@pytest.mark.parametrize("n_valid,pad", [(8, 0), (8, 96), (4000, 0), (4000, 96), (4096, 0), (4096, 96), (2056, 0)])
def test_reference_matches_the_float64_oracle(dtype, R, n_valid, pad):
    _run(*(lambda x, c, n: (x, n_valid, c, n))(*_case(R, n_valid, n_valid + pad, dtype, R * 10007 + n_valid + pad)))


def test_reference_ties_winners_shift_and_magnitude():
    V = 4096
    x, chosen, top_n = _case(3, V, V, torch.float32, 3)
    top_n[:] = 20
    ties = [1024 * k + d for k in (1, 2, 3) for d in (-1, 0)]
    x[0, ties] = 70.0
    x[1, 5], x[1, V - 3] = 71.0, 70.5
    x[2] = -60.0
    lp, ti, _ = _run(x, V, chosen, top_n)
    assert ti[0, :6].tolist() == sorted(ties) and ti[1, :2].tolist() == [5, V - 3]
    assert ti[2].tolist() == list(range(T)) and abs(float(lp[2]) + math.log(V)) <= TOL
    # +-3e4: the sum overflows unless the maximum is subtracted
    g = torch.Generator().manual_seed(11)
    sign = torch.where(torch.rand(3, 4000, generator=g) < 0.5, -1.0, 1.0)
    x = (sign * 3e4 + torch.randn(3, 4000, generator=g) * 8).float()
    chosen = torch.stack([torch.nonzero(x[r] > x[r].max() - 30)[3, 0] for r in range(3)])
    _run(x, 4000, chosen, top_n)
    # fresh outputs: a skipped row keeps the empty entries
    lp, ti, tl = ops.token_logprobs(x, 4000, chosen, torch.tensor([-1, 0, 2], dtype=torch.int32))
    assert float(lp[0]) == 0.0 and (ti[:2] == -1).all() and (tl[:2] == -math.inf).all() and (ti[2, :2] >= 0).all()
    assert ops.TOP_LOGPROBS_MAX == 20


# ----------------------------------------------------------------------------- SamplingParams
def test_sampling_params():
    sp = SamplingParams()
    assert sp.logprobs is False and sp.top_logprobs == 0 and sp.fused_greedy_ok and sp.neutral and sp.lp_n == -1
    lp = SamplingParams(logprobs=True, top_logprobs=5)
    assert not lp.fused_greedy_ok and lp.neutral and lp.lp_n == 5
    assert SamplingParams(logprobs=True).lp_n == 0
    assert SamplingParams(logprobs=True, top_logprobs=99).top_logprobs == 20
    assert SamplingParams(logprobs=True, top_logprobs=-3).top_logprobs == 0
    assert not SamplingParams(logprobs=True, repeat_penalty=1.2).neutral


# ----------------------------------------------------------------------------- LLMEngine
def _tiny(seed=4):
    torch.manual_seed(0)
    return LlamaModel(LlamaConfig.preset("tiny"), device="cpu", dtype=torch.float32, seed=seed)


def _prompts(lens=(20, 35, 9, 50), seed=2):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, 4000, (int(n),), generator=g).tolist() for n in lens]


def _spy(monkeypatch):
    calls = []
    orig = ops.token_logprobs

    def token_logprobs(logits, n_valid, chosen, top_n, *a, **k):
        rec = [logits.clone(), n_valid, chosen.clone(), top_n.clone()]
        out = orig(logits, n_valid, chosen, top_n, *a, **k)
        calls.append(rec + [o.clone() for o in out])
        return out

    monkeypatch.setattr(ops, "token_logprobs", token_logprobs)
    return calls


def _engine(m, **kw):
    return LLMEngine(m, max_batch=8, max_context=256, block_size=16, use_graphs=False, prefix_cache=False, **kw)


def test_engine_every_token_has_its_logprob(monkeypatch):
    m = _tiny()
    prompts = _prompts()
    N = 6
    plain = _engine(m).generate(prompts, SamplingParams(max_new_tokens=N, stop_on_eos=False))
    calls = _spy(monkeypatch)
    eng = _engine(m)
    sp = SamplingParams(max_new_tokens=N, stop_on_eos=False, logprobs=True, top_logprobs=3)
    h = eng.launch(prompts, sp)
    lps = eng.collect_logprobs(h)
    toks = eng.collect(h)
    assert toks == plain                             # the argmax of the logits is the fused pick
    assert len(calls) == N                           # the prefill's first token + N - 1 steps
    for step, (logits, n_valid, chosen, top_n, lp, ti, tl) in enumerate(calls):
        assert n_valid == m.cfg.vocab_size and top_n.tolist() == [3] * 4
        assert chosen.tolist() == [t[step] for t in toks]
        check(logits, n_valid, chosen, top_n, lp, ti, tl)
        for b in range(4):                           # what the caller gets is what the op wrote
            assert lps[b][step] == (float(lp[b]), [(int(i), float(v)) for i, v in zip(ti[b, :3], tl[b, :3])])
            assert lps[b][step][1][0] == (toks[b][step], lps[b][step][0])     # greedy neutral: entry 0
    assert h.lp.shape == (4, N) and h.lp_top_ids.shape == (4, N, T) and h.lp_top.shape == (4, N, T)
    # cut at EOS like the tokens
    m.cfg.eos_token_id = toks[0][2]
    try:
        h = eng.launch(prompts, SamplingParams(max_new_tokens=N, logprobs=True, top_logprobs=3))
        cut_l, cut_t = eng.collect_logprobs(h), eng.collect(h)
    finally:
        m.cfg.eos_token_id = LlamaConfig.preset("tiny").eos_token_id
    assert len(cut_t[0]) == toks[0].index(toks[0][2]) + 1 < N
    assert [len(r) for r in cut_l] == [len(r) for r in cut_t] and cut_l[0] == lps[0][:len(cut_t[0])]


def test_engine_without_logprobs_never_calls_the_op(monkeypatch):
    m = _tiny()
    prompts = _prompts()
    sp = SamplingParams(max_new_tokens=5, stop_on_eos=False)
    calls = _spy(monkeypatch)
    eng = _engine(m)
    h = eng.launch(prompts, sp)
    assert eng.collect_logprobs(h) is None and h.lp is None
    a = eng.collect(h)
    assert not calls

    def boom(*a, **k):
        raise AssertionError("token_logprobs called for a request without logprobs")

    monkeypatch.setattr(ops, "token_logprobs", boom)
    assert _engine(m).generate(prompts, sp) == a
    ce = ContinuousEngine(_engine(m))
    assert ce.generate(prompts, sp) == a and not any(k[5] for k in ce._graphs)


@pytest.mark.parametrize("extra", [{"repeat_penalty": 1.5, "presence_penalty": 0.5}, {"temperature": 0.7, "seed": 9}],
                         ids=["penalised", "sampled"])
def test_engine_logprobs_are_those_of_the_raw_logits(monkeypatch, extra):
    """The values describe the model's distribution: the op gets the LM head's logits unchanged,
    before the penalties / temperature and the pick."""
    m = _tiny()
    heads = []
    lm = ops.lm_head_logits
    monkeypatch.setattr(ops, "lm_head_logits", lambda x, w: (heads.append(lm(x, w)), heads[-1].clone())[1])
    calls = _spy(monkeypatch)
    sp = SamplingParams(max_new_tokens=5, stop_on_eos=False, logprobs=True, top_logprobs=2, **extra)
    toks, lps = _engine(m).generate_with_logprobs(_prompts((33, 9), 8), sp)
    assert len(calls) == len(heads) == 5
    for (logits, n_valid, chosen, top_n, lp, ti, tl), head in zip(calls, heads):
        assert torch.equal(logits, head[:, :n_valid])
        check(head, n_valid, chosen, top_n, lp, ti, tl)
    assert [len(r) for r in lps] == [5, 5]


# ----------------------------------------------------------------------------- ContinuousEngine
def _close(a, b):
    """Two (logprob, top list) lists agree: the same ids, values within the kernel tests' bound
    (a request alone and inside a batch runs differently shaped fp32 matmuls)."""
    assert len(a) == len(b)
    for (x, tx), (y, ty) in zip(a, b):
        assert abs(x - y) <= TOL and [i for i, _ in tx] == [i for i, _ in ty]
        assert all(abs(u[1] - v[1]) <= TOL for u, v in zip(tx, ty))


def _serve(ce, pairs, stagger=False):
    futs = []
    for i, (p, s) in enumerate(pairs):
        futs.append(ce.submit(p, s))
        for _ in range(i % 3 if stagger else 0):
            ce.step()
    while ce.has_work():
        ce.step()
    return futs


@pytest.mark.parametrize("lag", [False, True], ids=["direct", "lagged"])
def test_scheduler_mixed_batch(lag):
    m = _tiny()
    prompts = _prompts()
    base = dict(max_new_tokens=7, stop_on_eos=False)
    sps = [SamplingParams(logprobs=True, top_logprobs=3, **base), SamplingParams(**base),
           SamplingParams(logprobs=True, **base), SamplingParams(**base)]
    ce = ContinuousEngine(_engine(m))
    ce.lag_cpu = lag
    streamed = {}
    futs = []
    for i, (p, s) in enumerate(zip(prompts, sps)):
        futs.append(ce.submit(p, s, on_token=lambda rid, t, lp="none", i=i: streamed.setdefault(i, []).append((t, lp))))
        ce.step()
    while ce.has_work():
        ce.step()
    assert any(k[5] for k in ce._graphs)
    for i, (f, p, s) in enumerate(zip(futs, prompts, sps)):
        out, lps = f.result(), f.request.logprobs
        assert len(out) == 7 and [t for t, _ in streamed[i]] == out
        if not s.logprobs:
            assert lps == [] and all(lp == "none" for _, lp in streamed[i])     # rows that did not ask get nothing
            continue
        assert len(lps) == len(out) and [len(top) for _, top in lps] == [s.top_logprobs] * 7
        assert [lp for _, lp in streamed[i]] == lps
        if s.top_logprobs:
            assert all(top[0] == (t, lp) for t, (lp, top) in zip(out, lps))
        alone, = _serve(ContinuousEngine(_engine(m)), [(p, s)])
        assert alone.result() == out
        _close(lps, alone.request.logprobs)
        toks, static = _engine(m).generate_with_logprobs([p], s)
        assert toks[0] == out
        _close(lps, static[0])


def test_scheduler_preemption_keeps_the_lists_parallel():
    """The small pool of test_scheduler_cpu: requests are preempted and recomputed; the logprobs
    of the tokens they keep stay, and the lists still line up with the tokens."""
    m = _tiny()
    prompts = _prompts((20, 35, 9, 50, 28, 17))
    sps = [SamplingParams(max_new_tokens=40, stop_on_eos=False, logprobs=i % 2 == 1, top_logprobs=2 * (i % 4 == 1))
           for i in range(6)]
    roomy = LLMEngine(m, max_batch=8, max_context=256, block_size=16, use_graphs=False, prefix_cache=False)
    expect = [roomy.generate_with_logprobs([p], s) if s.logprobs else (roomy.generate([p], s), None)
              for p, s in zip(prompts, sps)]
    small = LLMEngine(m, max_batch=8, max_context=256, block_size=16, num_blocks=14, use_graphs=False,
                      prefix_cache=False)
    ce = ContinuousEngine(small, max_running=8)
    free0 = small.kv.allocator.num_free()
    futs = _serve(ce, list(zip(prompts, sps)))
    assert ce.preempted > 0 and small.kv.allocator.num_free() == free0
    assert any(f.request.preemptions and f.request.params.logprobs for f in futs)
    for f, s, (toks, lps) in zip(futs, sps, expect):
        assert f.result() == toks[0]
        if s.logprobs:
            assert len(f.request.logprobs) == len(f.result()) == 40
            _close(f.request.logprobs, lps[0])
        else:
            assert f.request.logprobs == []


# ----------------------------------------------------------------------------- the Ollama routes
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


def _lines(resp):
    lines = [json.loads(x) for x in resp.text.splitlines() if x.strip()]
    assert lines[-1]["done"] is True and all(not x["done"] for x in lines[:-1])
    return lines


def _entries_ok(entries, top):
    for e in entries:
        assert set(e) == {"token", "logprob", "bytes", "top_logprobs"}
        assert bytes(e["bytes"]).decode("utf-8") == e["token"] and e["logprob"] <= 0.0
        assert len(e["top_logprobs"]) == top
        for t in e["top_logprobs"]:
            assert set(t) == {"token", "logprob", "bytes"} and bytes(t["bytes"]).decode("utf-8") == t["token"]
        vals = [t["logprob"] for t in e["top_logprobs"]]
        assert vals == sorted(vals, reverse=True)
        if top:                                       # greedy: the token is the most likely one
            assert e["top_logprobs"][0]["logprob"] == e["logprob"] and e["top_logprobs"][0]["token"] == e["token"]


@pytest.mark.parametrize("mode", ["continuous", "batch"])
def test_ollama_routes_return_logprobs(tmp_path, mode):
    from fastapi.testclient import TestClient

    s = _stack(tmp_path, mode)
    try:
        qa = TestClient(s.qa_app)
        N = 24
        routes = [("/api/generate", {"prompt": "Vide de Qi ?"}, lambda j: j["response"]),
                  ("/api/chat", {"messages": [{"role": "user", "content": "Vide de Qi ?"}]},
                   lambda j: j["message"]["content"])]
        for path, body, text_of in routes:
            req = {**body, "stream": False, "options": {"num_predict": N, "temperature": 0}}
            plain = qa.post(path, json=req).json()
            assert "logprobs" not in plain and plain["eval_count"] == N
            lp = {"logprobs": True, "top_logprobs": 2}
            j = qa.post(path, json={**req, **lp}).json()
            assert text_of(j) == text_of(plain) and j["eval_count"] == N
            assert len(j["logprobs"]) == j["eval_count"]
            _entries_ok(j["logprobs"], 2)
            if path == "/api/generate":               # "token" is the tokenizer's decoding of that single id
                tok = s.pipeline.chat_tok
                out = s.pipeline.engine.generate([tok.chat_prompt("Vide de Qi ?")],
                                                 SamplingParams(max_new_tokens=N, stop_on_eos=False))[0]
                assert [e["token"] for e in j["logprobs"]] == [tok.decode([t]) for t in out]
            # logprobs without alternatives: "top_logprobs" present and empty
            j0 = qa.post(path, json={**req, "logprobs": True}).json()
            _entries_ok(j0["logprobs"], 0)
            assert [e["logprob"] for e in j0["logprobs"]] == pytest.approx([e["logprob"] for e in j["logprobs"]],
                                                                           abs=TOL)
            # streamed: the entries of all lines are the non-streamed list
            lines = _lines(qa.post(path, json={**req, **lp, "stream": True}))
            assert "".join(text_of(x) for x in lines) == text_of(j)
            assert all("logprobs" in x for x in lines)
            assert [e for x in lines for e in x["logprobs"]] == j["logprobs"]
            plain_lines = _lines(qa.post(path, json={**req, "stream": True}))
            assert not any("logprobs" in x for x in plain_lines)
            if mode == "continuous":
                assert len(lines) > 2 and sum(bool(x["logprobs"]) for x in lines) > 1     # token by token
            # a stop string: the tokens it cuts off are dropped from the list like their text
            text = text_of(plain)
            k = len(text) // 2
            stop = text[k:k + 2]
            opts = {**req["options"], "stop": [stop]}
            js = qa.post(path, json={**req, **lp, "options": opts}).json()
            assert text_of(js) == text[:text.find(stop)] and js["done_reason"] == "stop"
            assert 0 < len(js["logprobs"]) < N and js["logprobs"] == j["logprobs"][:len(js["logprobs"])]
            ls = _lines(qa.post(path, json={**req, **lp, "stream": True, "options": opts}))
            assert "".join(text_of(x) for x in ls) == text_of(js)
            assert [e for x in ls for e in x["logprobs"]] == js["logprobs"]
        # refusals
        for bad in ({"logprobs": True, "top_logprobs": 21}, {"logprobs": True, "top_logprobs": -1},
                    {"top_logprobs": 3}, {"logprobs": False, "top_logprobs": 1}):
            for path, body, _ in routes:
                r = qa.post(path, json={**body, "stream": False, **bad})
                assert r.status_code == 400 and "error" in r.json(), (path, bad)
    finally:
        s.close()


# ----------------------------------------------------------------------------- TP = 2 (gloo)
def _tp_worker(rank, world, port, sd_path, out_path):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port)})
    torch.set_num_threads(1)
    from docqa_amd.parallel import comm

    comm.init_distributed(tp_size=world, backend="gloo")
    m = LlamaModel(LlamaConfig.preset("test-tp8"), device="cpu", dtype=torch.float32, init=False)
    m.load_state_dict_hf(torch.load(sd_path, weights_only=True))
    assert m.lm_head.shape[0] < m.cfg.vocab_size      # a vocab shard: the op needs the gathered logits
    eng = LLMEngine(m, max_batch=4, max_context=256, block_size=16, use_graphs=False)
    out = eng.generate_with_logprobs(_TP_PROMPTS, _TP_PARAMS)
    if rank == 0:
        torch.save(out, out_path)
    comm.destroy()


_TP_PROMPTS = [[1, 2, 3, 4, 5], list(range(7, 40))]
_TP_PARAMS = SamplingParams(max_new_tokens=4, stop_on_eos=False, logprobs=True, top_logprobs=3)


def test_tp2_gathers_the_vocabulary_before_the_op(tmp_path):
    """At TP > 1 the logprobs come from ``full_logits``: two gloo ranks give the single-process
    tokens and logprobs."""
    from docqa_amd.parallel import comm
    from tests.test_tp_worlds_cpu import _free_port

    comm.destroy()
    ref = LlamaModel(LlamaConfig.preset("test-tp8"), device="cpu", dtype=torch.float32, seed=5)
    sd_path = tmp_path / "sd.pt"
    torch.save(ref.export_state_dict_hf(), sd_path)
    eng = LLMEngine(ref, max_batch=4, max_context=256, block_size=16, use_graphs=False)
    toks, lps = eng.generate_with_logprobs(_TP_PROMPTS, _TP_PARAMS)
    out = tmp_path / "out.pt"
    mp.start_processes(_tp_worker, args=(2, _free_port(), str(sd_path), str(out)), nprocs=2, join=True,
                       start_method="spawn")
    got_t, got_l = torch.load(out, weights_only=False)
    assert got_t == toks
    for a, b in zip(got_l, lps):
        _close(a, b)
