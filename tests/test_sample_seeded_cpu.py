"""Seeded per-request sampling and ``min_p``, CPU side: Philox4x32-10 known answers and the
``seeded_uniform`` mapping, the reference ``sample_tokens`` against the fp64 oracle
(tests/sample_seeded_oracle.py), the continuous scheduler's invariance of a seeded request to its
neighbours, its slot and a preemption, the static engine's ``min_p`` path against a Python loop,
the Ollama option, the service's reproducibility and two lockstep ranks on one unseeded request."""
import os
import socket
import time

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from docqa_amd import ops
from docqa_amd.config import Settings
from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
from docqa_amd.engine.scheduler import ContinuousEngine
from docqa_amd.models.llama import LlamaConfig, LlamaModel
from docqa_amd.ops import reference as ref
from tests.sample_oracle import CASES, DELTA, check, make_row, uniforms
from tests.sample_seeded_oracle import INDICES, SEEDS, build_case_min_p

MIN_PS = (0.0, ("m*", 0.05), ("m*", 0.5), 1.0)


# ------------------------------------------------------------------ Philox / seeded_uniform
def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    assert ref.philox4x32((0, 0, 0, 0), (0, 0)) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert ref.philox4x32((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)


def test_seeded_uniform_mapping():
    grid = [(s, i) for s in SEEDS for i in INDICES]
    seed = torch.tensor([s for s, _ in grid], dtype=torch.int64)
    index = torch.tensor([i for _, i in grid], dtype=torch.int32)
    u = ops.seeded_uniform(seed, index)
    assert u.dtype == torch.float32 and u.shape == (len(grid),)
    for (s, i), got in zip(grid, u.tolist()):
        w0 = ref.philox4x32((i, 0, 0, 0), (s & 0xffffffff, s >> 32))[0]
        assert got == (w0 >> 8) / 2.0 ** 24          # exact: 24 bits in an fp32
        assert 0.0 <= got < 1.0
    assert len(set(u.tolist())) == len(grid)
    # the largest value the mapping can give is below 1 in fp32
    assert float(np.float32((0xffffffff >> 8) * 2.0 ** -24)) == 1.0 - 2.0 ** -24 < 1.0


# ------------------------------------------------------------------ reference op vs the oracle
def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


@pytest.mark.parametrize("form", ["u", "seed"])
@pytest.mark.parametrize("V", (16, 255, 257, 1000))
def test_reference_sample_tokens_matches_oracle(V, form):
    n = 64
    worst = 0.0
    for ci, case in enumerate(CASES):
        row = make_row(V, seed=100 * ci + V)
        for mi, mp_ in enumerate(MIN_PS):
            (it, k, p, m), keep, cdf, _ = build_case_min_p(row, case, mp_)
            logits = _t(row, torch.float32).expand(n, -1).contiguous()
            par = (torch.full((n,), it), torch.full((n,), k, dtype=torch.int32), torch.full((n,), p),
                   torch.full((n,), m))
            if form == "u":
                u = uniforms(n, seed=ci)
                tok = ops.sample_tokens(logits, V, *par, u=_t(u, torch.float32))
            else:
                seed = torch.arange(n, dtype=torch.int64) * 7919 + (1 << 40) + mi
                index = torch.arange(n, dtype=torch.int32) * 3 + ci
                u = ref.seeded_uniform(seed, index).numpy()
                tok = ops.sample_tokens(logits, V, *par, seed=seed, index=index)
            worst = max(worst, check(tok.numpy(), u, keep, cdf))
    print(f"overshoot {worst:.3e} of delta {DELTA:g}: V={V} form={form}")


def test_reference_sample_tokens_columns_valid_and_argmax():
    """Columns at or past n_valid take no part, valid == 0 rows get token 0, top_k == 1 is the
    lowest index of the maximum, min_p == 1 keeps exactly the copies of the maximum."""
    V = 257
    row = make_row(V, seed=5)
    wide = np.concatenate([row, np.full(7, 1e30, dtype=np.float32)])
    (it, k, p, m), keep, cdf, _ = build_case_min_p(row, (1.25, 40, "p*"), ("m*", 0.05))
    n = 32
    u = uniforms(n, seed=3)
    par = (torch.full((n,), it), torch.full((n,), k, dtype=torch.int32), torch.full((n,), p), torch.full((n,), m))
    valid = torch.ones(n, dtype=torch.int32)
    valid[5] = 0
    tok = ops.sample_tokens(_t(wide, torch.float32).expand(n, -1), V, *par, u=_t(u, torch.float32), valid=valid)
    assert tok[5] == 0
    sel = np.arange(n) != 5
    check(tok.numpy()[sel], u[sel], keep, cdf)
    tied = row.copy()
    tied[[30, 200]] = tied.max() + 1.0
    one = torch.ones(2)
    tok = ops.sample_tokens(_t(tied, torch.float32).expand(2, -1), V, one, torch.tensor([1, 0], dtype=torch.int32), one,
                            torch.tensor([0.0, 1.0]), u=torch.tensor([0.9, 0.9]))
    assert tok.tolist() == [30, 200]           # argmax: the lowest copy; min_p 1 at u 0.9: the second copy
    with pytest.raises(ValueError):
        ops.sample_tokens(_t(row, torch.float32)[None], V, one[:1], torch.zeros(1, dtype=torch.int32), one[:1], None)


# ------------------------------------------------------------------ scheduler
def _model(seed=7):
    cfg = LlamaConfig(name="tiny-gqa4", vocab_size=4096, hidden=256, intermediate=512, layers=2,
                      heads=8, kv_heads=2, head_dim=128, max_position=2048, bos_token_id=1, eos_token_id=2)
    return LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=seed)


def _prompts(lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, 4096, (int(n),), generator=g).tolist() for n in lens]


def _engine(m, **kw):
    return LLMEngine(m, max_batch=8, max_context=256, block_size=16, use_graphs=False, prefix_cache=False, **kw)


def _invariance(a: SamplingParams):
    """Request ``a`` (on prompt 0) served alone, among five staggered sampled and greedy requests,
    and last into a KV pool too small for all of them (so it is the one preempted)."""
    m = _model()
    pa, *others = _prompts((28, 20, 35, 9, 50, 17))
    op = [SamplingParams(max_new_tokens=n, stop_on_eos=False, temperature=t, top_k=20, seed=s)
          for n, t, s in ((30, 0.9, 5), (40, 0.0, 0), (25, 1.1, 0), (40, 0.0, 0), (35, 0.7, 99))]
    torch.manual_seed(1)
    alone = ContinuousEngine(_engine(m)).generate([pa], a)[0]
    assert len(alone) == a.max_new_tokens
    # among the others, arriving while they decode; the global generator is elsewhere by now
    torch.manual_seed(2)
    ce = ContinuousEngine(_engine(m))
    futs = []
    for i, (p, sp) in enumerate(zip(others[:3], op[:3])):
        futs.append(ce.submit(p, sp))
        for _ in range(i + 1):
            ce.step()
    fa = ce.submit(pa, a)
    for p, sp in zip(others[3:], op[3:]):
        ce.step()
        futs.append(ce.submit(p, sp))
    while ce.has_work():
        ce.step()
    assert fa.result() == alone
    assert fa.request.seed == a.seed
    assert all(len(f.result()) == sp.max_new_tokens for f, sp in zip(futs, op))
    # full reservations need sum(ceil((len + new) / 16)) = 27 blocks; with 20 every request is
    # admitted and the pool runs out while all six decode (lengths are fixed: no EOS stop)
    small = _engine(m, num_blocks=20)
    ce = ContinuousEngine(small, max_running=8)
    futs = [ce.submit(p, sp) for p, sp in zip(others, op)]
    fa = ce.submit(pa, a)                      # the latest arrival: the first to be preempted
    while ce.has_work():
        ce.step()
    assert ce.preempted > 0 and fa.request.preemptions > 0
    assert fa.result() == alone
    return m, pa, alone


def test_scheduler_seeded_request_is_invariant():
    _invariance(SamplingParams(max_new_tokens=40, stop_on_eos=False, seed=1234, temperature=0.8, top_k=40))


def test_scheduler_seeded_min_p_request_and_seeds():
    b = SamplingParams(max_new_tokens=40, stop_on_eos=False, seed=1234, temperature=0.8, top_k=40, min_p=0.05)
    m, pb, alone = _invariance(b)
    # min_p reaches the slots: at 1.0 only the maximum is kept, so the sampled request is greedy
    top = SamplingParams(max_new_tokens=40, stop_on_eos=False, seed=1234, temperature=0.8, top_k=40, min_p=1.0)
    greedy = ContinuousEngine(_engine(m)).generate([pb], SamplingParams(max_new_tokens=40, stop_on_eos=False))[0]
    assert ContinuousEngine(_engine(m)).generate([pb], top)[0] == greedy != alone
    # one batch: same prompt and seed -> equal tokens; another seed -> others
    other = SamplingParams(max_new_tokens=40, stop_on_eos=False, seed=4321, temperature=0.8, top_k=40, min_p=0.05)
    ce = ContinuousEngine(_engine(m))
    f1, f2, f3 = ce.submit(pb, b), ce.submit(pb, b), ce.submit(pb, other)
    while ce.has_work():
        ce.step()
    assert f1.result() == f2.result() == alone
    assert f3.result() != alone
    # unseeded copies: each request draws a seed of its own, the shared params stay untouched
    un = SamplingParams(max_new_tokens=8, stop_on_eos=False, temperature=0.8, top_k=40, min_p=0.05)
    ce = ContinuousEngine(_engine(m))
    g1, g2 = ce.submit(pb, un), ce.submit(pb, un)
    while ce.has_work():
        ce.step()
    s1, s2 = g1.request.seed, g2.request.seed
    assert s1 != 0 and s2 != 0 and s1 != s2 and 0 < s1 < 2 ** 63 and 0 < s2 < 2 ** 63
    assert un.seed == 0
    assert len(g1.result()) == len(g2.result()) == 8


# ------------------------------------------------------------------ static engine
def _last_logits(eng, seq):
    r = eng.reserve([seq], SamplingParams(max_new_tokens=1))
    try:
        with torch.inference_mode():
            return eng.model.full_logits(eng._prefill([seq], r.tables, r.cached))[0].float().clone()
    finally:
        eng.release(r)


def test_static_engine_min_p_equals_python_loop():
    m = LlamaModel(LlamaConfig.preset("tiny"), device="cpu", dtype=torch.float32, seed=3)
    sp = SamplingParams(max_new_tokens=16, stop_on_eos=False, temperature=0.8, top_k=50, top_p=0.95, min_p=0.3, seed=11)
    prompt = _prompts((40,), seed=2)[0]

    def eng():
        return LLMEngine(m, max_batch=4, max_context=512, block_size=16, use_graphs=False, prefix_cache=False)

    e1 = eng()
    got = e1.generate([prompt], sp)[0]
    assert e1._graphs_min_p and not e1._graphs            # the flavour whose pick is ops.sample_tokens
    e, seq, out = eng(), list(prompt), []
    torch.manual_seed(sp.seed)
    for _ in range(sp.max_new_tokens):
        x = _last_logits(e, seq)
        t = int(ref.sample_tokens(x[None], x.numel(), torch.tensor([1.0 / sp.temperature]),
                                  torch.tensor([sp.top_k], dtype=torch.int32), torch.tensor([sp.top_p]),
                                  torch.tensor([sp.min_p]), u=torch.rand(1))[0])
        seq.append(t)
        out.append(t)
    assert got == out
    # without min_p the static path is the one it was (ops.sample on the batch-level stream)
    sp0 = SamplingParams(max_new_tokens=16, stop_on_eos=False, temperature=0.8, top_k=50, top_p=0.95, seed=11)
    e0 = eng()
    e0.generate([prompt], sp0)
    assert e0._graphs and not e0._graphs_min_p


# ------------------------------------------------------------------ API
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


def test_min_p_option(tmp_path):
    from fastapi.testclient import TestClient

    from docqa_amd.services.ollama_api import sampling_from_options

    st = Settings()
    assert sampling_from_options({"min_p": 0.05}, st, 1024, 100).min_p == 0.05
    assert sampling_from_options(None, st, 1024, 100).min_p == 0.0
    with pytest.raises(ValueError):
        sampling_from_options({"min_p": -0.1}, st, 1024, 100)
    s = _stack(tmp_path)
    try:
        qa = TestClient(s.qa_app)
        bad = qa.post("/api/generate", json={"prompt": "abc", "stream": False, "options": {"min_p": 1.5}})
        assert bad.status_code == 400 and "min_p" in bad.json()["error"]
        ok = qa.post("/api/generate", json={"prompt": "abc", "stream": False,
                                            "options": {"min_p": 0.05, "temperature": 0.8, "num_predict": 4}})
        assert ok.status_code == 200 and ok.json()["eval_count"] >= 1
    finally:
        s.close()


def test_service_reproducibility(tmp_path):
    """The same seeded /api/generate request twice, the second time with another sampled request
    decoding next to it: the same response."""
    from fastapi.testclient import TestClient

    s = _stack(tmp_path)
    try:
        qa = TestClient(s.qa_app)
        body = {"prompt": "Vide de Qi de la Rate ?", "stream": False,
                "options": {"seed": 7, "temperature": 0.8, "num_predict": 12}}
        first = qa.post("/api/generate", json=body)
        assert first.status_code == 200 and first.json()["eval_count"] >= 1
        batcher = s.qa_app.state.batcher
        other = batcher.submit("gen", {"ids": _prompts((30,), seed=9)[0],
                                       "params": SamplingParams(max_new_tokens=400, stop_on_eos=False,
                                                                temperature=0.9, top_k=20)})
        while not batcher.engine.running:
            assert not other.done()
            time.sleep(0.002)
        second = qa.post("/api/generate", json=body)
        assert not other.done()                # it was in flight all along
        assert second.status_code == 200
        assert second.json()["response"] == first.json()["response"]
        assert len(other.result(timeout=300)["ids"]) == 400
    finally:
        s.close()


# ------------------------------------------------------------------ lockstep
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _lockstep_worker(rank, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=2)
    from docqa_amd.engine.scheduler import Lockstep

    torch.set_num_threads(1)
    eng = LLMEngine(_model(), max_batch=4, max_context=256, block_size=16, use_graphs=False)
    torch.manual_seed(100 + rank)              # the ranks' global generators differ on purpose
    ce = ContinuousEngine(eng, lockstep=Lockstep(None, src=0, leader=rank == 0))
    sp = SamplingParams(max_new_tokens=12, stop_on_eos=False, temperature=0.8, top_k=40)    # no seed
    if rank == 1:
        seen = []
        retire = ce._retire

        def spy(r):
            seen.append((r.seed, list(r.out)))
            retire(r)

        ce._retire = spy
        ce.follow()
        q.put((1, seen))
    else:
        ce.start()
        fut = ce.submit(_prompts((20,), seed=4)[0], sp)
        out = fut.result(timeout=120)
        ce.stop()
        ce.stop_followers()
        q.put((0, [(fut.request.seed, out)]))
    dist.destroy_process_group()


def test_lockstep_ranks_sample_the_same_stream():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_lockstep_worker, args=(r, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in ps:
        p.join(timeout=120)
        assert p.exitcode == 0, p.exitcode
    assert got[0] == got[1]
    (seed, out), = got[0]
    assert seed != 0 and len(out) == 12
