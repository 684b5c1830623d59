"""format: "json" on the GPU: the grammar kernels against the CPU reference (exact), the existing
picks on masked rows, and the HIP-graph scheduler end to end."""
from __future__ import annotations

import functools
import json

import numpy as np
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import grammar as G
from docqa_amd.ops import reference as ref
from tests.format_json_common import (EOS_SYN, coverage_states, engine_vocab, states_tensor, synthetic_vocab,
                                      vocab_on)
from tests.sample_oracle import CASES, DELTA, check, make_row
from tests.sample_seeded_oracle import build_case_min_p

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}
NEG = -float("inf")


@pytest.fixture(scope="module")
def native():
    assert ops.load_native(build_if_missing=True), "native extension missing"


@functools.lru_cache(maxsize=2)
def _vocab(kind: str):
    """(token bytes, eos id, n_valid, ld) of the two vocabularies."""
    if kind == "syn":
        toks = list(synthetic_vocab())
        return toks, EOS_SYN, len(toks), len(toks)
    from docqa_amd.text.tokenizer import ChatTokenizer

    tok = ChatTokenizer()
    return tok.token_bytes(32000), tok.tok.token_to_id("<|eot_id|>"), 32000, 32768


def _bits(x: torch.Tensor) -> torch.Tensor:
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


def _rows(R: int):
    """States and valid flags of an R-row bucket: the coverage states in turn; the 256-row
    bucket mixes in unconstrained rows (state 0) and padding rows (valid 0)."""
    cs = coverage_states()
    states = [cs[i % len(cs)] for i in range(R)]
    valid = [1] * R
    if R >= 256:
        for i in range(0, R, 5):
            states[i] = 0
        for i in range(3, R, 7):
            valid[i] = 0
    return states, valid


# ------------------------------------------------------------------ the kernels
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("R", (1, 3, 33, 256))
@pytest.mark.parametrize("kind", ("syn", "chat"))
def test_grammar_mask_matches_reference(native, kind, R, dt):
    toks, eos, n_valid, ld = _vocab(kind)
    assert kind != "syn" or n_valid % 64 != 0
    off, data, table = vocab_on("cpu", toks)
    states, valid = _rows(R)
    g = torch.Generator().manual_seed(R)
    x0 = (torch.randn(R, ld, generator=g) * 4).to(DTYPES[dt])
    want = x0.clone()
    st, vl = states_tensor(states, "cpu"), torch.tensor(valid, dtype=torch.int32)
    ref.grammar_mask(want, n_valid, st, off, data, table, eos, vl)
    got = x0.to(DEV)
    ops.grammar_mask(got, n_valid, st.to(DEV), off.to(DEV), data.to(DEV), table.to(DEV), eos,
                     vl.to(DEV) if R >= 256 else None)
    got = got.cpu()
    # the set of -inf columns is the reference's and every other element is the input's, bit for bit
    assert torch.equal(_bits(got), _bits(want))
    masked = want.float() == NEG
    assert torch.equal(_bits(got)[~masked], _bits(x0)[~masked])
    for r, (s, v) in enumerate(zip(states, valid)):
        if s == 0 or v == 0:
            assert not masked[r].any()
        else:
            assert masked[r, :n_valid].any() and not masked[r, :n_valid].all() and not masked[r, n_valid:].any()
            assert bool(masked[r, eos]) != G.is_done(s)


def test_grammar_advance_matches_reference(native):
    toks = list(synthetic_vocab())
    V = len(toks)
    off, data, table = vocab_on("cpu", toks)
    cs = coverage_states()
    st = torch.tensor(cs, dtype=torch.int64).repeat_interleave(V)
    nxt = torch.arange(V).repeat(len(cs))
    want = st.clone()
    ref.grammar_advance(want, nxt, off, data, table, EOS_SYN)
    got = st.to(DEV)
    ops.grammar_advance(got, nxt.to(DEV), off.to(DEV), data.to(DEV), table.to(DEV), EOS_SYN)
    assert torch.equal(got.cpu(), want)
    assert int((want != st).sum()) > V                            # most states move on many tokens
    # state 0, valid 0 and out-of-table ids stay
    z = torch.tensor([0, cs[0], cs[0], cs[0]], dtype=torch.int64, device=DEV)
    ops.grammar_advance(z, torch.tensor([300, 3 + 0x7B, V + 5, -1], device=DEV), off.to(DEV), data.to(DEV),
                        table.to(DEV), EOS_SYN, torch.tensor([1, 0, 1, 1], dtype=torch.int32, device=DEV))
    assert z.tolist() == [0, cs[0], cs[0], cs[0]]


# ------------------------------------------------------------------ picks on masked rows
def _pick_states():
    """After ``{`` (few tokens allowed), inside a string (most), after a value, inside a number,
    and DONE (exactly one: EOS)."""
    w = lambda d: G.walk(G.START_STATE, d)   # noqa: E731
    return {"open": w(b'{'), "string": w(b'{"a":"x'), "after": w(b'{"a":[1,"b"'), "number": w(b'{"a":-12'),
            "done": w(b'{"a":1}')}


@functools.lru_cache(maxsize=8)
def _masked_rows(kind: str, dt: str):
    """One masked row per pick state -> (names, x [S, V] of the dtype on the CPU, allowed [S, V])."""
    toks, eos, n_valid, _ = _vocab(kind)
    off, data, table = vocab_on("cpu", toks)
    names, states = zip(*_pick_states().items())
    x = torch.stack([torch.from_numpy(make_row(n_valid, 100 + i)) for i in range(len(states))]).to(DTYPES[dt])
    ref.grammar_mask(x, n_valid, states_tensor(states, "cpu"), off, data, table, eos)
    allowed = x.float() != NEG
    assert int(allowed[names.index("done")].sum()) == 1 and bool(allowed[names.index("done"), eos])
    return names, x, allowed


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ("syn", "chat"))
def test_greedy_picks_on_masked_rows(native, kind, dt):
    names, x, allowed = _masked_rows(kind, dt)
    S, V = x.shape
    got = ops.argmax(x.to(DEV)).cpu()
    assert torch.equal(got, ref.argmax(x))
    assert bool(allowed[torch.arange(S), got].all())
    # penalised: the window holds masked tokens, allowed tokens and the row's favourite
    W = ops.PENALTY_WINDOW
    g = torch.Generator().manual_seed(5)
    hist = torch.randint(0, V, (S, W), generator=g, dtype=torch.int32)
    for r in range(S):
        ok = torch.nonzero(allowed[r])[:, 0]
        hist[r, :8] = ok[torch.randint(0, len(ok), (8,), generator=g)].int()
        hist[r, 8] = got[r].int()
    hn = torch.full((S,), W, dtype=torch.int32)
    ln = torch.full((S,), 64, dtype=torch.int32)
    pen = [torch.full((S,), v) for v in (1.3, 0.5, 0.25)]
    want = ref.penalized_argmax(x, V, hist, hn, ln, *pen)
    gotp = ops.penalized_argmax(x.clone().to(DEV), V, hist.to(DEV), hn.to(DEV), ln.to(DEV),
                                *[p.to(DEV) for p in pen]).cpu()
    assert torch.equal(gotp, want)
    assert bool(allowed[torch.arange(S), gotp].all())
    assert gotp[names.index("done")] == got[names.index("done")]      # one allowed token: EOS either way


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("kind", ("syn", "chat"))
def test_seeded_sampler_on_masked_rows(native, kind, dt):
    """ops.sample_tokens (seed + index) on masked rows, every case of tests/sample_oracle.py (two
    of them with min_p as well): the draws lie in the fp64 CDF of the ALLOWED tokens -- a masked
    column has probability 0 and is never returned -- and equal the CPU reference's wherever the
    uniform is further than DELTA from an interval's end."""
    names, x, allowed = _masked_rows(kind, dt)
    S, V = x.shape
    n = 128
    seed = torch.full((n,), 2 ** 40 + 7, dtype=torch.int64)
    index = torch.arange(n, dtype=torch.int32)
    u = ref.seeded_uniform(seed, index).numpy()
    for r, name in enumerate(names):
        idx = torch.nonzero(allowed[r])[:, 0].numpy()
        row_c = x[r].float().numpy()[idx]                         # the allowed tokens' logits, as stored
        xr = x[r:r + 1].expand(n, -1).contiguous().to(DEV)
        for ci, case in enumerate(CASES):
            for min_p in ((0.0, ("m*", 0.05)) if ci in (1, 3) and len(idx) > 8 else (0.0,)):
                if len(idx) == 1 and case[2] == "p*":
                    case = (case[0], case[1], 1.0)               # one token: no top-p cutoff to place
                (it, k, p, mp), keep_c, cdf_c, _ = build_case_min_p(row_c, case, min_p)
                keep = np.zeros(V, dtype=bool)
                keep[idx] = keep_c
                cdf = np.zeros(V)
                cdf[idx] = cdf_c
                cdf = np.maximum.accumulate(cdf)                  # masked columns add no mass
                par = [torch.full((n,), v, dtype=t) for v, t in ((it, torch.float32), (k, torch.int32),
                                                                 (p, torch.float32), (mp, torch.float32))]
                tok = ops.sample_tokens(xr, V, *[t.to(DEV) for t in par], seed=seed.to(DEV),
                                        index=index.to(DEV)).cpu().numpy()
                assert allowed[r].numpy()[tok].all(), (name, case)
                check(tok, u, keep, cdf)
                sub = np.arange(0, n, 16)
                want = ref.sample_tokens(x[r:r + 1].expand(len(sub), -1), V, *[t[sub] for t in par],
                                         seed=seed[sub], index=index[sub]).numpy()
                ends = np.unique(cdf)
                clear = np.array([np.abs(ends - float(u[i])).min() > DELTA for i in sub])
                assert (tok[sub][clear] == want[clear]).all(), (name, case)
        if name == "done":
            assert len(idx) == 1


# ------------------------------------------------------------------ HIP-graph scheduler
@pytest.fixture(scope="module")
def model(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    return LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=23)


def test_scheduler_graphs_constrain_the_rows_that_ask(model, monkeypatch):
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.engine.scheduler import ContinuousEngine
    from tests.native_trace import record

    vocab, eos = engine_vocab(32000), 2
    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(3, 32000, (n,), generator=g).tolist() for n in (40, 23, 77, 5, 30, 51)]
    # fixed lengths (no EOS stop: a closed object goes on picking EOS, the one token DONE allows), so
    # the batch has the same rows at every step whether or not requests 0..3 are constrained
    seeded = SamplingParams(max_new_tokens=16, format="json", temperature=0.8, top_k=4, seed=99, stop_on_eos=False)
    cons = {0: SamplingParams(max_new_tokens=14, format="json", stop_on_eos=False),
            1: seeded,
            2: SamplingParams(max_new_tokens=12, format="json", repeat_penalty=1.3, presence_penalty=0.4,
                              repeat_last_n=32, logprobs=True, top_logprobs=2, stop_on_eos=False),
            3: SamplingParams(max_new_tokens=10, format="json", logprobs=True, top_logprobs=3, stop_on_eos=False)}
    free = {4: SamplingParams(max_new_tokens=12, stop_on_eos=False),
            5: SamplingParams(max_new_tokens=9, stop_on_eos=False, logprobs=True, top_logprobs=2)}

    def serve(which: dict):
        eng = LLMEngine(model, max_batch=8, max_context=256, use_graphs=True, prefix_cache=False)
        eng.set_vocab_bytes(vocab)
        ce = ContinuousEngine(eng)
        trace: list = []
        with record(trace):
            futs = {}
            for i, sp in which.items():
                futs[i] = ce.submit(prompts[i], sp)
                for _ in range(i % 3):
                    ce.step()
            while ce.has_work():
                ce.step()
        names = {t[0] for t in trace}
        return ce, {i: f.result() for i, f in futs.items()}, {i: f.request.logprobs for i, f in futs.items()}, names

    ce, out, lps, names = serve({**cons, **free})
    assert {"grammar_mask", "grammar_advance"} <= names
    assert any(k[-1] == "json" and gr.graph is not None for k, gr in ce._graphs.items())
    for i, sp in cons.items():
        s = G.START_STATE
        for t in out[i]:
            assert G.token_allowed(s, t, vocab, eos), (i, t, vocab[t], G.STATE_NAMES[s & 0xFF])
            s = G.advance_token(s, t, vocab, eos)
        assert len(out[i]) == sp.max_new_tokens
        if eos in out[i]:
            assert G.is_done(s) and set(out[i][out[i].index(eos):]) == {eos}
            assert isinstance(json.loads(b"".join(vocab[t] for t in out[i]).decode()), dict)
        assert len(lps[i]) == (len(out[i]) if sp.logprobs else 0)
    # unconstrained rows: what they get without the constrained requests, and such a batch
    # creates no constrained-flavour graph and launches neither grammar kernel
    plain = {i: SamplingParams(max_new_tokens=sp.max_new_tokens, stop_on_eos=False) for i, sp in cons.items()}
    ce0, out0, lps0, names0 = serve({**plain, **free})
    assert not names0 & {"grammar_mask", "grammar_advance"}
    assert all(len(k) == 6 for k in ce0._graphs)
    assert {i: out0[i] for i in free} == {i: out[i] for i in free} and lps0[5] == lps[5]
    assert any(out0[i] != out[i] for i in cons)
    # a seeded constrained request alone
    _, alone, _, _ = serve({1: seeded})
    assert alone[1] == out[1]
