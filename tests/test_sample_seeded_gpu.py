"""``sample_tokens_kernel`` / ``seeded_uniform_kernel`` (csrc/kernels/sample.hip) against the CPU
Philox reference and the fp64 oracle of tests/sample_seeded_oracle.py: every vocabulary shape of
the case matrix in fp32 (rows read from memory) and bf16 (rows held in registers, 1..16 vectors a
thread), ``min_p`` off and on, padded and misaligned rows, per-row parameters in one launch, and
the continuous scheduler's HIP-graph decode reproducing its seeded requests.

Every input's preconditions are asserted and every draw is checked against ``DELTA``; each check
prints the largest distance of a draw from its exact CDF interval.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from docqa_amd.ops import reference as ref
from tests.sample_oracle import CASES, DELTA, VS, check, make_row, peaked_row, scaled, tied_kth_row
from tests.sample_seeded_oracle import INDICES, SEEDS, build_case_min_p, to_bf16

pytestmark = pytest.mark.gpu

DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops.native_loaded()
    return ops


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _streams(n: int, salt: int):
    """Row i's (seed_i, index_i) and the uniform the CPU reference gives it."""
    seed = torch.arange(n, dtype=torch.int64) * 2654435761 + (salt << 33) + 1
    index = (torch.arange(n, dtype=torch.int32) * 37 + salt) % 8192
    return seed, index, ref.seeded_uniform(seed, index).numpy()


def _rounded(row, dt):
    return to_bf16(row) if dt == "bf16" else np.asarray(row, dtype=np.float32)


def _launch(logits, n_valid, par, seed, index, valid=None):
    it, k, p, m = (np.asarray(c) for c in zip(*par))
    out = torch.ops.docqa.sample_tokens(logits, n_valid, _dev(it, torch.float32), _dev(k, torch.int32),
                                        _dev(p, torch.float32), _dev(m, torch.float32), None, seed.cuda(),
                                        index.cuda(), None if valid is None else valid.cuda())
    return out.cpu().numpy()


def test_seeded_uniform_bit_equal(native):
    grid = [(s, i) for s in SEEDS for i in INDICES]
    seed = torch.tensor([s for s, _ in grid], dtype=torch.int64)
    index = torch.tensor([i for _, i in grid], dtype=torch.int32)
    got = native.seeded_uniform(seed.cuda(), index.cuda()).cpu()
    want = ref.seeded_uniform(seed, index)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert float(got.max()) < 1.0


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("V", VS)
def test_case_matrix(V, dt):
    n = 256
    worst = 0.0
    for ci, case in enumerate(CASES):
        row = _rounded(make_row(V, seed=100 * ci + V), dt)
        logits = _dev(row, DTYPES[dt]).expand(n, -1).contiguous()
        for mi, mp in enumerate((0.0, ("m*", 0.05))):
            params, keep, cdf, _ = build_case_min_p(row, case, mp)
            seed, index, u = _streams(n, salt=2 * ci + mi)
            tok = _launch(logits, V, [params] * n, seed, index)
            worst = max(worst, check(tok, u, keep, cdf))
    print(f"overshoot {worst:.3e} of delta {DELTA:g}: V={V} {dt}")


def test_min_p_keeps_hundreds():
    """A flat row (spread 1): min_p 0.05 keeps hundreds of tokens, 0.5 still dozens."""
    V, n = 32000, 256
    for dt in DTYPES:
        row = _rounded(make_row(V, seed=900 + V, spread=1.0), dt)
        logits = _dev(row, DTYPES[dt]).expand(n, -1).contiguous()
        for mi, target in enumerate((0.05, 0.5)):
            params, keep, cdf, info = build_case_min_p(row, (1.25, 0, 1.0), ("m*", target))
            assert info["n_keep"] > (100 if target == 0.05 else 10)
            seed, index, u = _streams(n, salt=40 + mi)
            over = check(_launch(logits, V, [params] * n, seed, index), u, keep, cdf)
            print(f"overshoot {over:.3e} of delta {DELTA:g}: flat row {dt} min_p={params[3]:.4f} keeps {info['n_keep']}")


@pytest.mark.parametrize("dt,n_valid,ld", [("bf16", 2051, 2056), ("fp32", 2051, 2052), ("bf16", 2051, 2053),
                                           ("bf16", 1000, 1001)])
def test_padded_columns(dt, n_valid, ld):
    """Columns at or past n_valid hold +1e30 and would win every draw if they were read; a bf16
    row stride that is no multiple of 8 takes the kernel's path over memory."""
    n = 256
    row = _rounded(make_row(n_valid, seed=900 + n_valid), dt)
    wide = torch.full((n, ld), 1e30, dtype=DTYPES[dt], device="cuda")
    wide[:, :n_valid] = _dev(row, DTYPES[dt])
    for mi, mp in enumerate((0.0, ("m*", 0.05))):
        params, keep, cdf, _ = build_case_min_p(row, (1.25, 40, "p*"), mp)
        seed, index, u = _streams(n, salt=60 + mi)
        over = check(_launch(wide, n_valid, [params] * n, seed, index), u, keep, cdf)
        print(f"overshoot {over:.3e} of delta {DELTA:g}: {dt} n_valid={n_valid} ld={ld}")
    # an unaligned base: rows of a view that starts one element in
    if dt == "bf16" and ld % 8 == 0:
        params, keep, cdf, _ = build_case_min_p(row[1:], (1.0, 0, 1.0), 0.0)
        seed, index, u = _streams(n, salt=63)
        check(_launch(wide[:, 1:], n_valid - 1, [params] * n, seed, index), u, keep, cdf)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("rows", [1, 3, 64, 257])
def test_mixed_launch(rows, dt):
    """Each row its own logits (a strided view of a wider buffer), parameter tuple, min_p and
    stream; ``top_k == 1`` rows and a ``valid == 0`` row sit between the sampled ones."""
    V, ld = 1000, 1008
    tuples = list(CASES) + [(1.0, 1, 1.0), (1.25, 1, 0.5)]
    logits = np.stack([_rounded(make_row(V, seed=5000 + r), dt) for r in range(rows)])
    seed, index, u = _streams(rows, salt=70)
    valid = torch.ones(rows, dtype=torch.int32)
    dead = 1 if rows > 1 else -1
    if dead >= 0:
        valid[dead] = 0
    par, orc = [], []
    for r in range(rows):
        case = tuples[r % len(tuples)]
        mp = ("m*", 0.05) if r % 2 else 0.0
        if case[1] == 1:
            par.append((case[0], 1, case[2], 0.3 if r % 2 else 0.0))
            orc.append(None)
        else:
            params, keep, cdf, _ = build_case_min_p(logits[r], case, mp)
            par.append(params)
            orc.append((keep, cdf))
    wide = torch.full((rows, ld), 1e30, dtype=DTYPES[dt], device="cuda")
    wide[:, :V] = _dev(logits, DTYPES[dt])
    tok = _launch(wide[:, :V], V, par, seed, index, valid)
    worst = 0.0
    for r in range(rows):
        if r == dead:
            assert tok[r] == 0, "a valid == 0 row writes token 0"
        elif orc[r] is None:
            assert tok[r] == int(np.argmax(scaled(logits[r], par[r][0]))), f"row {r}: top_k == 1 is an argmax"
        else:
            worst = max(worst, check(tok[r:r + 1], u[r:r + 1], *orc[r]))
    print(f"overshoot {worst:.3e} of delta {DELTA:g}: mixed launch rows={rows} {dt}")


@pytest.mark.parametrize("dt", list(DTYPES))
def test_ties_and_peaks(dt):
    n = 256
    # ties at the k-th value are all kept, with and without min_p
    row = _rounded(tied_kth_row(), dt)
    for mi, mp in enumerate((0.0, ("m*", 0.05))):
        params, keep, cdf, info = build_case_min_p(row, (1.25, 40, 1.0), mp)
        if mi == 0:
            assert info["n_keep"] >= 42
        seed, index, u = _streams(n, salt=80 + mi)
        check(_launch(_dev(row, DTYPES[dt]).expand(n, -1).contiguous(), len(row), [params] * n, seed, index),
              u, keep, cdf)
    # a tied maximum under min_p 1.0: both copies kept, u picks between them; top_k 1: the lower
    row, at = peaked_row(1000, seed=9)
    row[at + 100] = row[at]
    row = _rounded(row, dt)
    params, keep, cdf, info = build_case_min_p(row, (1.0, 0, 1.0), 1.0)
    assert info["n_keep"] == 2
    seed, index, u = _streams(n, salt=82)
    logits = _dev(row, DTYPES[dt]).expand(n, -1).contiguous()
    tok = _launch(logits, len(row), [params] * n, seed, index)
    check(tok, u, keep, cdf)
    assert (tok == np.where(u < 0.5, at, at + 100)).all() and len(set(tok.tolist())) == 2
    tok = _launch(logits, len(row), [(1.0, 1, 1.0, 1.0)] * n, seed, index)
    assert (tok == at).all()
    # one token holds all the mass: every draw returns it
    row, at = peaked_row(128256, seed=10)
    row = _rounded(row, dt)
    params, keep, cdf, _ = build_case_min_p(row, (1.0, 0, 1.0), ("m*", 0.05))
    tok = _launch(_dev(row, DTYPES[dt]).expand(n, -1).contiguous(), len(row), [params] * n, seed, index)
    check(tok, u, keep, cdf)
    assert (tok == at).all()


# ----------------------------------------------------------------------------- llama3-1b-test
@pytest.fixture(scope="module")
def model(native):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    return LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=23)


def test_scheduler_graphs_reproduce_seeded_requests(model, monkeypatch):
    """Six staggered requests on HIP graphs, three of them seeded-sampled (one penalised, one with
    logprobs): two runs on fresh schedulers, the global generator never reseeded, give the seeded
    requests the same tokens; the greedy ones get what they get when the other three slots hold
    greedy requests instead."""
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.engine.scheduler import ContinuousEngine

    g = torch.Generator().manual_seed(12)
    prompts = [torch.randint(3, 32000, (n,), generator=g).tolist() for n in (40, 23, 77, 5, 30, 51)]
    base = dict(stop_on_eos=False)
    sampled = {0: SamplingParams(max_new_tokens=12, seed=1234, temperature=0.8, top_k=40, **base),
               2: SamplingParams(max_new_tokens=10, seed=77, temperature=1.0, top_p=0.9, min_p=0.05,
                                 repeat_penalty=1.3, repeat_last_n=16, **base),
               4: SamplingParams(max_new_tokens=9, seed=2 ** 40 + 3, temperature=0.7, top_k=20, logprobs=True,
                                 top_logprobs=2, **base)}
    lens = [12, 8, 10, 11, 9, 7]

    def serve(with_sampled: bool):
        ce = ContinuousEngine(LLMEngine(model, max_batch=8, max_context=256, use_graphs=True, prefix_cache=False))
        futs = []
        for i, (p, n) in enumerate(zip(prompts, lens)):
            sp = sampled[i] if with_sampled and i in sampled else SamplingParams(max_new_tokens=n, **base)
            futs.append(ce.submit(p, sp))
            for _ in range(i % 3):
                ce.step()
        while ce.has_work():
            ce.step()
        assert any(g.graph is not None and g.seeded and not k[1] for k, g in ce._graphs.items()) == with_sampled
        return [f.result() for f in futs], [f.request.logprobs for f in futs]

    one, lp1 = serve(True)
    torch.rand(3, device="cuda")                 # the global generators move on between the runs
    torch.rand(3)
    two, lp2 = serve(True)
    for i in sampled:
        assert one[i] == two[i] and len(one[i]) == lens[i]
    assert lp1[4] == lp2[4] and len(lp1[4]) == lens[4]
    assert len({tuple(one[i]) for i in sampled}) == 3
    greedy, _ = serve(False)
    for i in (1, 3, 5):
        assert one[i] == two[i] == greedy[i]
    assert any(one[i] != greedy[i] for i in sampled)
