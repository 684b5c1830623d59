"""Which native ops a model step launches, and with what arguments.

:func:`record` wraps ``ops._native()`` in a recording proxy (the trick of ``_spy_native`` in
tests/test_dgemm_mxfp4_gpu.py): every native op called through the ops wrappers appends its name,
every int / bool / float argument and the shape and dtype of every tensor argument.  :data:`CASES`
is the matrix tests/test_step_trace_gpu.py replays against tests/golden/step_traces.json:

  * the ``llama3-1b-test`` preset, seed 17, as bf16 / ``quantize_fp8()`` / ``quantize_mxfp4()``;
  * non-cascade decode steps of 1, 2, 3, 8, 16, 32 and 33 rows after prompts of 9..130 tokens,
    with the greedy pick of the M rows (``forward(..., greedy_ids=True)``).  The KV pool holds 16
    blocks where the prompts fit (M <= 3, the existing model tests' shape), else as many as the
    prompts take -- every row owns its blocks;
  * one 100-token prefill (the short-prefill plans) and one 600-token prefill;
  * each quantized model once with the shipped ring plan tables and once with every preset shape
    listed at every bucket (:func:`all_listed`).

``python -m tests.native_trace --record`` (on a GPU, from the repository root) rewrites the golden
file from the tree it runs in; the test never does.
"""
from __future__ import annotations

import contextlib
import json
import sys
from pathlib import Path

import torch

from docqa_amd import ops

GOLDEN = Path(__file__).resolve().parent / "golden" / "step_traces.json"
BS = 64
DECODE_ROWS = (1, 2, 3, 8, 16, 32, 33)
PREFILLS = (100, 600)
_LENS = (77, 130, 9, 20, 64, 100, 33, 128)          # the model tests' 77 / 130 / 9 first
STEPS = [f"decode{M}" for M in DECODE_ROWS] + [f"prefill{n}" for n in PREFILLS]
# (weights, plan tables)
VARIANTS = [("bf16", "shipped"), ("fp8", "shipped"), ("fp8", "listed"), ("mxfp4", "shipped"), ("mxfp4", "listed")]
CASES = [f"{w}-{t}-{s}" for w, t in VARIANTS for s in STEPS]


def _arg(a):
    if isinstance(a, torch.Tensor):
        return ["T", list(a.shape), str(a.dtype).replace("torch.", "")]
    if a is None or isinstance(a, (bool, int, float, str)):
        return a
    if isinstance(a, (list, tuple)):
        return [_arg(v) for v in a]
    return repr(type(a))


@contextlib.contextmanager
def record(trace: list):
    """Every native op called through ``ops._native()`` inside the block -> ``trace``."""
    real, orig = ops._native(), ops._native

    class Proxy:
        def __getattr__(self, name):
            fn = getattr(real, name)

            def call(*a, **k):
                trace.append([name, [_arg(v) for v in a], {n: _arg(v) for n, v in sorted(k.items())}])
                return fn(*a, **k)
            return call

    proxy = Proxy()
    ops._native = lambda: proxy
    try:
        yield trace
    finally:
        ops._native = orig


@contextlib.contextmanager
def all_listed(m, weights: str):
    """The ring kernels' three plan tables list every preset shape at every bucket (the fixture of
    tests/test_dgemm_mxfp4_gpu.py, for either format)."""
    d = {"fp8": "8", "mxfp4": "4"}[weights]
    L0, b = m.layers[0], (2, 4, 8, 16, 32)
    new = {f"_DGEMM{d}_SLAB": {tuple(L0[k].shape): b for k in ("qkv", "o", "down")},
           f"_DGEMM{d}_GLU": {tuple(L0["gate_up"].shape): b},
           f"_DGEMM{d}_LM": {tuple(m.lm_head.shape): b}}
    old = {k: getattr(ops, k) for k in new}
    for k, v in new.items():
        setattr(ops, k, v)
    try:
        yield m
    finally:
        for k, v in old.items():
            setattr(ops, k, v)


def build_model(weights: str):
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    m = LlamaModel(LlamaConfig.preset("llama3-1b-test"), device="cuda", seed=17)
    if weights == "fp8":
        m.quantize_fp8()
    elif weights == "mxfp4":
        m.quantize_mxfp4()
    return m


def _prompts(lens):
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, 32000, (n,), generator=g).tolist() for n in lens]


def _prefill(m, kv, prompts):
    from docqa_amd.models.llama import AttnMeta

    ids, pos, slots, cu, tables, nb = [], [], [], [0], [], 0
    for p in prompts:
        n = len(p)
        blocks = list(range(nb, nb + (n + BS) // BS + 1))
        nb += len(blocks)
        tables.append(blocks)
        ids += p
        pos += list(range(n))
        slots += [blocks[t // BS] * BS + t % BS for t in range(n)]
        cu.append(cu[-1] + n)
    meta = AttnMeta(prefill=True, positions=torch.tensor(pos, dtype=torch.int32, device="cuda"),
                    slot_mapping=torch.tensor(slots, dtype=torch.int32, device="cuda"),
                    cu_seqlens=torch.tensor(cu, dtype=torch.int32, device="cuda"),
                    max_len=max(len(p) for p in prompts))
    last = torch.tensor(cu[1:], device="cuda") - 1
    m.forward(torch.tensor(ids, dtype=torch.int32, device="cuda"), meta, kv, last)
    return tables


def _decode_greedy(m, kv, lens, tables):
    from docqa_amd.models.llama import AttnMeta

    B, maxb = len(lens), max(len(t) for t in tables)
    bt = torch.zeros(B, maxb, dtype=torch.int32)
    for i, t in enumerate(tables):
        bt[i, :len(t)] = torch.tensor(t)
    slots = [tables[i][n // BS] * BS + n % BS for i, n in enumerate(lens)]
    meta = AttnMeta(prefill=False, positions=torch.tensor(lens, dtype=torch.int32, device="cuda"),
                    slot_mapping=torch.tensor(slots, dtype=torch.int32, device="cuda"), block_tables=bt.cuda(),
                    context_lens=torch.tensor([n + 1 for n in lens], dtype=torch.int32, device="cuda"),
                    max_context=maxb * BS)
    tok = torch.tensor([4 + i for i in range(B)], dtype=torch.int32, device="cuda")
    return m.forward(tok, meta, kv, greedy_ids=True)


def run_step(m, step: str) -> list:
    """The trace of one step of :data:`STEPS` on model ``m``."""
    from docqa_amd.engine.kv_cache import KVCache

    n = int(step.removeprefix("prefill").removeprefix("decode"))
    lens = [n] if step.startswith("prefill") else [_LENS[i % len(_LENS)] for i in range(n)]
    blocks = max(16, sum((x + BS) // BS + 1 for x in lens))
    kv = KVCache(m.cfg.layers, blocks, m.hkv, m.cfg.head_dim, BS).caches
    prompts, trace = _prompts(lens), []
    if step.startswith("prefill"):
        with record(trace):
            _prefill(m, kv, prompts)
    else:
        tables = _prefill(m, kv, prompts)
        with record(trace):
            ids = _decode_greedy(m, kv, lens, tables)
        assert ids.shape == (n,)
    torch.cuda.synchronize()
    assert trace, step
    return trace


def run_case(m, case: str) -> list:
    weights, tables, step = case.split("-")
    assert m.weight_format.startswith(weights), (m.weight_format, case)
    if tables == "listed":
        with all_listed(m, weights):
            return run_step(m, step)
    return run_step(m, step)


def pack(traces: dict) -> dict:
    """{case: trace} with every distinct call stored once (the layers of a step repeat)."""
    calls, index, cases = [], {}, {}
    for case, trace in traces.items():
        row = []
        for c in trace:
            key = json.dumps(c)
            if key not in index:
                index[key] = len(calls)
                calls.append(c)
            row.append(index[key])
        cases[case] = row
    return {"calls": calls, "cases": cases}


def unpack(packed: dict) -> dict:
    return {case: [packed["calls"][i] for i in row] for case, row in packed["cases"].items()}


def load_golden() -> dict:
    return unpack(json.loads(GOLDEN.read_text()))


def main(argv) -> int:
    if argv != ["--record"]:
        print("usage: python -m tests.native_trace --record", file=sys.stderr)
        return 2
    assert ops.load_native(), "native extension missing"
    traces, models = {}, {}
    for case in CASES:
        w = case.split("-")[0]
        if w not in models:
            models.clear()          # one model resident at a time
            models[w] = build_model(w)
        traces[case] = json.loads(json.dumps(run_case(models[w], case)))
        print(f"{case}: {len(traces[case])} calls", flush=True)
    packed = pack(traces)
    GOLDEN.write_text(json.dumps(packed, separators=(",", ":")) + "\n")
    print(f"wrote {GOLDEN} ({len(packed['calls'])} distinct calls, {len(traces)} cases)")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
