"""Cost of per-token log-probabilities (csrc/kernels/logprobs.hip).

Operator part, bf16 logits of V = 128256 (Llama-3) and 32768 (Mistral) at R = 1 / 32 / 256 rows:
``ops.argmax`` (the project's yardstick for one pass over the logits) against
``ops.token_logprobs`` into caller-supplied buffers with every row's ``top_n`` at 0 (the picked
token's logprob only) and at 20.  The logits rotate through up to 16 copies (at most 768 MB): only
256 rows of 128256 logits (16 x 66 MB) go past the 256 MB MALL, every other case stays within
it -- cache-resident for both ops alike, as the logits the LM head has just written are in a decode
step.  Medians of WINDOWS windows of ITERS calls.

Engine part: Llama-3-8B random-init, ``engine.generate`` at batch 1, 32 and 256 for 128 tokens,
greedy with ``logprobs`` off (the fused LM-head argmax), with ``logprobs`` and ``top_logprobs`` 0,
and with ``top_logprobs`` 20; then penalised greedy (``repeat_penalty`` 1.1 over 64 tokens) and
sampled (temperature 0.8, top-k 40) without and with ``logprobs`` (``top_logprobs`` 0), whose logprob
flavours copy the logits for the pick; one process: ms per decode step from the engine's event-timed decode
span, median of RUNS runs after a warm-up run that captures the graph.

python benchmarks/bench_logprobs.py [--part ops|engine|all] [--flavours off,lp0,lp20,pen,pen_lp0,smp,smp_lp0]
                                    [--batches 1,32,256] [--llm llama3-8b]
-> one JSON line per measurement, then a table."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

VOCABS = (128256, 32768)
WINDOWS, ITERS, RUNS = 7, 20, 3


def _time(fn, copies):
    for i in range(max(copies, 3)):
        fn(i % copies)
    torch.cuda.synchronize()
    ts = []
    for w in range(WINDOWS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(ITERS):
            fn((w * ITERS + i) % copies)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / ITERS)
    return statistics.median(ts), min(ts), max(ts)


def ops_part(rows_out):
    T = ops.TOP_LOGPROBS_MAX
    g = torch.Generator(device="cuda").manual_seed(1)
    for V in VOCABS:
        for R in (1, 32, 256):
            copies = min(16, max(2, (768 << 20) // (R * V * 2) + 1))
            bf = [(torch.randn(R, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(copies)]
            chosen = torch.randint(0, V, (R,), device="cuda", generator=g)
            tn = {n: torch.full((R,), n, dtype=torch.int32, device="cuda") for n in (0, T)}
            lp = torch.empty(R, device="cuda")
            ti = torch.empty(R, T, dtype=torch.int32, device="cuda")
            tl = torch.empty(R, T, device="cuda")
            cands = {
                "argmax_bf16": lambda i: ops.argmax(bf[i]),
                "token_logprobs_top0": lambda i: ops.token_logprobs(bf[i], V, chosen, tn[0], lp, ti, tl),
                "token_logprobs_top20": lambda i: ops.token_logprobs(bf[i], V, chosen, tn[T], lp, ti, tl),
            }
            base = None
            for name, fn in cands.items():
                med, lo, hi = _time(fn, copies)
                base = med if base is None else base
                rows_out.append({"part": "ops", "op": name, "R": R, "V": V, "us": round(med, 2),
                                 "min_us": round(lo, 2), "max_us": round(hi, 2), "x_argmax": round(med / base, 2)})
                print(json.dumps(rows_out[-1]), flush=True)
            del bf
            torch.cuda.empty_cache()


def engine_part(rows_out, llm, batches, flavours, new=128):
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.models import checkpoint as ck

    model = ck.resolve_llama(llm, device="cuda", seed=0)
    eng = LLMEngine(model, max_batch=max(batches), max_context=512, use_graphs=True, prefix_cache=False)
    params = {
        "off": SamplingParams(max_new_tokens=new, stop_on_eos=False),
        "lp0": SamplingParams(max_new_tokens=new, stop_on_eos=False, logprobs=True),
        "lp20": SamplingParams(max_new_tokens=new, stop_on_eos=False, logprobs=True, top_logprobs=20),
        "pen": SamplingParams(max_new_tokens=new, stop_on_eos=False, repeat_penalty=1.1, repeat_last_n=64),
        "pen_lp0": SamplingParams(max_new_tokens=new, stop_on_eos=False, repeat_penalty=1.1, repeat_last_n=64,
                                  logprobs=True),
        "smp": SamplingParams(max_new_tokens=new, stop_on_eos=False, temperature=0.8, top_k=40, seed=3),
        "smp_lp0": SamplingParams(max_new_tokens=new, stop_on_eos=False, temperature=0.8, top_k=40, seed=3,
                                  logprobs=True),
    }
    over = {"lp0": "off", "lp20": "off", "pen_lp0": "pen", "smp_lp0": "smp"}
    g = torch.Generator().manual_seed(2)
    for B in batches:
        prompts = [torch.randint(3, model.cfg.vocab_size, (64,), generator=g).tolist() for _ in range(B)]
        ms = {}
        for name in flavours:
            eng.collect(eng.launch(prompts, params[name]))         # captures the flavour's graph
            runs = []
            for _ in range(RUNS):
                d0 = eng.stats.decode_s
                eng.collect(eng.launch(prompts, params[name]))
                runs.append((eng.stats.decode_s - d0) * 1e3 / (new - 1))
            ms[name] = statistics.median(runs)
            rows_out.append({"part": "engine", "llm": llm, "batch": B, "flavour": name, "new_tokens": new,
                             "ms_per_step": round(ms[name], 4), "min_ms": round(min(runs), 4),
                             "max_ms": round(max(runs), 4)})
            if over.get(name) in ms:
                rows_out[-1]["us_over_" + over[name]] = round((ms[name] - ms[over[name]]) * 1e3, 1)
            print(json.dumps(rows_out[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["ops", "engine", "all"])
    ap.add_argument("--flavours", default="off,lp0,lp20,pen,pen_lp0,smp,smp_lp0")
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--llm", default="llama3-8b")
    a = ap.parse_args()
    assert ops.load_native()
    rows = []
    with torch.inference_mode():
        if a.part in ("ops", "all"):
            ops_part(rows)
        if a.part in ("engine", "all"):
            engine_part(rows, a.llm, [int(b) for b in a.batches.split(",")], a.flavours.split(","))
    print("\n%-8s %-24s %7s %6s %12s %12s %12s" % ("part", "what", "vocab", "rows", "median", "min", "max"))
    for r in rows:
        if r["part"] == "ops":
            print("%-8s %-24s %7d %6d %9.2f us %9.2f us %9.2f us  %.2fx argmax" % (
                "ops", r["op"], r["V"], r["R"], r["us"], r["min_us"], r["max_us"], r["x_argmax"]))
        else:
            print("%-8s %-24s %7s %6d %9.4f ms %9.4f ms %9.4f ms" % ("engine", r["flavour"] + " /step", "", r["batch"],
                                                                     r["ms_per_step"], r["min_ms"], r["max_ms"]))


if __name__ == "__main__":
    main()
