"""Cost of the repeat / presence / frequency penalties (csrc/kernels/embed_sample.hip).

Operator part, V = 128256 (Llama-3) at R = 1 / 32 / 256 rows: ``ops.argmax`` on bf16 logits
(the unpenalised pick from materialised logits), ``ops.penalized_argmax`` on the same logits
with a full 64-token window per row, ``ops.apply_penalties`` on fp32 logits, and the stochastic
path with the same penalties (fp32 copy + apply_penalties + ``ops.sample`` at top-k 40).  The
logits rotate through copies past the 256 MB MALL; medians of WINDOWS windows of ITERS calls.

Engine part: Llama-3-8B random-init, ``engine.generate`` at batch 1 and 256 for 128 tokens with
``repeat_penalty`` 1.0 (the fused LM-head argmax) against 1.1 (penalised greedy), and sampled
at temperature 0.8 with 1.1, one process: ms per decode step from the engine's event-timed
decode span, median of RUNS runs after a warm-up run that captures the graph.

python benchmarks/bench_penalties.py [--part ops|engine|all] [--flavours plain,greedy,sampled]
                                     [--batches 1,256] [--llm llama3-8b]
-> one JSON line per measurement, then a table."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

V = 128256
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
    W = ops.PENALTY_WINDOW
    g = torch.Generator(device="cuda").manual_seed(1)
    for R in (1, 32, 256):
        copies = min(16, max(2, (768 << 20) // (R * V * 2) + 1))
        bf = [(torch.randn(R, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(copies)]
        f32 = [x.float() for x in bf[:max(2, copies // 2)]]
        hist = torch.randint(0, V, (R, W), device="cuda", generator=g, dtype=torch.int32)
        hn = torch.full((R,), W + 17, dtype=torch.int32, device="cuda")
        ln = torch.full((R,), 64, dtype=torch.int32, device="cuda")
        rp = torch.full((R,), 1.1, device="cuda")
        z = torch.zeros(R, device="cuda")
        valid = torch.ones(R, dtype=torch.int32, device="cuda")
        it, tk, tp = torch.full((R,), 1.25, device="cuda"), torch.full((R,), 40, dtype=torch.int32, device="cuda"), \
            torch.ones(R, device="cuda")
        u = torch.rand(R, device="cuda", generator=g)

        def sampled(i):
            full = bf[i].float()
            ops.apply_penalties(full, hist, hn, ln, rp, z, z, valid)
            return ops.sample(full, it, tk, tp, u)

        cands = {
            "argmax_bf16": (lambda i: ops.argmax(bf[i]), copies),
            "penalized_argmax_bf16": (lambda i: ops.penalized_argmax(bf[i], V, hist, hn, ln, rp, z, z, valid), copies),
            "apply_penalties_fp32": (lambda i: ops.apply_penalties(f32[i], hist, hn, ln, rp, z, z, valid), len(f32)),
            "float_apply_sample": (sampled, copies),
        }
        for name, (fn, c) in cands.items():
            med, lo, hi = _time(fn, c)
            rows_out.append({"part": "ops", "op": name, "R": R, "V": V, "us": round(med, 2), "min_us": round(lo, 2),
                             "max_us": round(hi, 2)})
            print(json.dumps(rows_out[-1]), flush=True)
        del bf, f32
        torch.cuda.empty_cache()


def engine_part(rows_out, llm, batches, flavours, new=128):
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.models import checkpoint as ck

    model = ck.resolve_llama(llm, device="cuda", seed=0)
    eng = LLMEngine(model, max_batch=max(batches), max_context=512, use_graphs=True, prefix_cache=False)
    params = {
        "plain": SamplingParams(max_new_tokens=new, stop_on_eos=False, repeat_penalty=1.0),
        "greedy": SamplingParams(max_new_tokens=new, stop_on_eos=False, repeat_penalty=1.1, repeat_last_n=64),
        "sampled": SamplingParams(max_new_tokens=new, stop_on_eos=False, repeat_penalty=1.1, repeat_last_n=64,
                                  temperature=0.8, top_k=40, seed=3),
    }
    g = torch.Generator().manual_seed(2)
    for B in batches:
        prompts = [torch.randint(3, model.cfg.vocab_size, (64,), generator=g).tolist() for _ in range(B)]
        ms = {}
        for name in flavours:
            eng.generate(prompts, params[name])                     # captures the flavour's graph
            runs = []
            for _ in range(RUNS):
                d0 = eng.stats.decode_s
                out = eng.generate(prompts, params[name])
                runs.append((eng.stats.decode_s - d0) * 1e3 / (new - 1))
            ms[name] = statistics.median(runs)
            rep = sum(len(o) - len(set(o)) for o in out) / B       # repeated tokens per answer
            rows_out.append({"part": "engine", "llm": llm, "batch": B, "flavour": name, "new_tokens": new,
                             "ms_per_step": round(ms[name], 4), "min_ms": round(min(runs), 4),
                             "max_ms": round(max(runs), 4), "repeated_tokens_per_answer": round(rep, 1)})
            if "plain" in ms and name != "plain":
                rows_out[-1]["us_over_plain"] = round((ms[name] - ms["plain"]) * 1e3, 1)
            print(json.dumps(rows_out[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["ops", "engine", "all"])
    ap.add_argument("--flavours", default="plain,greedy,sampled")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--llm", default="llama3-8b")
    a = ap.parse_args()
    assert ops.load_native()
    rows = []
    with torch.inference_mode():
        if a.part in ("ops", "all"):
            ops_part(rows)
        if a.part in ("engine", "all"):
            engine_part(rows, a.llm, [int(b) for b in a.batches.split(",")], a.flavours.split(","))
    print("\n%-8s %-24s %6s %12s %12s %12s" % ("part", "what", "rows", "median", "min", "max"))
    for r in rows:
        if r["part"] == "ops":
            print("%-8s %-24s %6d %9.2f us %9.2f us %9.2f us" % ("ops", r["op"], r["R"], r["us"], r["min_us"], r["max_us"]))
        else:
            print("%-8s %-24s %6d %9.4f ms %9.4f ms %9.4f ms" % ("engine", r["flavour"] + " /step", r["batch"],
                                                                 r["ms_per_step"], r["min_ms"], r["max_ms"]))


if __name__ == "__main__":
    main()
