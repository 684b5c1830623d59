"""Cost of a sampled pick: the one-read sampler (csrc/kernels/sample.hip) against the path it
replaces in the continuous scheduler.

Operator part, bf16 logits of V = 128256 (Llama-3) and 32768 (Mistral) at R = 1 / 32 / 256 rows,
temperature 0.8, top-k 40, top-p 0.9: ``logits.float()`` + ``torch.rand`` + ``ops.sample`` (the
scheduler's pick before ``ops.sample_tokens``) against ``ops.sample_tokens(seed=.., index=..)`` with
``min_p`` 0 and 0.05.  The logits rotate through up to 16 copies (at most 768 MB), as in
bench_logprobs.py.  Medians of WINDOWS windows of ITERS calls.  A tree without
``ops.sample_tokens`` measures the first path alone.

Scheduler part: Llama-3-8B random-init, ``ContinuousEngine.generate`` at batch 1, 32 and 256 for
128 tokens, greedy and sampled (temperature 0.8, top-k 40, top-p 0.9, a seed per run): ms per decode
step from the scheduler's decode span over its step count, median of RUNS runs after a warm-up
run that captures the graphs.  Run it on two trees to compare their sampled steps.

python benchmarks/bench_sample_seeded.py [--part ops|engine|all] [--batches 1,32,256] [--llm llama3-8b]
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
    g = torch.Generator(device="cuda").manual_seed(1)
    for V in VOCABS:
        for R in (1, 32, 256):
            copies = min(16, max(2, (768 << 20) // (R * V * 2) + 1))
            bf = [(torch.randn(R, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(copies)]
            it = torch.full((R,), 1.0 / 0.8, device="cuda")
            tk = torch.full((R,), 40, dtype=torch.int32, device="cuda")
            tp = torch.full((R,), 0.9, device="cuda")
            mp = {m: torch.full((R,), m, device="cuda") for m in (0.0, 0.05)}
            seed = torch.arange(1, R + 1, dtype=torch.int64, device="cuda") * 7919
            index = torch.full((R,), 100, dtype=torch.int32, device="cuda")
            cands = {"float_rand_sample": lambda i: ops.sample(bf[i].float(), it, tk, tp, torch.rand(R, device="cuda"))}
            if hasattr(ops, "sample_tokens"):
                cands["sample_tokens_seeded"] = lambda i: ops.sample_tokens(bf[i], V, it, tk, tp, mp[0.0], seed=seed,
                                                                            index=index)
                cands["sample_tokens_seeded_min_p"] = lambda i: ops.sample_tokens(bf[i], V, it, tk, tp, mp[0.05],
                                                                                  seed=seed, index=index)
            base = None
            for name, fn in cands.items():
                med, lo, hi = _time(fn, copies)
                base = med if base is None else base
                rows_out.append({"part": "ops", "op": name, "R": R, "V": V, "us": round(med, 2),
                                 "min_us": round(lo, 2), "max_us": round(hi, 2), "x_old": round(med / base, 3)})
                print(json.dumps(rows_out[-1]), flush=True)
            del bf
            torch.cuda.empty_cache()


def engine_part(rows_out, llm, batches, new=128):
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.engine.scheduler import ContinuousEngine
    from docqa_amd.models import checkpoint as ck

    model = ck.resolve_llama(llm, device="cuda", seed=0)
    eng = LLMEngine(model, max_batch=max(batches), max_context=512, use_graphs=True, prefix_cache=False)
    ce = ContinuousEngine(eng)
    g = torch.Generator().manual_seed(2)
    for B in batches:
        prompts = [torch.randint(3, model.cfg.vocab_size, (64,), generator=g).tolist() for _ in range(B)]
        ms = {}
        for name in ("greedy", "sampled"):
            def params(run):
                if name == "greedy":
                    return SamplingParams(max_new_tokens=new, stop_on_eos=False)
                return SamplingParams(max_new_tokens=new, stop_on_eos=False, temperature=0.8, top_k=40, top_p=0.9,
                                      seed=3 + run)

            ce.generate(prompts, params(0))                       # captures the flavour's graphs
            runs = []
            for run in range(RUNS):
                d0, s0 = eng.stats.decode_s, ce.steps
                ce.generate(prompts, params(run + 1))
                runs.append((eng.stats.decode_s - d0) * 1e3 / max(1, ce.steps - s0))
            ms[name] = statistics.median(runs)
            rows_out.append({"part": "engine", "llm": llm, "batch": B, "flavour": name, "new_tokens": new,
                             "seeded": hasattr(ops, "sample_tokens"), "ms_per_step": round(ms[name], 4),
                             "min_ms": round(min(runs), 4), "max_ms": round(max(runs), 4)})
            if name == "sampled":
                rows_out[-1]["us_over_greedy"] = round((ms[name] - ms["greedy"]) * 1e3, 1)
            print(json.dumps(rows_out[-1]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default="all", choices=["ops", "engine", "all"])
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--llm", default="llama3-8b")
    a = ap.parse_args()
    assert ops.load_native()
    rows = []
    with torch.inference_mode():
        if a.part in ("ops", "all"):
            ops_part(rows)
        if a.part in ("engine", "all"):
            engine_part(rows, a.llm, [int(b) for b in a.batches.split(",")])
    print("\n%-8s %-28s %7s %6s %12s %12s %12s" % ("part", "what", "vocab", "rows", "median", "min", "max"))
    for r in rows:
        if r["part"] == "ops":
            print("%-8s %-28s %7d %6d %9.2f us %9.2f us %9.2f us  %.3fx old" % (
                "ops", r["op"], r["V"], r["R"], r["us"], r["min_us"], r["max_us"], r["x_old"]))
        else:
            print("%-8s %-28s %7s %6d %9.4f ms %9.4f ms %9.4f ms" % ("engine", r["flavour"] + " /step", "", r["batch"],
                                                                     r["ms_per_step"], r["min_ms"], r["max_ms"]))


if __name__ == "__main__":
    main()
