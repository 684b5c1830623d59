"""Cost of ``format: "json"``: the grammar kernels (csrc/kernels/grammar.hip) alone and inside
the continuous scheduler's decode step.

Operator part, bf16 logits of V = 128256 (Llama-3) and 32768 at R = 1 / 32 / 256 rows, the chat
tokenizer's bytes, every row in the same state, three states: ``open`` (after ``{``: few tokens
allowed, most die on the first-byte set), ``string`` (inside a string: most tokens allowed, every
byte of every token walked) and ``done`` (no table, everything but EOS masked).  ``ops.grammar_mask``,
``ops.grammar_advance`` and, beside them, ``ops.argmax`` on the same logits.  The logits rotate
through up to 16 copies (at most 768 MB), as in bench_logprobs.py; medians of WINDOWS windows of
ITERS calls.  The mask writes -inf over the copies, which does not change what it costs: it reads
no logit and stores to the same columns every time.

Engine part: Llama-3-8B random-init, ``ContinuousEngine.generate`` at batch 1, 32 and 256 for 128
tokens (fixed length: a closed object goes on picking EOS), arms interleaved in one process: plain
greedy, greedy with logits (``logprobs`` with ``top_logprobs`` 0: the same unfused LM head),
constrained greedy, sampled and constrained sampled.  ms per decode step from the scheduler's
decode span over its step count, median of RUNS runs after a warm-up run that captures the graphs.

python benchmarks/bench_format_json.py [--part ops|engine|all] [--batches 1,32,256] [--llm llama3-8b]
-> one JSON line per measurement, then a table."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402
from docqa_amd.ops import grammar as G  # noqa: E402

VOCABS = (128256, 32768)
WINDOWS, ITERS, RUNS = 7, 20, 3
STATES = {"open": b'{', "string": b'{"a":"x', "done": b'{"a":1}'}


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


def _chat_vocab(V):
    from docqa_amd.text.tokenizer import ChatTokenizer

    tok = ChatTokenizer(model_vocab=V)
    tb = tok.token_bytes(V)
    off, data = G.vocab_tensors(tb)
    return tb, tok.eos_id if tok.eos_id < V else tok.tok.token_to_id("<|eot_id|>"), off.cuda(), data.cuda()


def ops_part(rows_out):
    g = torch.Generator(device="cuda").manual_seed(1)
    table = G.table().cuda()
    for V in VOCABS:
        tb, eos, off, data = _chat_vocab(V)
        nbytes = sum(map(len, tb))
        for R in (1, 32, 256):
            copies = min(16, max(2, (768 << 20) // (R * V * 2) + 1))
            bf = [(torch.randn(R, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(copies)]
            base, _, _ = _time(lambda i: ops.argmax(bf[i]), copies)
            rows_out.append({"part": "ops", "op": "argmax", "state": "-", "R": R, "V": V, "us": round(base, 2)})
            print(json.dumps(rows_out[-1]), flush=True)
            for name, doc in STATES.items():
                s = G.walk(G.START_STATE, doc)
                st = torch.full((R,), s, dtype=torch.int64, device="cuda")
                allowed = sum(G.token_allowed(s, t, tb, eos) for t in range(len(tb)) if tb[t] or t == eos)
                nxt = torch.full((R,), next(t for t in range(len(tb)) if G.token_allowed(s, t, tb, eos)),
                                 dtype=torch.int64, device="cuda")
                keep = st.clone()
                for op, fn in (("grammar_mask", lambda i: ops.grammar_mask(bf[i], V, st, off, data, table, eos)),
                               ("grammar_advance", lambda i: (st.copy_(keep), ops.grammar_advance(
                                   st, nxt, off, data, table, eos)))):
                    med, lo, hi = _time(fn, copies)
                    st.copy_(keep)
                    rows_out.append({"part": "ops", "op": op, "state": name, "R": R, "V": V, "allowed": allowed,
                                     "vocab_bytes": nbytes, "us": round(med, 2), "min_us": round(lo, 2),
                                     "max_us": round(hi, 2), "x_argmax": round(med / base, 3)})
                    print(json.dumps(rows_out[-1]), flush=True)
            del bf
            torch.cuda.empty_cache()


def engine_part(rows_out, llm, batches, new=128):
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.engine.scheduler import ContinuousEngine
    from docqa_amd.models import checkpoint as ck
    from docqa_amd.text.tokenizer import ChatTokenizer

    model = ck.resolve_llama(llm, device="cuda", seed=0)
    eng = LLMEngine(model, max_batch=max(batches), max_context=512, use_graphs=True, prefix_cache=False)
    eng.set_vocab_bytes(ChatTokenizer(model_vocab=model.cfg.vocab_size).token_bytes(model.cfg.vocab_size))
    ce = ContinuousEngine(eng)
    g = torch.Generator().manual_seed(2)
    base = dict(max_new_tokens=new, stop_on_eos=False)
    sampled = dict(temperature=0.8, top_k=40, top_p=0.9)
    arms = {"greedy": lambda run: SamplingParams(**base),
            "greedy_logits": lambda run: SamplingParams(logprobs=True, top_logprobs=0, **base),
            "greedy_json": lambda run: SamplingParams(format="json", **base),
            "sampled": lambda run: SamplingParams(seed=3 + run, **sampled, **base),
            "sampled_json": lambda run: SamplingParams(seed=3 + run, format="json", **sampled, **base)}
    for B in batches:
        prompts = [torch.randint(3, model.cfg.vocab_size, (64,), generator=g).tolist() for _ in range(B)]
        for name, params in arms.items():
            ce.generate(prompts, params(0))                       # captures the flavour's graphs
        runs = {name: [] for name in arms}
        for run in range(RUNS):                                   # arms interleaved
            for name, params in arms.items():
                d0, s0 = eng.stats.decode_s, ce.steps
                ce.generate(prompts, params(run + 1))
                runs[name].append((eng.stats.decode_s - d0) * 1e3 / max(1, ce.steps - s0))
        ms = {name: statistics.median(v) for name, v in runs.items()}
        for name in arms:
            row = {"part": "engine", "llm": llm, "batch": B, "flavour": name, "new_tokens": new,
                   "ms_per_step": round(ms[name], 4), "min_ms": round(min(runs[name]), 4),
                   "max_ms": round(max(runs[name]), 4)}
            if name == "greedy_json":
                row["us_over_greedy_logits"] = round((ms[name] - ms["greedy_logits"]) * 1e3, 1)
                row["us_over_greedy"] = round((ms[name] - ms["greedy"]) * 1e3, 1)
            if name == "sampled_json":
                row["us_over_sampled"] = round((ms[name] - ms["sampled"]) * 1e3, 1)
            rows_out.append(row)
            print(json.dumps(row), flush=True)


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
    print("\n%-8s %-18s %-8s %7s %6s %12s" % ("part", "what", "state", "vocab", "rows", "median"))
    for r in rows:
        if r["part"] == "ops":
            print("%-8s %-18s %-8s %7d %6d %9.2f us  %s" % ("ops", r["op"], r["state"], r["V"], r["R"], r["us"],
                                                           "%.2fx argmax" % r["x_argmax"] if "x_argmax" in r else ""))
        else:
            print("%-8s %-18s %-8s %7s %6d %9.4f ms  [%.4f, %.4f]" % ("engine", r["flavour"], "", "", r["batch"],
                                                                      r["ms_per_step"], r["min_ms"], r["max_ms"]))


if __name__ == "__main__":
    main()
