"""Cost of a JSON-schema ``format``: the schema kernels (csrc/kernels/grammar_schema.hip) alone and
inside the continuous scheduler's decode step.

Operator part, bf16 logits of V = 128256 (Llama-3) and 32768 at R = 1 / 32 / 256 rows, the chat
tokenizer's bytes.  Two schemas: ``small`` (three properties: a free string, an enum, an integer)
and ``large`` (an enum and 70 properties of three types each, near the size cap of a table slot).
Four states: ``open`` (after ``{``: few tokens allowed, most die on the first-byte set), ``string``
(inside a free string: most tokens allowed, every byte of every token walked, two lookups a byte),
``enum`` (inside an enum literal) and ``done`` (no table, everything but EOS masked).  Every row in
the same state, once with all rows on one table slot and once with the rows spread over 8 slots
(8 schemas that differ in their key names).  ``ops.schema_mask`` (tables read through L2; the
A/B against a variant that staged tables of <= 60 KiB in LDS is recorded in
profiles/format_schema_bench.log, the variant is not kept), ``ops.schema_advance``, and beside them ``ops.grammar_mask`` in the comparable state of the JSON automaton and ``ops.argmax``
on the same logits.  Timing as in bench_format_json.py.

Engine part: Llama-3-8B random-init, ``ContinuousEngine.generate`` at batch 1, 32 and 256 for 128
tokens (fixed length), arms interleaved in one process: plain greedy, greedy "json", greedy on the
small schema, sampled, sampled "json", sampled on the small schema.  ms per decode step as in
bench_format_json.py.

python benchmarks/bench_format_schema.py [--part ops|engine|all] [--batches 1,32,256] [--llm llama3-8b]
-> one JSON line per measurement, then a table."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from benchmarks.bench_format_json import RUNS, VOCABS, _chat_vocab, _time  # noqa: E402
from docqa_amd import ops  # noqa: E402
from docqa_amd.ops import grammar as G  # noqa: E402
from docqa_amd.ops import json_schema as J  # noqa: E402

N_SLOTS = 8
N_LARGE = 70          # properties of the large schema beside its enum: 90 % of a slot's entries


def small_schema(tag: str = "") -> dict:
    return {"type": "object", "required": ["answer" + tag, "verdict" + tag, "score" + tag], "properties": {
        "answer" + tag: {"type": "string"}, "verdict" + tag: {"enum": ["oui", "non"]}, "score" + tag: {"type": "integer"}}}


def large_schema(tag: str = "") -> dict:
    props = {"verdict" + tag: {"enum": ["oui", "non"]}}
    props.update({f"k{tag}{i}": {"type": ["number", "string", "null"]} for i in range(N_LARGE)})
    return {"type": "object", "properties": props, "required": ["verdict" + tag] + [f"k{tag}{i}" for i in range(0, N_LARGE, 2)]}


def _state_docs(kind: str, tag: str) -> dict:
    if kind == "small":
        return {"open": b'{', "string": b'{"answer%s":"x' % tag.encode(),
                "enum": b'{"answer%s":"x","verdict%s":"o' % (tag.encode(), tag.encode()), "done": None}
    return {"open": b'{', "enum": b'{"verdict%s":"o' % tag.encode(),
            "string": b'{"verdict%s":"oui","k%s0":"x' % (tag.encode(), tag.encode()), "done": None}


GRAMMAR_STATES = {"open": b'{', "string": b'{"a":"x', "enum": b'{"a":"x","b":"o', "done": b'{"a":1}'}


def ops_part(rows_out):
    g = torch.Generator(device="cuda").manual_seed(1)
    table = G.table().cuda()
    pools = {}
    for kind, make in (("small", small_schema), ("large", large_schema)):
        pool = J.pool_new(N_SLOTS)
        css = [J.compile_schema(make("" if i == 0 else chr(ord("a") + i))) for i in range(N_SLOTS)]
        for i, cs in enumerate(css):
            J.pool_put(pool, i, cs)
        pools[kind] = (pool.cuda(), css)
        print(json.dumps({"part": "schema", "schema": kind, "n_states": css[0].n_states, "n_classes": css[0].n_classes,
                          "table_bytes": 2 * css[0].n_states * css[0].n_classes}), flush=True)
    for V in VOCABS:
        tb, eos, off, data = _chat_vocab(V)
        for R in (1, 32, 256):
            copies = min(16, max(2, (768 << 20) // (R * V * 2) + 1))
            bf = [(torch.randn(R, V, device="cuda", generator=g) * 3).bfloat16() for _ in range(copies)]
            base, _, _ = _time(lambda i: ops.argmax(bf[i]), copies)
            rows_out.append({"part": "ops", "op": "argmax", "schema": "-", "state": "-", "slots": 0, "R": R, "V": V,
                             "us": round(base, 2)})
            print(json.dumps(rows_out[-1]), flush=True)
            gm = {}
            for name, doc in GRAMMAR_STATES.items():
                st = torch.full((R,), G.walk(G.START_STATE, doc), dtype=torch.int64, device="cuda")
                gm[name], lo, hi = _time(lambda i: ops.grammar_mask(bf[i], V, st, off, data, table, eos), copies)
                rows_out.append({"part": "ops", "op": "grammar_mask", "schema": "json", "state": name, "slots": 0, "R": R,
                                 "V": V, "us": round(gm[name], 2), "min_us": round(lo, 2), "max_us": round(hi, 2),
                                 "x_argmax": round(gm[name] / base, 3)})
                print(json.dumps(rows_out[-1]), flush=True)
            for kind, (pool, css) in pools.items():
                for spread in (1, N_SLOTS):
                    if spread > 1 and R == 1:
                        continue
                    for name in ("open", "string", "enum", "done"):
                        words = []
                        for r in range(R):
                            slot = r % spread
                            doc = _state_docs(kind, "" if slot == 0 else chr(ord("a") + slot))[name]
                            w = J.pack(J.DONE, 0, slot) if doc is None else J.walk(css[slot], J.start_state(slot), doc)
                            assert w > 0
                            words.append(w)
                        st = torch.tensor(words, dtype=torch.int64, device="cuda")
                        allowed = sum(J.token_allowed(css[0], words[0], t, tb, eos) for t in range(len(tb))
                                      if tb[t] or t == eos)
                        nxt = torch.full((R,), next(t for t in range(len(tb)) if J.token_allowed(css[0], words[0], t, tb, eos)),
                                         dtype=torch.int64, device="cuda")
                        keep = st.clone()
                        arms = (("schema_mask", lambda i: ops.schema_mask(bf[i], V, st, off, data, pool, eos)),
                                ("schema_advance", lambda i: (st.copy_(keep), ops.schema_advance(st, nxt, off, data, pool, eos))))
                        for op, fn in arms:
                            med, lo, hi = _time(fn, copies)
                            st.copy_(keep)
                            rows_out.append({"part": "ops", "op": op, "schema": kind, "state": name, "slots": spread,
                                             "R": R, "V": V, "allowed": allowed, "us": round(med, 2),
                                             "min_us": round(lo, 2), "max_us": round(hi, 2),
                                             "x_argmax": round(med / base, 3),
                                             "x_grammar_mask": round(med / gm[name], 3)})
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
    schema = small_schema()
    arms = {"greedy": lambda run: SamplingParams(**base),
            "greedy_json": lambda run: SamplingParams(format="json", **base),
            "greedy_schema": lambda run: SamplingParams(format="json", json_schema=schema, **base),
            "sampled": lambda run: SamplingParams(seed=3 + run, **sampled, **base),
            "sampled_json": lambda run: SamplingParams(seed=3 + run, format="json", **sampled, **base),
            "sampled_schema": lambda run: SamplingParams(seed=3 + run, format="json", json_schema=schema, **sampled, **base)}
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
            kind = name.split("_")[0]
            if name.endswith("_schema"):
                row["us_over_json"] = round((ms[name] - ms[kind + "_json"]) * 1e3, 1)
            if "_" in name:
                row["us_over_" + kind] = round((ms[name] - ms[kind]) * 1e3, 1)
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
    print("\n%-7s %-16s %-6s %-7s %5s %7s %5s %12s" % ("part", "what", "schema", "state", "slots", "vocab", "rows", "median"))
    for r in rows:
        if r["part"] == "ops":
            print("%-7s %-16s %-6s %-7s %5d %7d %5d %9.2f us  %s" % (
                "ops", r["op"], r["schema"], r["state"], r["slots"], r["V"], r["R"], r["us"],
                ("%.2fx argmax" % r["x_argmax"] if "x_argmax" in r else "")
                + (", %.2fx grammar_mask" % r["x_grammar_mask"] if "x_grammar_mask" in r else "")))
        else:
            print("%-7s %-16s %-6s %-7s %5s %7s %5d %9.4f ms  [%.4f, %.4f]" % (
                "engine", r["flavour"], "", "", "", "", r["batch"], r["ms_per_step"], r["min_ms"], r["max_ms"]))


if __name__ == "__main__":
    main()
