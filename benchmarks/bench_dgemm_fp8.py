"""Decode projections at 2..32 rows: the FP8-weight ring kernel (dgemm.hip dgemm8_kernel) against
the bf16 skinny kernel at its shipped plan (ops.decode_plan / glu_linear / dgemm_argmax_val), per
projection of Llama-3-8B, both LM heads (Llama-3-8B, Mistral-7B) and the llama3-1b-test preset
the suite runs, at M in {2, 4, 8, 16, 32}.  Weights are rotated past the 256 MB MALL (a decode
step streams the whole model between two uses of a weight), every candidate is warmed up, and
the figure is the median of WINDOWS timed windows of ITERS launches each, the bf16 launch and the
FP8 candidates (every split count the K granule allows up to 16) taking turns window by window.
TB/s counts weight bytes only (2 per weight bf16, 1 FP8).

python benchmarks/bench_dgemm_fp8.py [--out FILE] [--only NAME,...]  -> one JSON line per
(projection, M, variant), then a table.  ``rule``: the FP8 variant ops.dgemm8_splits picks;
``wins``: its median is below the bf16 median and the two min..max window ranges do not overlap
-- the condition for a (shape, bucket) pair to be listed in the ops._DGEMM8_* plan tables;
``plan``: the tables list it (what a quantized model runs)."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

WINDOWS, ITERS = 9, 40
ROWS = (2, 4, 8, 16, 32)
# (name, N, K, kind): kind slab | glu | argmax
SHAPES = [("qkv", 6144, 4096, "slab"), ("o", 4096, 4096, "slab"), ("gate_up", 28672, 4096, "glu"),
          ("down", 4096, 14336, "slab"), ("lm_head_8b", 128256, 4096, "argmax"),
          ("lm_head_mistral", 32768, 4096, "argmax"),
          ("qkv_1b", 3072, 2048, "slab"), ("o_1b", 2048, 2048, "slab"), ("gate_up_1b", 16384, 2048, "glu"),
          ("down_1b", 2048, 8192, "slab"), ("lm_head_1b", 32000, 2048, "argmax")]


def _window(fn, copies, start):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(ITERS):
        fn((start + i) % copies)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def time_all(cands, copies):
    """{name: (median, min, max) us}: candidates take turns, one window each, WINDOWS rounds."""
    for fn in cands.values():
        for i in range(max(copies, 3)):
            fn(i % copies)
    torch.cuda.synchronize()
    t = {k: [] for k in cands}
    for w in range(WINDOWS):
        for k, fn in cands.items():
            t[k].append(_window(fn, copies, w * ITERS))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def planned(kind, M, N, K):
    if kind == "slab":
        return bool(ops.dgemm8_plan(M, N, K)[0])
    return ops.dgemm8_glu_ok(M, N, K) if kind == "glu" else ops.dgemm8_argmax_ok(M, N, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma list of projection names")
    a = ap.parse_args()
    assert ops.load_native()
    nat = torch.ops.docqa
    only = {n for n in a.only.split(",") if n}
    rows = []
    for name, N, K, kind in SHAPES:
        if only and name not in only:
            continue
        copies = max(2, (768 << 20) // (N * K) + 1)       # FP8 bytes: both formats rotate past the MALL
        g = torch.Generator(device="cuda").manual_seed(1)
        ws, qs = [], []
        for _ in range(copies):
            w = ((torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
            q, s = ops.quantize_fp8_rows(w)
            ws.append(ops.dequantize_fp8_rows(q, s, torch.bfloat16))
            qs.append((q, s))
            del w
        turns = K // ops.DGEMM8_K
        rule = ops.dgemm8_splits(N, K)
        for M in ROWS:
            x = (torch.rand(M, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
            cands = {}
            if kind == "slab":
                S, t = ops.decode_plan(M, N, K)
                cands[f"bf16_S{S}_t{t}"] = lambda i, S=S, t=t: nat.dgemm_partial(x, ws[i], S, t)
                for S8 in [S8 for S8 in range(1, min(turns, 16) + 1) if turns % S8 == 0]:
                    cands[f"fp8_S{S8}"] = lambda i, S8=S8: nat.dgemm8_partial(x, qs[i][0], qs[i][1], S8, 64)
                rulename = f"fp8_S{rule}"
            elif kind == "glu":
                cands["bf16_glu"] = lambda i: nat.dgemm_glu(x, ws[i])
                cands["fp8_glu"] = lambda i: nat.dgemm8_glu(x, qs[i][0], qs[i][1])
                rulename = "fp8_glu"
            else:
                cands["bf16_argmax"] = lambda i: nat.dgemm_argmax_val(x, ws[i], N)
                cands["fp8_argmax"] = lambda i: nat.dgemm8_argmax_val(x, qs[i][0], qs[i][1], N)
                rulename = "fp8_argmax"
            times = time_all(cands, copies)
            base = next(v for k, v in times.items() if k.startswith("bf16"))
            for k, (med, lo, hi) in times.items():
                nbytes = N * K * (2 if k.startswith("bf16") else 1)
                is_rule = k == rulename
                rows.append({"proj": name, "N": N, "K": K, "M": M, "variant": k, "us": round(med, 2),
                             "min_us": round(lo, 2), "max_us": round(hi, 2), "TBps": round(nbytes / med / 1e6, 2),
                             "vs_bf16": round(base[0] / med, 2), "rule": is_rule,
                             "wins": bool(is_rule and med < base[0] and hi < base[1]),
                             "plan": bool(is_rule and planned(kind, M, N, K))})
                print(json.dumps(rows[-1]), flush=True)
        del ws, qs
        torch.cuda.empty_cache()
    print("\n%-16s %3s %-14s %9s %9s %9s %7s %8s %5s %5s" % ("projection", "M", "variant", "us", "min", "max", "TB/s",
                                                              "vs bf16", "wins", "plan"))
    for r in rows:
        if r["rule"] or r["variant"].startswith("bf16"):
            print("%-16s %3d %-14s %9.2f %9.2f %9.2f %7.2f %8.2f %5s %5s"
                  % (r["proj"], r["M"], r["variant"], r["us"], r["min_us"], r["max_us"], r["TBps"], r["vs_bf16"],
                     "yes" if r["wins"] else "-", "yes" if r["plan"] else "-"))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
