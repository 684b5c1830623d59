"""Decode projections at 2..32 rows: the MXFP4-weight ring kernel (dgemm.hip dgemm4_kernel) against
the bf16 skinny kernel at its shipped plan (ops.decode_plan / glu_linear / dgemm_argmax_val), per
projection of Llama-3-8B, both LM heads (Llama-3-8B, Mistral-7B) and the llama3-1b-test preset
the suite runs (bench_dgemm_fp8.SHAPES), at M in {2, 4, 8, 16, 32}.  Weights are rotated past the
256 MB MALL (a decode step streams the whole model between two uses of a weight), every candidate
is warmed up, and the figure is the median of WINDOWS timed windows of ITERS launches each, the
bf16 launch, the FP8 ring kernel at its rule (for information: a model holds one streamed format,
so inside an MXFP4 model W' is the only alternative) and the MXFP4 candidates (every split count
the 2048-deep K granule allows, slabs at each tile height) taking turns window by window.  TB/s counts weight bytes only (2
per weight bf16, 1 FP8, 0.53125 MXFP4).

python benchmarks/bench_dgemm_mxfp4.py [--out FILE] [--only NAME,...]  -> one JSON line per
(projection, M, variant), then a table.  ``rule``: the MXFP4 variant the plan table names for the
pair (slabs: split count and 64 | 32 | 16 weight rows per workgroup), else ops.dgemm4_splits at 64 rows;
``wins``: its median is below the bf16 median and the two min..max window ranges do not overlap
-- the condition for a (shape, bucket) pair to be listed in the ops._DGEMM4_* plan tables;
``plan``: the tables list it (what a quantized model runs)."""
import argparse
import json
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from benchmarks.bench_dgemm_fp8 import ROWS, SHAPES, time_all  # noqa: E402
from docqa_amd import ops  # noqa: E402


def planned(kind, M, N, K):
    if kind == "slab":
        return bool(ops.dgemm4_plan(M, N, K)[0])
    return ops.dgemm4_glu_ok(M, N, K) if kind == "glu" else ops.dgemm4_argmax_ok(M, N, K)


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
        copies = max(2, (768 << 20) // (N * K // 2) + 1)    # MXFP4 bytes: every format rotates past the MALL
        g = torch.Generator(device="cuda").manual_seed(1)
        ws, q8, q4 = [], [], []
        for _ in range(copies):
            w = ((torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
            q, e = ops.quantize_mxfp4_rows(w)
            q4.append((q, e))
            ws.append(ops.dequantize_mxfp4_rows(q, e, torch.bfloat16))
            q8.append(ops.quantize_fp8_rows(ws[-1]))
            del w
        turns = K // ops.DGEMM4_K
        rule = ops.dgemm4_splits(N, K)
        S8 = ops.dgemm8_splits(N, K)
        for M in ROWS:
            x = (torch.rand(M, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
            cands = {}
            if kind == "slab":
                S, t = ops.decode_plan(M, N, K)
                cands[f"bf16_S{S}_t{t}"] = lambda i, S=S, t=t: nat.dgemm_partial(x, ws[i], S, t)
                cands[f"fp8_S{S8}"] = lambda i: nat.dgemm8_partial(x, q8[i][0], q8[i][1], S8, 64)
                for t4 in (64, 32, 16):
                    for S4 in [S4 for S4 in range(1, turns + 1) if turns % S4 == 0]:
                        if (N // t4) * S4 <= 1024:     # beyond four workgroups per CU nothing is left to fill
                            cands[f"mxfp4_S{S4}_t{t4}"] = (lambda i, S4=S4, t4=t4:
                                                           nat.dgemm4_partial(x, q4[i][0], q4[i][1], S4, t4))
                Sp, tp = ops.dgemm4_plan(M, N, K)
                rulename = f"mxfp4_S{Sp}_t{tp}" if Sp else f"mxfp4_S{rule}_t64"
            elif kind == "glu":
                cands["bf16_glu"] = lambda i: nat.dgemm_glu(x, ws[i])
                cands["fp8_glu"] = lambda i: nat.dgemm8_glu(x, q8[i][0], q8[i][1])
                cands["mxfp4_glu"] = lambda i: nat.dgemm4_glu(x, q4[i][0], q4[i][1])
                rulename = "mxfp4_glu"
            else:
                cands["bf16_argmax"] = lambda i: nat.dgemm_argmax_val(x, ws[i], N)
                cands["fp8_argmax"] = lambda i: nat.dgemm8_argmax_val(x, q8[i][0], q8[i][1], N)
                cands["mxfp4_argmax"] = lambda i: nat.dgemm4_argmax_val(x, q4[i][0], q4[i][1], N)
                rulename = "mxfp4_argmax"
            times = time_all(cands, copies)
            base = next(v for k, v in times.items() if k.startswith("bf16"))
            for k, (med, lo, hi) in times.items():
                nbytes = N * K * (2 if k.startswith("bf16") else 1 if k.startswith("fp8") else 17 / 32)
                is_rule = k == rulename
                rows.append({"proj": name, "N": N, "K": K, "M": M, "variant": k, "us": round(med, 2),
                             "min_us": round(lo, 2), "max_us": round(hi, 2), "TBps": round(nbytes / med / 1e6, 2),
                             "vs_bf16": round(base[0] / med, 2), "rule": is_rule,
                             "wins": bool(is_rule and med < base[0] and hi < base[1]),
                             "plan": bool(is_rule and planned(kind, M, N, K))})
                print(json.dumps(rows[-1]), flush=True)
        del ws, q8, q4
        torch.cuda.empty_cache()
    print("\n%-16s %3s %-14s %9s %9s %9s %7s %8s %5s %5s" % ("projection", "M", "variant", "us", "min", "max", "TB/s",
                                                              "vs bf16", "wins", "plan"))
    for r in rows:
        best = min((q for q in rows if (q["proj"], q["M"]) == (r["proj"], r["M"]) and q["variant"].startswith("mxfp4")),
                   key=lambda q: q["us"])
        if r["rule"] or r is best or not r["variant"].startswith("mxfp4"):
            print("%-16s %3d %-14s %9.2f %9.2f %9.2f %7.2f %8.2f %5s %5s"
                  % (r["proj"], r["M"], r["variant"], r["us"], r["min_us"], r["max_us"], r["TBps"], r["vs_bf16"],
                     "yes" if r["wins"] else "-", "yes" if r["plan"] else "-"))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
