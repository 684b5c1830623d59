"""Decode projections at 33..128 rows: the wide FP8-weight kernel (dgemm.hip dgemm8w_kernel) against
the shipped bf16 plan -- what LlamaModel._step_plan picks with the option off: ops.mid_plan /
ops.decode_plan for the slab projections, ops.glu_split16 / mgemm_glu / glu_linear for gate|up, the
mid-M LM head + argmax (ops.lm_head_argmax) -- per projection of Llama-3-8B / Mistral-7B and both
LM heads, at M = 64 and 128 (the buckets) and 33 and 65 (the first row of each instantiation, as
information).  Weights are rotated past the 256 MB MALL, every candidate is warmed up, and the
figure is the median of WINDOWS timed windows of ITERS launches each, the candidates taking turns
window by window.  Every slab projection is timed alone and together with its consumer
(add_rmsnorm_splitk for O / down, rope_cache_splitk for QKV): the slab bytes differ with the split
count, and at 128 rows they are not small.  TB/s counts weight bytes only.

python benchmarks/bench_dgemm_fp8_wide.py [--out FILE] [--only NAME,...]  -> one JSON line per
(projection, M, variant), then a table.  ``wins``: the FP8 variant's median is below the bf16
plan's and the two min..max window ranges do not overlap -- judged with the consumer where the
variant's split count differs from the bf16 plan's, alone otherwise.  A (shape, bucket) pair goes
into the ops._DGEMM8W_* tables only if the same variant wins in two runs.  ``plan``: the tables
list this variant."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

WINDOWS, ITERS = 9, 40
ROWS = (64, 128, 33, 65)
EPS = 1e-5
HQ, HKV, D = 32, 8, 128       # the QKV shape's heads (Llama-3-8B / Mistral-7B)
# (name, N, K, kind): kind slab | glu | argmax; slab consumers: rope (QKV) | norm (O, down)
SHAPES = [("qkv", 6144, 4096, "slab"), ("o", 4096, 4096, "slab"), ("gate_up", 28672, 4096, "glu"),
          ("down", 4096, 14336, "slab"), ("lm_head_8b", 128256, 4096, "argmax"),
          ("lm_head_mistral", 32768, 4096, "argmax")]


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


def bf16_slab(M, N, K, qkv):
    """(label, split count, launch) of the bf16 plan of a slab projection, as _step_plan at TP = 1."""
    S, c = ops.mid_plan(M, N, K)
    if S:
        b16 = bool(ops.SLAB_BF16 and S > 1)
        if S == 1:
            return f"bf16_mgemm_S1_c{c}", 1, lambda x, w: ops.mgemm_partial(x, w, 1, c).float()[None]
        return f"bf16_mgemm_S{S}_c{c}", S, lambda x, w: ops.mgemm_partial(x, w, S, c, bf16=b16)
    S, t = ops.decode_plan(M, N, K)
    return f"bf16_dgemm_S{S}_t{t}", S, lambda x, w: ops.dgemm_partial(x, w, S, t)


def bf16_glu(M, N, K):
    S, c = ops.glu_split16_plan(M, N, K) if ops.SLAB_BF16 else (0, 0)
    if S:
        return "bf16_glu_split16", lambda x, w: ops.glu_split16(x, w, S, c)
    Sg, cg = ops.mid_plan(M, N, K, glu=True)
    if Sg:
        return "bf16_mgemm_glu", lambda x, w: ops.mgemm_glu(x, w, cg)
    return "bf16_glu_linear", lambda x, w: ops.glu_linear(x, w)


def fp8_splits(N, K):
    turns = K // ops.DGEMM8W_K
    return [S for S in range(1, turns + 1) if turns % S == 0 and S <= 16 and (N // ops.DGEMM8W_TILE) * S <= 1024]


def planned(kind, M, N, K, S=0):
    if kind == "slab":
        return ops.dgemm8w_plan(M, N, K)[0] == S and S > 0
    return ops.dgemm8w_glu_ok(M, N, K) if kind == "glu" else ops.dgemm8w_argmax_ok(M, N, K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="comma list of projection names")
    a = ap.parse_args()
    assert ops.load_native()
    nat = torch.ops.docqa
    only = {n for n in a.only.split(",") if n}
    rows = []
    dev = "cuda"
    cos_sin = ops.rope_cos_sin(4096, D, 500000.0, torch.device(dev))
    for name, N, K, kind in SHAPES:
        if only and name not in only:
            continue
        copies = max(2, (768 << 20) // (N * K) + 1)       # FP8 bytes: both formats rotate past the MALL
        g = torch.Generator(device=dev).manual_seed(1)
        ws, qs = [], []
        for _ in range(copies):
            w = ((torch.rand(N, K, device=dev, generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
            q, s = ops.quantize_fp8_rows(w)
            ws.append(ops.dequantize_fp8_rows(q, s, torch.bfloat16))
            qs.append((q, s))
            del w
        for M in ROWS:
            x = (torch.rand(M, K, device=dev, generator=g) * 2 - 1).to(torch.bfloat16)
            cands, judged = {}, {}
            if kind == "slab":
                qkv = name == "qkv"
                residual = torch.zeros(M, N, device=dev, dtype=torch.bfloat16)
                gamma = torch.ones(N, device=dev, dtype=torch.bfloat16)
                pos = torch.arange(M, device=dev, dtype=torch.int32)

                def consume(P):
                    if qkv:
                        return ops.rope_cache_splitk(P, pos, cos_sin, None, None, None, HQ, HKV, D)
                    return ops.add_rmsnorm_splitk(P, residual, gamma, EPS)

                base, Sb, fb = bf16_slab(M, N, K, qkv)
                cands[base] = lambda i, fb=fb: fb(x, ws[i])
                cands[base + "+c"] = lambda i, fb=fb: consume(fb(x, ws[i]))
                for S8 in fp8_splits(N, K):
                    f8 = lambda i, S8=S8: nat.dgemm8w_partial(x, qs[i][0], qs[i][1], S8, ops.DGEMM8W_TILE)  # noqa: E731
                    cands[f"fp8w_S{S8}"] = f8
                    cands[f"fp8w_S{S8}+c"] = lambda i, f8=f8: consume(f8(i))
                    judged[f"fp8w_S{S8}"] = S8 == Sb        # same split: judged alone
                    judged[f"fp8w_S{S8}+c"] = S8 != Sb      # other split: judged with the consumer
            elif kind == "glu":
                base, fb = bf16_glu(M, N, K)
                cands[base] = lambda i, fb=fb: fb(x, ws[i])
                cands["fp8w_glu"] = lambda i: nat.dgemm8w_glu(x, qs[i][0], qs[i][1])
                judged["fp8w_glu"] = True
            else:
                base = "bf16_lm_head_argmax"
                cands[base] = lambda i: ops.lm_head_argmax(x, ws[i], N)
                cands["fp8w_argmax"] = lambda i: nat.dgemm8w_argmax_val(x, qs[i][0], qs[i][1], N)
                judged["fp8w_argmax"] = True
            times = time_all(cands, copies)
            for k, (med, lo, hi) in times.items():
                ref_t = times[base + "+c"] if k.endswith("+c") else times[base]
                nbytes = N * K * (2 if k.startswith("bf16") else 1)
                S8 = int(k.split("_S")[1].split("+")[0]) if k.startswith("fp8w_S") else 0
                rows.append({"proj": name, "N": N, "K": K, "M": M, "variant": k, "us": round(med, 2),
                             "min_us": round(lo, 2), "max_us": round(hi, 2), "TBps": round(nbytes / med / 1e6, 2),
                             "vs_bf16": round(ref_t[0] / med, 2), "judged": bool(judged.get(k, False)),
                             "wins": bool(judged.get(k, False) and med < ref_t[0] and hi < ref_t[1]),
                             "plan": bool(k.startswith("fp8w") and planned(kind, M, N, K, S8))})
                print(json.dumps(rows[-1]), flush=True)
        del ws, qs
        torch.cuda.empty_cache()
    print("\n%-16s %3s %-22s %9s %9s %9s %7s %8s %6s %5s %5s" % ("projection", "M", "variant", "us", "min", "max",
                                                                 "TB/s", "vs bf16", "judged", "wins", "plan"))
    for r in rows:
        print("%-16s %3d %-22s %9.2f %9.2f %9.2f %7.2f %8.2f %6s %5s %5s"
              % (r["proj"], r["M"], r["variant"], r["us"], r["min_us"], r["max_us"], r["TBps"], r["vs_bf16"],
                 "yes" if r["judged"] else "-", "yes" if r["wins"] else "-", "yes" if r["plan"] else "-"))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
