"""Batch-1 decode projections: the FP8-weight GEMV (dgemm.hip gemv8_kernel) against the bf16
GEMV at its shipped plan, per projection of Llama-3-8B / Mistral-7B, as a decode step runs
them: QKV and gate|up with the in-kernel input row (XN), O / down as split-K slabs, the LM head
with the fused argmax.  Weights are rotated past the 256 MB MALL (a decode step streams 15 GB
between two uses of a weight), every candidate is warmed up, and the figure is the median of
WINDOWS timed windows of ITERS launches each, the bf16 and FP8 candidates of a projection
taking turns window by window.  TB/s counts weight bytes only (2 per weight bf16, 1 FP8).

python benchmarks/bench_gemv_fp8.py [--out FILE]  -> one JSON line per (projection, variant),
then the table of the plan entries.  ``plan: true`` marks what ops.gemv8_plan / gemv8_glu_ok
ship; an FP8 entry that is not faster than its bf16 row belongs out of the plan tables."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

WINDOWS, ITERS = 9, 40
# (name, N, K, kind): kind slab | slab_xn | glu_xn | argmax
SHAPES = [("qkv_xn", 6144, 4096, "slab_xn"), ("o", 4096, 4096, "slab"), ("gate_up_xn", 28672, 4096, "glu_xn"),
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
    """{name: median us}: candidates take turns, one window each, WINDOWS rounds."""
    for fn in cands.values():
        for i in range(max(copies, 3)):
            fn(i % copies)
    torch.cuda.synchronize()
    t = {k: [] for k in cands}
    for w in range(WINDOWS):
        for k, fn in cands.items():
            t[k].append(_window(fn, copies, w * ITERS))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def fp8_variants(N, K, kind):
    """(S, R, lb) of every instantiation that takes this shape."""
    out = []
    if kind == "slab":
        cases, splits = ops.GEMV8_CASES, (1, 2, 7)
    elif kind == "slab_xn":
        cases, splits = ops.GEMV8_XN_CASES, (1,)
    else:
        cases, splits = ops.GEMV8_EPI_CASES, (1,)
    for S in splits:
        for R, C, lb in cases:
            if K % S == 0 and K // S == C * 256 * lb and N % R == 0:
                out.append((S, R, lb))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert ops.load_native()
    nat = torch.ops.docqa
    rows = []
    for name, N, K, kind in SHAPES:
        copies = max(2, (768 << 20) // (N * K) + 1)       # FP8 bytes: both formats rotate past the MALL
        g = torch.Generator(device="cuda").manual_seed(1)
        ws, qs = [], []
        for _ in range(copies):
            w = ((torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
            q, s = ops.quantize_fp8_rows(w)
            ws.append(ops.dequantize_fp8_rows(q, s, torch.bfloat16))
            qs.append((q, s))
            del w
        x = (torch.rand(1, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        Pin = torch.randn(1, 1, K, device="cuda", generator=g)
        res = torch.randn(1, K, device="cuda", generator=g).to(torch.bfloat16)
        res2 = torch.empty_like(res)
        gamma = torch.ones(K, device="cuda", dtype=torch.bfloat16)
        cands, plan = {}, None
        if kind == "slab":
            S, R = ops.gemv_plan(1, N, K)
            cands[f"bf16_S{S}_R{R}"] = lambda i, S=S, R=R: nat.gemv(x, ws[i], S, R, False)
            p8 = ops.gemv8_plan(1, N, K)
            plan = (p8[0], p8[1], ops.gemv8_lb(K, p8[0])) if p8[0] else None
            mk = lambda S, R, lb: (lambda i: nat.gemv8(x, qs[i][0], qs[i][1], S, R, lb, False))  # noqa: E731
        elif kind == "slab_xn":
            S, R = ops.gemv_plan(1, N, K)
            cands[f"bf16_S{S}_R{R}"] = lambda i, S=S, R=R: nat.gemv_xn(Pin, res, res2, gamma, 1e-5, ws[i], S, R, False)
            p8 = ops.gemv8_plan(1, N, K)
            plan = (p8[0], p8[1], ops.gemv8_lb(K, p8[0])) if p8[0] else None
            mk = lambda S, R, lb: (lambda i: nat.gemv8_xn(Pin, res, res2, gamma, 1e-5, qs[i][0], qs[i][1], S, R, lb,  # noqa: E731
                                                          False))
        elif kind == "glu_xn":
            cands["bf16_R16"] = lambda i: nat.gemv_xn(Pin, res, res2, gamma, 1e-5, ws[i], 1, 16, True)
            plan = (1, *ops._GEMV8_EPI[K]) if ops.gemv8_glu_ok(1, N, K) else None
            mk = lambda S, R, lb: (lambda i: nat.gemv8_xn(Pin, res, res2, gamma, 1e-5, qs[i][0], qs[i][1], 1, R, lb,  # noqa: E731
                                                          True))
        else:
            cands["bf16_R16"] = lambda i: nat.gemv_argmax_val(x, ws[i], N)
            plan = (1, *ops._GEMV8_EPI[K]) if ops.gemv8_argmax_ok(1, N, K) else None
            mk = lambda S, R, lb: (lambda i: nat.gemv8_argmax_val(x, qs[i][0], qs[i][1], N, R, lb))  # noqa: E731
        for v in fp8_variants(N, K, kind):
            cands["fp8_S%d_R%d_L%d" % v] = mk(*v)
        planname = "fp8_S%d_R%d_L%d" % plan if plan else None
        times = time_all(cands, copies)
        base = next(v[0] for k, v in times.items() if k.startswith("bf16"))
        for k, (med, lo, hi) in times.items():
            nbytes = N * K * (2 if k.startswith("bf16") else 1)
            rows.append({"proj": name, "N": N, "K": K, "variant": k, "us": round(med, 2), "min_us": round(lo, 2),
                         "max_us": round(hi, 2), "TBps": round(nbytes / med / 1e6, 2),
                         "vs_bf16": round(base / med, 2), "plan": k == planname})
            print(json.dumps(rows[-1]), flush=True)
        del ws, qs
        torch.cuda.empty_cache()
    print("\n%-16s %-16s %9s %7s %8s" % ("projection", "variant", "us", "TB/s", "vs bf16"))
    for r in rows:
        if r["plan"] or r["variant"].startswith("bf16"):
            print("%-16s %-16s %9.2f %7.2f %8.2f" % (r["proj"], r["variant"], r["us"], r["TBps"], r["vs_bf16"]))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
