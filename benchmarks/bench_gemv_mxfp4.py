"""Batch-1 decode projections: the MXFP4-weight GEMV (dgemm.hip gemv4_kernel) against the bf16
GEMV and the FP8-weight GEMV at their shipped plans, per projection of Llama-3-8B / Mistral-7B
(and of the llama3-1b-test preset the GPU tests decode), as a decode step runs them: QKV and
gate|up with the in-kernel input row (XN), O / down as split-K slabs, the LM head with the fused
argmax.  Weights are rotated past the 256 MB MALL (a decode step streams gigabytes between two
uses of a weight), every candidate is warmed up, and the figure is the median of WINDOWS timed
windows of ITERS launches each, the candidates of a projection taking turns window by window.
TB/s counts weight bytes only (2 per weight bf16, 1 FP8, 17 / 32 MXFP4 with its scales).

python benchmarks/bench_gemv_mxfp4.py [--out FILE]  -> one JSON line per (projection, variant),
then the table of the shipped plans.  ``plan: true`` marks what ops.gemv4_plan / gemv4_glu_ok
ship; ``wins: true`` marks an MXFP4 variant whose whole min..max window range lies below both the
bf16 and the FP8 arm's -- only such a variant belongs in the plan tables."""
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
          ("lm_head_mistral", 32768, 4096, "argmax"),
          ("1b_qkv_xn", 3072, 2048, "slab_xn"), ("1b_o", 2048, 2048, "slab"), ("1b_gate_up_xn", 16384, 2048, "glu_xn"),
          ("1b_down", 2048, 8192, "slab"), ("1b_lm_head", 32000, 2048, "argmax")]


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


def mx4_variants(N, K, kind):
    """(S, R, lb, kw) of every instantiation that takes this shape."""
    out = []
    if kind == "slab":
        cases, splits = ops.GEMV4_CASES, (1, 2)
    elif kind == "slab_xn":
        cases, splits = ops.GEMV4_XN_CASES, (1,)
    else:
        cases, splits = ops.GEMV4_EPI_CASES, (1,)
    for S in splits:
        for R, C, lb, kw in cases:
            if K % S == 0 and K // S == C * 64 * lb * kw and N % R == 0:
                out.append((S, R, lb, kw))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert ops.load_native()
    nat = torch.ops.docqa
    rows = []
    for name, N, K, kind in SHAPES:
        copies = max(2, (768 << 20) // (N * K // 2) + 1)      # MXFP4 bytes: every format rotates past the MALL
        g = torch.Generator(device="cuda").manual_seed(1)
        ws, q8, q4 = [], [], []
        for _ in range(copies):
            w = ((torch.rand(N, K, device="cuda", generator=g) * 2 - 1) / K ** 0.5).to(torch.bfloat16)
            q, e = ops.quantize_mxfp4_rows(w)
            w = ops.dequantize_mxfp4_rows(q, e, torch.bfloat16)   # every arm multiplies the same W'
            ws.append(w)
            q4.append((q, e))
            q8.append(ops.quantize_fp8_rows(w))                   # the FP8 arm's bytes (timing only)
            del w
        x = (torch.rand(1, K, device="cuda", generator=g) * 2 - 1).to(torch.bfloat16)
        Pin = torch.randn(1, 1, K, device="cuda", generator=g)
        res = torch.randn(1, K, device="cuda", generator=g).to(torch.bfloat16)
        res2 = torch.empty_like(res)
        gamma = torch.ones(K, device="cuda", dtype=torch.bfloat16)
        cands, plan = {}, None
        p8 = ops.gemv8_plan(1, N, K)
        l8 = ops.gemv8_lb(K, p8[0]) if p8[0] else 0
        if kind in ("slab", "slab_xn"):
            S, R = ops.gemv_plan(1, N, K)
            p4 = ops.gemv4_plan(1, N, K)
            plan = (p4[0], p4[1], *ops.gemv4_cfg(N, K, p4[0])) if p4[0] else None
        else:
            ok4 = ops.gemv4_glu_ok(1, N, K) if kind == "glu_xn" else ops.gemv4_argmax_ok(1, N, K)
            plan = (1, *ops._GEMV4_EPI[K]) if ok4 else None
        if kind == "slab":
            if S:
                cands[f"bf16_S{S}_R{R}"] = lambda i, S=S, R=R: nat.gemv(x, ws[i], S, R, False)
            if p8[0]:
                cands["fp8_S%d_R%d_L%d" % (*p8, l8)] = lambda i: nat.gemv8(x, q8[i][0], q8[i][1], p8[0], p8[1], l8, False)
            mk = lambda S, R, lb, kw: (lambda i: nat.gemv4(x, q4[i][0], q4[i][1], S, R, lb, kw, False))  # noqa: E731
        elif kind == "slab_xn":
            if S:
                cands[f"bf16_S{S}_R{R}"] = lambda i, S=S, R=R: nat.gemv_xn(Pin, res, res2, gamma, 1e-5, ws[i], S, R,
                                                                           False)
            if p8[0]:
                cands["fp8_S%d_R%d_L%d" % (*p8, l8)] = lambda i: nat.gemv8_xn(Pin, res, res2, gamma, 1e-5, q8[i][0],
                                                                              q8[i][1], p8[0], p8[1], l8, False)
            mk = lambda S, R, lb, kw: (lambda i: nat.gemv4_xn(Pin, res, res2, gamma, 1e-5, q4[i][0], q4[i][1], S, R,  # noqa: E731
                                                              lb, kw, False))
        elif kind == "glu_xn":
            cands["bf16_R16"] = lambda i: nat.gemv_xn(Pin, res, res2, gamma, 1e-5, ws[i], 1, 16, True)
            if ops.gemv8_glu_ok(1, N, K):
                R8, L8 = ops._GEMV8_EPI[K]
                cands[f"fp8_S1_R{R8}_L{L8}"] = lambda i: nat.gemv8_xn(Pin, res, res2, gamma, 1e-5, q8[i][0], q8[i][1],
                                                                      1, R8, L8, True)
            mk = lambda S, R, lb, kw: (lambda i: nat.gemv4_xn(Pin, res, res2, gamma, 1e-5, q4[i][0], q4[i][1], 1, R,  # noqa: E731
                                                              lb, kw, True))
        else:
            cands["bf16_R16"] = lambda i: nat.gemv_argmax_val(x, ws[i], N)
            if ops.gemv8_argmax_ok(1, N, K):
                R8, L8 = ops._GEMV8_EPI[K]
                cands[f"fp8_S1_R{R8}_L{L8}"] = lambda i: nat.gemv8_argmax_val(x, q8[i][0], q8[i][1], N, R8, L8)
            mk = lambda S, R, lb, kw: (lambda i: nat.gemv4_argmax_val(x, q4[i][0], q4[i][1], N, R, lb, kw))  # noqa: E731
        for v in mx4_variants(N, K, kind):
            cands["mxfp4_S%d_R%d_L%d_W%d" % v] = mk(*v)
        planname = "mxfp4_S%d_R%d_L%d_W%d" % plan if plan else None
        times = time_all(cands, copies)
        base = [v for k, v in times.items() if not k.startswith("mxfp4")]
        bf = next((v[0] for k, v in times.items() if k.startswith("bf16")), float("nan"))
        f8 = next((v[0] for k, v in times.items() if k.startswith("fp8")), float("nan"))
        for k, (med, lo, hi) in times.items():
            per = 2.0 if k.startswith("bf16") else 1.0 if k.startswith("fp8") else 17 / 32
            wins = k.startswith("mxfp4") and all(hi < b[1] for b in base)
            rows.append({"proj": name, "N": N, "K": K, "variant": k, "us": round(med, 2), "min_us": round(lo, 2),
                         "max_us": round(hi, 2), "TBps": round(N * K * per / med / 1e6, 2),
                         "vs_bf16": round(bf / med, 2), "vs_fp8": round(f8 / med, 2), "wins": wins,
                         "plan": k == planname})
            print(json.dumps(rows[-1]), flush=True)
        del ws, q8, q4
        torch.cuda.empty_cache()
    print("\n%-16s %-20s %9s %7s %8s %7s" % ("projection", "variant", "us", "TB/s", "vs bf16", "vs fp8"))
    for r in rows:
        if r["plan"] or not r["variant"].startswith("mxfp4"):
            print("%-16s %-20s %9.2f %7.2f %8.2f %7.2f" % (r["proj"], r["variant"], r["us"], r["TBps"], r["vs_bf16"],
                                                          r["vs_fp8"]))
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
