"""Decode attention over an FP8 (e4m3) paged KV cache against the bf16 cache, per kernel:
the wave-parallel grouped split kernel (attn_decode.hip paged_decode_group_wave8_kernel vs
paged_decode_group_wave_kernel, the same split plan from block 0 and ticket merge) and the
per-row kernel (paged_decode_kernel<.., F8> vs what ops.paged_decode picks for bf16), at the
headline decode step's shape: batch 256, 8 KV heads, GQA 4, head_dim 128.

Length mix: an approximation of the headline workload's decode batch -- every row starts with
the 3 template blocks, clusters of rows share 4..8 blocks of retrieved chunks, then 3..7 own
blocks (prompts of ~650..1150 tokens, ~100k distinct tokens per layer: the ~13 GB of distinct
K/V per 32-layer step the README's roofline table counts).  The pool is replicated COPIES
times and the launches rotate through the copies, so every launch streams K/V that left the
256 MB MALL (one copy is ~2 x 200 MB in bf16).  Every candidate is warmed up; the figure is
the median of WINDOWS timed windows of ITERS launches, the candidates taking turns window by
window.  TB/s counts the distinct K/V bytes of the batch (2 per element bf16, 1 FP8).

python benchmarks/bench_kv_fp8.py [--out FILE] [--batch N]  -> one JSON line per candidate."""
import argparse
import json
import math
import random
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/benchmarks/", 1)[0])
from docqa_amd import ops  # noqa: E402

WINDOWS, ITERS, COPIES = 7, 12, 3
HKV, D, BS = 8, 128, 64


def headline_mix(B, seed=0):
    rnd = random.Random(seed)
    tables, lens = [], []
    nxt = 3
    while len(tables) < B:
        shared = list(range(nxt, nxt + rnd.randint(4, 8)))
        nxt += len(shared)
        for _ in range(min(rnd.choice([2, 3, 4, 6]), B - len(tables))):
            own = list(range(nxt, nxt + rnd.randint(3, 7)))
            nxt += len(own)
            t = [0, 1, 2] + shared + own
            tables.append(t)
            lens.append(64 * (len(t) - 1) + rnd.randint(1, 64))
    return tables, lens, nxt


def _window(fn, start):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for i in range(ITERS):
        fn((start + i) % COPIES)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / ITERS


def time_all(cands):
    for fn in cands.values():
        for i in range(COPIES):
            fn(i)
    torch.cuda.synchronize()
    t = {k: [] for k in cands}
    for w in range(WINDOWS):
        for k, fn in cands.items():
            t[k].append(_window(fn, w * ITERS))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    assert ops.load_native()
    B, Hq = a.batch, 4 * HKV
    tables, lens, nblk = headline_mix(B)
    maxb = max(len(t) for t in tables)
    bt = torch.tensor([t + [0] * (maxb - len(t)) for t in tables], dtype=torch.int32, device="cuda")
    cl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    distinct = len({b for t, L in zip(tables, lens) for b in t[:(L + BS - 1) // BS]}) * BS
    pools8, pools16 = [], []
    for c in range(COPIES):
        g = torch.Generator(device="cuda").manual_seed(c)
        k = torch.randn(nblk, HKV, BS, D, device="cuda", generator=g).to(ops.KV_FP8)
        v = torch.randn(nblk, HKV, BS, D, device="cuda", generator=g).to(ops.KV_FP8)
        pools8.append((k, v))
        pools16.append((k.to(torch.bfloat16), v.to(torch.bfloat16)))
    q = torch.randn(B, (Hq + 2 * HKV) * D, device="cuda", dtype=torch.bfloat16)
    scale = 1 / math.sqrt(D)
    quads = ops.pack_decode_groups(tables, lens, 0, BS, (B + 1) // 2)
    plan, used = None, 0
    for budget in (8, 12, 16, 24, 32, 40, 48, 64, 96, 128):     # the engine's auto budget (set_groups)
        p = ops.split_decode_groups(quads, tables, lens, 0, BS, B, budget)
        used = int((p[0, :, :4] >= 0).any(1).sum())
        if used <= 82:
            plan = p
            break
    plan = (plan if plan is not None else p).cuda()
    tick = ops.decode_ticket(plan.shape[1] * HKV, "cuda")
    pt = torch.zeros(maxb, dtype=torch.int32, device="cuda")
    plen = torch.zeros(1, dtype=torch.int32, device="cuda")

    def wave(pools):
        return lambda i: ops.paged_decode_cascade_grouped(q, pools[i][0], pools[i][1], bt, cl, Hq, scale, pt, plen,
                                                          4, plan, False, tick, True)

    def row(pools):
        return lambda i: ops.paged_decode(q, pools[i][0], pools[i][1], bt, cl, Hq, maxb * BS, scale)

    cands = {"wave_bf16": wave(pools16), "wave_fp8": wave(pools8), "row_bf16": row(pools16), "row_fp8": row(pools8)}
    d = (cands["wave_fp8"](0).float() - cands["wave_bf16"](0).float()).abs().max().item()
    d2 = (cands["row_fp8"](0).float() - cands["wave_fp8"](0).float()).abs().max().item()
    times = time_all(cands)
    rows = []
    for k, (med, lo, hi) in times.items():
        nbytes = 2 * distinct * HKV * D * (1 if k.endswith("fp8") else 2)
        base = times[k.split("_")[0] + "_bf16"][0]
        rows.append({"kernel": k, "B": B, "Hkv": HKV, "distinct_tokens": distinct, "plan_items": used,
                     "us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1),
                     "kv_TBps": round(nbytes / med / 1e6, 2), "vs_bf16": round(base / med, 2)})
        print(json.dumps(rows[-1]), flush=True)
    print(json.dumps({"check": "max |fp8 wave - bf16 wave on the image|", "value": d,
                      "row_vs_wave_fp8": d2}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
