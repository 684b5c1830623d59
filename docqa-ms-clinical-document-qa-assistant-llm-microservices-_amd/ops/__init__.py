"""Operator dispatch: GPU tensors -> hand-written gfx950 HIP kernels (torch.ops.docqa.*),
CPU tensors -> the fp32 PyTorch reference in :mod:`docqa_amd.ops.reference`.

The native library is built in-tree by :mod:`docqa_amd.ops.build` into
``ops/_docqa_C.so``.  On a GPU tensor there is deliberately NO silent fallback: if the
extension is missing the op raises, so a GPU run can never pass on eager PyTorch by
accident.  Set ``DOCQA_FORCE_REFERENCE=1`` to route GPU tensors through the reference
(numerics debugging only).
"""
from __future__ import annotations

import os
import threading
from pathlib import Path
from typing import Callable, NamedTuple

import torch

from . import reference as ref

# DOCQA_NATIVE_LIB: load another build of the extension (same-box A/B of two kernel builds)
_LIB_PATH = Path(os.environ.get("DOCQA_NATIVE_LIB") or Path(__file__).resolve().parent / "_docqa_C.so")
_lock = threading.Lock()
_loaded = False
_load_error: str | None = None
_FORCE_REF = os.environ.get("DOCQA_FORCE_REFERENCE", "0") == "1"


def library_path() -> Path:
    return _LIB_PATH


def load_native(build_if_missing: bool = False) -> bool:
    """Load ``_docqa_C.so`` (optionally building it first). Returns True on success."""
    global _loaded, _load_error
    if _loaded:
        return True
    with _lock:
        if _loaded:
            return True
        if not _LIB_PATH.exists() and build_if_missing:
            from .build import build

            build(verbose=False)
        if not _LIB_PATH.exists():
            _load_error = f"native library not built: {_LIB_PATH} (run python -m docqa_amd.ops.build)"
            return False
        try:
            torch.ops.load_library(str(_LIB_PATH))
            _loaded = True
        except Exception as e:  # pragma: no cover - surfaced by native()
            _load_error = f"failed to load {_LIB_PATH}: {e}"
        return _loaded


def native_loaded() -> bool:
    return _loaded


def _native():
    if not _loaded and not load_native():
        raise RuntimeError(f"docqa native kernels unavailable on a GPU tensor: {_load_error}")
    return torch.ops.docqa


def _gpu(t: torch.Tensor) -> bool:
    return t.is_cuda and not _FORCE_REF


class use_reference:
    """Context manager: route GPU tensors through the PyTorch reference (model-level
    numerics tests compare a whole forward on native vs reference ops)."""

    def __enter__(self):
        global _FORCE_REF
        self._prev = _FORCE_REF
        _FORCE_REF = True
        return self

    def __exit__(self, *exc):
        global _FORCE_REF
        _FORCE_REF = self._prev
        return False


# ----------------------------------------------------------------------------- norms
def rmsnorm(x, w, eps: float):
    if _gpu(x):
        return _native().rmsnorm(x.contiguous(), w, eps)
    return ref.rmsnorm(x, w, eps)


def add_rmsnorm(x, residual, w, eps: float):
    """residual <- residual + x (in place, bf16); returns rmsnorm(residual) * w."""
    if _gpu(x):
        return _native().add_rmsnorm(x.contiguous(), residual, w, eps)
    return ref.add_rmsnorm(x, residual, w, eps)


def layernorm(x, residual, gamma, beta, eps: float):
    if _gpu(x):
        return _native().layernorm(x.contiguous(), residual, gamma, beta, eps)
    return ref.layernorm(x, residual, gamma, beta, eps)


# ----------------------------------------------------------------------------- rope / kv
def rope_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D):
    if _gpu(qkv):
        if slot_mapping is None:
            k_cache = v_cache = qkv  # unused placeholders
        _native().rope_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)
        return
    ref.rope_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)


rope_cos_sin = ref.rope_cos_sin


# ----------------------------------------------------------------------------- activations
def silu_mul(gu, interleaved: bool = False):
    if _gpu(gu):
        return _native().silu_mul(gu.contiguous(), interleaved)
    return ref.silu_mul(gu, interleaved)


glu_interleave, glu_split = ref.glu_interleave, ref.glu_split


def glu_linear(x, w_il):
    """silu(x Wg^T) * (x Wu^T) for 8-interleaved gate|up weights at <= 128 decode rows: the
    skinny fused-SwiGLU decode GEMM (dgemm.hip); 129..512 rows take the mid-M kernel
    (:func:`mid_plan`), so no decode bucket runs the library GEMM.  Measured vs hipBLASLt +
    silu_mul at M = 64 / 96 / 128: 50.9 / 60.0 / 63.1 us vs 56.4 / 57.6 / 59.7
    (profiles/r4_lm_head_probe.log)."""
    if _gpu(x):
        N, K = w_il.shape
        if x.numel() // K <= 128 and N % 64 == 0 and K % 512 == 0:
            return _native().dgemm_glu(x.contiguous(), w_il)
    return silu_mul(torch.nn.functional.linear(x, w_il), interleaved=True)


def bias_act(x, bias, residual=None, gelu: bool = False):
    if _gpu(x):
        return _native().bias_act(x.contiguous(), bias, residual, gelu)
    return ref.bias_act(x, bias, residual, gelu)


# ----------------------------------------------------------------------------- fused GEMM
EPI_NONE, EPI_BIAS, EPI_BIAS_GELU, EPI_BIAS_RES, EPI_GLU = 0, 1, 2, 3, 4


def linear_fused(x, w, bias=None, residual=None, epi: int = EPI_BIAS):
    """act(x @ w^T + bias) (+ residual) on the hand-written MFMA GEMM (N % 128 == 0,
    K % 64 == 0); other shapes fall back to hipBLASLt + the element-wise kernel."""
    if _gpu(x):
        N, K = w.shape
        if N % 128 == 0 and K % 64 == 0:
            return _native().gemm(x.contiguous(), w, bias, residual, epi)
        y = torch.nn.functional.linear(x, w)
        if epi == EPI_NONE:
            return y
        return bias_act(y, bias, residual if epi == EPI_BIAS_RES else None, epi == EPI_BIAS_GELU)
    return ref.linear_fused(x, w, bias, residual, epi)


def _splits_for(N: int, K: int, tile: int, min_wgs: int = 192) -> int:
    """Smallest split-K count giving >= ``min_wgs`` workgroups of ``tile`` weight rows
    (whole 512-deep ring turns per slice)."""
    tiles, S = N // tile, 1
    while tiles * S < min_wgs and K % (2 * S) == 0 and (K // (2 * S)) % 512 == 0:
        S *= 2
    return S if K % S == 0 and (K // S) % 512 == 0 else 0


def decode_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the skinny decode GEMM
    (csrc/kernels/dgemm.hip) for an [M, K] x [N, K]^T projection; split 0 where hipBLASLt
    is faster or the shape is unsupported.

    Measured per Llama-3-8B projection (profiles/r1_bench_kernels_dgemm.json at M <= 64,
    profiles/r1_dgemm_m128_sweep.log at 65-128 rows, weights rotated past the MALL): the
    LM head and, above 32 rows, gate|up stay on hipBLASLt; at <= 64 rows QKV / O / down use
    64-row tiles with the smallest split giving >= 192 workgroups; at 65-128 rows 128-row
    tiles (X re-read from L2 half as often) where such a split exists (QKV S=4: 21.9 us vs
    hipBLASLt 25.2 at M=128; O S=8: 17.2 vs 24.4), else 64-row tiles (down S=4: 40.7 vs 75.1)."""
    if M > 192 or N % 64 or N >= 65536 or (N >= 16384 and M > 32):
        return 0, 64
    if M > 128:
        # 129-192 rows (three m-tiles per wave, 64-row tiles only): only where a split gives
        # a full round of 256 workgroups -- O 21.8 us vs tuned hipBLASLt 23.9, down 54.2 vs
        # 65.3 at M=192; QKV (192 workgroups at S=2: 33.7 vs 27.3) stays on hipBLASLt
        # (profiles/r1_dgemm_m192_sweep.log)
        S = _splits_for(N, K, 64)
        return (S, 64) if S and (N // 64) * S >= 256 else (0, 64)
    # (QKV at S=4 times 11.6 vs 13.4 us alone at M = 1, profiles/r4_b1_decode_gemm_split_probe.log,
    # but the fused attention then sums twice the slabs: batch-1 decode 471-473 vs 468-470 ms
    # per query, profiles/r4_b1_ab.log -- S=2 stays)
    if M <= 64:
        return _splits_for(N, K, 64), 64
    S64 = _splits_for(N, K, 64)
    if N % 128 == 0:
        S = _splits_for(N, K, 128)
        # 128-row tiles, unless they need more than 4 split-K slabs where 64-row tiles fill
        # the chip with <= 4: the fused consumer re-reads every fp32 slab (O at M=128:
        # S=8 t128 17.2 us + 16.8 MB of slabs vs S=4 t64 16.5 us + 8.4 MB)
        if S and (N // 128) * S >= 192 and not (S > 4 and 0 < S64 <= 4 and (N // 64) * S64 >= 192):
            return S, 128
    return S64, 64


def decode_splits(M: int, N: int, K: int) -> int:
    """Split-K count of :func:`decode_plan` (0: use hipBLASLt)."""
    return decode_plan(M, N, K)[0]


def decode_linear(x, w):
    """x @ w^T for a decode step (<= 128 rows): the skinny weight-streaming MFMA kernel
    where it beats hipBLASLt on MI355X, else F.linear."""
    if _gpu(x):
        N, K = w.shape
        S = decode_splits(x.numel() // K, N, K)
        if S:
            return _native().dgemm(x.contiguous(), w, S)
    return torch.nn.functional.linear(x, w)


def dgemm_partial(x, w, splits: int, tile_rows: int = 64):
    """Split-K partial slabs [S, M, N] fp32 of x @ w^T (combine fused into the consumer:
    add_rmsnorm_splitk / rope_cache_splitk); tile_rows 64 or 128 weight rows per workgroup."""
    if _gpu(x):
        return _native().dgemm_partial(x.contiguous(), w, splits, tile_rows)
    K = w.shape[1]
    xs = x.float().reshape(-1, splits, K // splits)
    ws = w.float().reshape(-1, splits, K // splits)
    return torch.einsum("msk,nsk->smn", xs, ws).contiguous()


MID_M_MIN, MID_M_MAX = 129, 512
_MID_OFF = os.environ.get("DOCQA_MID_GEMM", "1") == "0"
_MID_CFG = int(os.environ.get("DOCQA_MID_CFG", "2"))
_MID_NARROW = os.environ.get("DOCQA_MID_NARROW", "1") == "1"
_MID_WG_CAP = int(os.environ.get("DOCQA_MID_WG_CAP", "224"))
_L2_XCD_BYTES = 4 << 20          # one XCD's L2 (MI355X_MICROARCH.md)


def mid_plan(M: int, N: int, K: int, glu: bool = False) -> tuple[int, int]:
    """(split-K count, kernel variant) of the mid-M decode GEMM (csrc/kernels/mgemm.hip) for
    an [M, K] x [N, K]^T projection at 129..512 rows; (0, 0) where it does not apply.
    ``glu``: the plan is for the fused-SwiGLU gate|up launch (mgemm_glu), which never
    splits K and has no 64-wide (cfg 7) variant -- only a non-zero S means "use it".

    Every workgroup owns all 256 rows of an m-tile x 128 weight rows; S is the largest
    divisor of K / 128 keeping (N / 128) x m-tiles x S <= 224 workgroups (one round on the
    256 CUs; fewer, larger slabs for the consumer where a round is already full).
    Measured at M = 256 against hipBLASLt (scripts/mgemm_probe.py, weights rotated past the
    MALL; profiles/r2_mgemm_probe_m256_v5.log): QKV S=4 21.9 us vs 43.1, O S=4 20.3 vs
    26.8 (S=8: 20.8 with twice the slab bytes), down S=7 40.1 vs 63.3, fused SwiGLU gate|up
    S=1 75.4 vs 67.8 + a 5.9 us silu_mul + a [M, 2I] round trip."""
    if _MID_OFF or not (MID_M_MIN <= M <= MID_M_MAX) or N % 128 or K % 128:
        return 0, 0
    # 129..192 rows: QKV / O / down gain over the skinny kernel and hipBLASLt (QKV 20.2-20.8
    # vs 27.7-33.4 us; profiles/r4_lm_head_probe.log, r2_mgemm_probe_m128_192.log); the wide
    # gate|up with fused SwiGLU is at parity with hipBLASLt + silu_mul (62.3 / 64.7 vs
    # 62.4 / 66.5 us at M = 160 / 192) and takes it too
    tiles = (N // 128) * ((M + 255) // 256)
    kb = K // 128
    S = max(s for s in range(1, kb + 1) if kb % s == 0 and (s == 1 or tiles * s <= _MID_WG_CAP))
    if glu:
        return S, _MID_CFG
    if _MID_CFG == 2 and M * K * 2 > _L2_XCD_BYTES and kb % 8 == 0 and tiles * 8 <= 256 and S < 8:
        # activations larger than one XCD's L2 (down: 256 x 14336 bf16 = 7.3 MB): 8 slices,
        # one per XCD (mgemm.hip remap 1), so each L2 holds only its 0.9 MB slice of X --
        # down S=8 40.5 vs S=7 44.1 us, 46.4 vs 48.8 with the add+norm consumer
        # (profiles/r5_mid_consumer_probe.log)
        return 8, _MID_CFG
    if _MID_CFG == 2 and _MID_NARROW and S > 1 and tiles * S <= 128 and N % 64 == 0:
        # the split left half the chip idle (O: 32 tiles x S=4): 64-wide tiles (cfg 7) at
        # the same split fill it with the same slab bytes -- O 17.5 vs 20.7 us
        # (profiles/r2_mgemm_probe_bn64.log)
        return S, 7
    if _MID_CFG == 2 and _MID_NARROW and S == 1 and tiles * 2 <= 256 and N % 64 == 0:
        # no split under the cap (the 70B TP-8 O / down shards, 128 tiles at 257..512 rows):
        # twice the workgroups -- short K (O, 1024) by 64-wide tiles, 22.6 vs 26.3 us at 512
        # rows (hipBLASLt 23.2), long K (down, 3584) by a 2-way split, 46.5 vs 58.8 (46.1)
        # (profiles/r6_prefill_mid_plans.log)
        return (2, 2) if K >= 2048 and kb % 2 == 0 else (1, 7)
    return S, _MID_CFG


# bf16 split-K slabs for the mid-M decode GEMM's fused consumers (RoPE + cache write, add +
# RMSNorm) at TP = 1: half the slab bytes the GEMM writes and its consumer reads; each
# partial is rounded to bf16 once before the consumer's fp32 sum (as a bf16 all-reduce
# rounds each rank's partial)
SLAB_BF16 = os.environ.get("DOCQA_SLAB_BF16", "1") == "1"


def mgemm_partial(x, w, splits: int, cfg: int = 0, bf16: bool = False):
    """Split-K partial slabs [S, M, N] fp32 (``bf16``: bf16) of x @ w^T on the mid-M decode
    GEMM (S = 1 without ``bf16``: the bf16 product [M, N])."""
    if _gpu(x):
        if bf16:
            return _native().mgemm_slab16(x.contiguous(), w, splits, cfg)
        return _native().mgemm(x.contiguous(), w, splits, cfg)
    if splits == 1 and not bf16:
        return torch.nn.functional.linear(x, w)
    K = w.shape[1]
    xs = x.float().reshape(-1, splits, K // splits)
    ws = w.float().reshape(-1, splits, K // splits)
    out = torch.einsum("msk,nsk->smn", xs, ws).contiguous()
    return out.to(torch.bfloat16) if bf16 else out


def pgemm_partial(x, w, splits: int):
    """Split-K partial slabs [S, M, N] fp32 of x @ w^T on the 256 x 256 prefill GEMM."""
    if _gpu(x):
        return _native().pgemm_partial(x.contiguous(), w, splits)
    K = w.shape[1]
    xs = x.float().reshape(-1, splits, K // splits)
    ws = w.float().reshape(-1, splits, K // splits)
    return torch.einsum("msk,nsk->smn", xs, ws).contiguous()


def mgemm_glu(x, w_il, cfg: int = 0):
    """silu(x Wg^T) * (x Wu^T) for 8-interleaved gate|up weights on the mid-M decode GEMM."""
    if _gpu(x):
        return _native().mgemm_glu(x.contiguous(), w_il, cfg)
    return silu_mul(torch.nn.functional.linear(x, w_il), interleaved=True)


# batch-256 decode gate|up as 256-wide tiles split over K into bf16 slabs + the split-K
# SwiGLU consumer (act.hip silu_mul_splitk16) instead of the fused-SwiGLU 128-wide tiles: X
# is re-read from L2 112 instead of 224 times (scripts/gateup_split_probe.py, cold weights:
# GEMM 64.3 us at cfg 6 S=2 vs 78.8 us fused)
_GLU_SPLIT16 = os.environ.get("DOCQA_GLU_SPLIT16", "0") == "1"


def glu_split16_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(S, cfg) of the split bf16-slab gate|up (:func:`glu_split16`) for an [M, K] x [N, K]^T
    gate|up at TP = 1, or (0, 0): one 256-row m-tile (193..256 rows), 256-wide tiles, two K
    slices -- (N / 256) x 2 workgroups must fit one round of the chip."""
    if not (SLAB_BF16 and _GLU_SPLIT16) or not (193 <= M <= 256):
        return 0, 0
    if N % 256 or K % 256 or (N // 256) * 2 > 256:
        return 0, 0
    return 2, 6


def glu_split16(x, w_il, S: int, cfg: int):
    """silu(x Wg^T) * (x Wu^T) from S bf16 split-K slabs (mgemm cfg ``cfg``)."""
    if _gpu(x):
        return _native().silu_mul_splitk(_native().mgemm_slab16(x.contiguous(), w_il, S, cfg))
    return silu_mul(torch.nn.functional.linear(x, w_il), interleaved=True)


# ----------------------------------------------------------------------------- prefill GEMM
_PGEMM_OFF = os.environ.get("DOCQA_PGEMM", "1") == "0"
# below this many 256 x 256 tiles the 128 x 128 encoder GEMM (gemm.hip, 4x the workgroups)
# fills the chip better (scripts/pgemm_probe.py)
_PGEMM_MIN_TILES = int(os.environ.get("DOCQA_PGEMM_MIN_TILES", "128"))


def pgemm_ok(M: int, N: int, K: int) -> bool:
    """Shapes the prefill GEMM (csrc/kernels/pgemm.hip) takes: N % 256, K % 128, 32-bit
    row offsets, and enough 256 x 256 tiles to fill the chip."""
    return (not _PGEMM_OFF and M > 0 and N % 256 == 0 and K % 128 == 0
            and max(M, N) * K * 2 < (1 << 32) and ((M + 255) // 256) * (N // 256) >= _PGEMM_MIN_TILES)


PREFILL_MID_MAX = 2048
# Mid-M prefill (513..2048 packed prompt tokens; the Llama-3-70B TP-8 shards from 257 rows):
# every projection on the hand-written kernels -- no library GEMM.  Measured WITH each
# projection's consumer and weights rotated past the MALL (scripts/prefill_mid_probe.py,
# profiles/r6_prefill_mid_plans.log): where the 256 x 256 tiles cannot fill the 256 CUs the
# K dimension is split into fp32 slabs (pgemm.hip EPI_PARTIAL, one K slice per XCD group)
# that the consumer which runs anyway sums -- RoPE + KV write (QKV), residual add + RMSNorm
# (O / down), SwiGLU (gate|up: act.hip silu_mul_splitk) -- :func:`prefill_split_plan`; a
# few measured shapes keep the mid-M kernel (:func:`prefill_plan`).  What the forward runs
# (:func:`prefill_route`) against hipBLASLt + the same consumer at 512..2048 rows: 0.93..1.47x,
# 36 of 40 (shape, M) points >= 0.95x.
_PREFILL_SPLIT_MIN_K = 1024       # K per slice below this loses to fewer slices (O at 512 rows: S=8 42.0 vs S=4 37.5 us)


_PREFILL_PLANS = os.environ.get("DOCQA_PREFILL_PLANS", "1") != "0"


def prefill_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, mgemm cfg) of a 513..2048-row prefill projection on the mid-M kernel,
    (0, 0) for the 256 x 256 kernel (split-K slabs where :func:`prefill_split_plan` says so,
    else bf16 tiles).  S >= 2: fp32 slabs into the split-K consumers (RoPE + KV write, add +
    RMSNorm); S == 1: the bf16 product.  Since round 6 the 256 x 256 split plans take every
    shape they apply to except the two points measured faster here (8B O and the 70B TP-8
    down shard at 769..1024 rows, profiles/r6_prefill_mid_plans.log); the remaining rules
    are round 4's (profiles/r4_prefill_mid_probe.log) for shapes no split plan takes."""
    if not _PREFILL_PLANS or _MID_OFF or not (MID_M_MAX < M <= PREFILL_MID_MAX) or N % 128 or K % 128:
        return 0, 0
    if 769 <= M <= 1024 and (N, K) in ((4096, 4096), (8192, 3584)):
        # the two measured points where the mid-M kernel beats the split 256 x 256 tiles:
        # 8B O S=2 48.5 vs pgemm S=4 50.9 us, 70B TP-8 down S=1 71.9 vs pgemm S=2 75.4
        return (2, 2) if N == 4096 else (1, 2)
    if prefill_split_plan(M, N, K):
        return 0, 0
    if N < 4096:
        # narrow N (the 70B TP-8 QKV shard, N 1280 x K 8192): the mid-M kernel's few 128-wide
        # tiles lose to the 256 x 256 kernel's split-K (profiles/r4_pgemm_mid_probe.log)
        return 0, 0
    if N >= 6144 and K <= 4096:          # QKV-like: wide N
        return (1, 2) if M <= 1024 else (0, 0)
    if M <= 1024 and (K // 128) % 2 == 0:
        return 2, 2
    return 1, 2


def prefill_split_plan(M: int, N: int, K: int, glu: bool = False) -> int:
    """Split-K count for a prefill projection whose 256 x 256 tiles cannot fill the chip:
    the largest S (<= DOCQA_PREFILL_SPLIT_MAX) with tiles x S <= 256 workgroups and >= 1024
    of K per slice.  The fp32 slabs [S, M, N] go straight into the split-K consumer that runs
    anyway (RoPE + KV write, (TP all-reduce +) add + RMSNorm, SwiGLU).  Measured with the
    consumer (profiles/r6_prefill_mid_plans.log): 8B down S=4 93.8 vs hipBLASLt 115.9 us at
    768 rows, QKV S=2 55.3 vs 55.2, O S=4 42.3 vs 40.3; 70B TP-8 gate|up S=4 69.2 vs 84.2 at
    512 rows, QKV shard S=8 32.2 vs 35.8.  0: no split (enough tiles, or not a pgemm shape).
    ``glu``: the gate|up shard's S (consumer silu_mul_splitk), from 257 rows (measured at
    512+; below that the decode-sized mid-M SwiGLU kernel keeps it).  DOCQA_PREFILL_SPLIT=0
    disables."""
    if (not _PREFILL_SPLIT or _PGEMM_OFF or M <= 0 or N % 256 or K % 256
            or max(M, N) * K * 2 >= (1 << 32)):
        return 0
    if M <= MID_M_MAX and not (N < 4096 or (glu and M > 256)):
        return 0          # decode-sized M: the mid-M kernel's plans (mid_plan)
    tiles = ((M + 255) // 256) * (N // 256)
    S = 1
    while (S < _PREFILL_SPLIT_MAX and tiles * S * 2 <= 256 and K % (128 * S * 2) == 0
           and K // (S * 2) >= _PREFILL_SPLIT_MIN_K):
        S *= 2
    return S if S >= 2 else 0


def down_small_split(M: int, N: int, K: int) -> int:
    """Split-K count of a 257..512-row prefill's down projection on the 256 x 256 kernel
    (long K: the 8B down, 14336): S=8 slabs into add + RMSNorm, 67.5 vs 77.5 us for the mid-M
    kernel's S=4 and 98.7 for hipBLASLt at 512 rows (profiles/r6_prefill_mid_plans.log).
    0 where it does not apply (fewer than 4 slices of >= 1024)."""
    if not (256 < M <= MID_M_MAX) or _PGEMM_OFF or not _PREFILL_SPLIT or N % 256 or K % 256:
        return 0
    tiles = ((M + 255) // 256) * (N // 256)
    S = 1
    while S < 8 and tiles * S * 2 <= 256 and K % (128 * S * 2) == 0 and K // (S * 2) >= _PREFILL_SPLIT_MIN_K:
        S *= 2
    return S if S >= 4 else 0


_PREFILL_SPLIT = os.environ.get("DOCQA_PREFILL_SPLIT", "1") != "0"
_PREFILL_SPLIT_MAX = int(os.environ.get("DOCQA_PREFILL_SPLIT_MAX", "8"))


def prefill_linear(x, w):
    """x @ w^T for the prefill projections (M = packed prompt tokens) on the hand-written
    MFMA GEMMs: the mid-M kernel's bf16 product where :func:`prefill_plan` says so, the
    256 x 256 8-phase kernel (pgemm.hip) where it has enough tiles, else the 128 x 128
    kernel (gemm.hip); hipBLASLt only for shapes none takes."""
    if _gpu(x):
        N, K = w.shape
        M = x.numel() // K
        S, cfg = prefill_plan(M, N, K)
        if S == 1:
            return _native().mgemm(x.contiguous(), w, 1, cfg)
        Sp = prefill_split_plan(M, N, K)
        if Sp:
            # a caller without a split-K consumer (the mixed prefill/decode forward): the
            # slabs summed here, still ahead of the 128 x 128 kernel at these shapes
            return _native().pgemm_partial(x.contiguous(), w, Sp).sum(0).to(torch.bfloat16)
        if pgemm_ok(M, N, K):
            return _native().pgemm(x.contiguous(), w, 0)
        if N % 128 == 0 and K % 64 == 0:
            return _native().gemm(x.contiguous(), w, None, None, EPI_NONE)
    return torch.nn.functional.linear(x, w)


def prefill_route(M: int, N: int, K: int, glu: bool = False, down: bool = False):
    """(label, fn(x, w)) of what a prefill projection of M rows runs in models/llama.py
    (its per-forward plan logic, mirrored here for probes): split-K slab plans return the
    fp32 slabs [S, M, N] their consumer sums; ``down``: the 257..512-row down override."""
    nat = _native
    if glu:
        if M <= MID_M_MAX and not (pgemm_ok(M, N, K) or prefill_split_plan(M, N, K, glu=True)):
            Sg, cg = mid_plan(M, N, K, glu=True)
            if Sg:
                return f"mgemm_glu c{cg}", lambda x, w: nat().mgemm_glu(x.contiguous(), w, cg)
            return "glu_linear", glu_linear
        Sg = prefill_split_plan(M, N, K, glu=True)
        return (f"pgemm S{Sg}+silu_splitk" if Sg else "prefill_glu"), prefill_glu
    if down and M <= MID_M_MAX and M > 256 and down_small_split(M, N, K):
        Sd = down_small_split(M, N, K)
        return f"pgemm S{Sd}", lambda x, w: nat().pgemm_partial(x.contiguous(), w, Sd)
    if M <= MID_M_MAX:
        S, c = mid_plan(M, N, K)
        if S:
            return f"mgemm S{S} c{c}", lambda x, w: nat().mgemm(x.contiguous(), w, S, c)
        S, t = decode_plan(M, N, K)
        return f"dgemm S{S} t{t}", lambda x, w: dgemm_partial(x, w, S, t)
    S, c = prefill_plan(M, N, K)
    if S >= 2:
        return f"mgemm S{S} c{c}", lambda x, w: nat().mgemm(x.contiguous(), w, S, c)
    if not S:
        Sp = prefill_split_plan(M, N, K)
        if Sp:
            return f"pgemm S{Sp}", lambda x, w: nat().pgemm_partial(x.contiguous(), w, Sp)
    return "prefill_linear", prefill_linear


_GLU128 = os.environ.get("DOCQA_GLU128", "1") != "0"


def prefill_glu(x, w_il):
    """silu(x Wg^T) * (x Wu^T) for 8-interleaved gate|up weights at prefill sizes: SwiGLU
    fused into the 256 x 256 GEMM's epilogue (no [M, 2I] round trip through HBM)."""
    if _gpu(x):
        N, K = w_il.shape
        M = x.numel() // K
        S = prefill_split_plan(M, N, K, glu=True)
        if S:
            # too few 256 x 256 tiles (the 70B TP-8 shard: 56 at 512 rows): K split into fp32
            # slabs, summed by the SwiGLU consumer -- 69.2 vs hipBLASLt + silu_mul 84.2 us
            return _native().silu_mul_splitk(_native().pgemm_partial(x.contiguous(), w_il, S))
        if pgemm_ok(M, N, K):
            return _native().pgemm(x.contiguous(), w_il, 1)
        if (_GLU128 and N % 128 == 0 and K % 64 == 0 and ((M + 255) // 256) * (N // 128) < 128
                and ((M + 127) // 128) * (N // 128) >= 192):
            # too few 256 x 256 tiles, and the 256 x 128 kernel would leave half the CUs idle:
            # the 128 x 128 tiles with the SwiGLU epilogue (gemm.hip EPI_GLU) -- 70B TP-8
            # gate|up shard at 512 rows 90.8 us vs 106.1 (256 x 128) and 132.7 (256 x 256);
            # hipBLASLt + silu_mul 64.6 (profiles/r5_pgemm_70b_split_probe.log)
            return _native().gemm(x.contiguous(), w_il, None, None, EPI_GLU)
        if N % 128 == 0 and K % 128 == 0:
            return _native().mgemm_glu(x.contiguous(), w_il, 2)
    return silu_mul(prefill_linear(x, w_il), interleaved=True)


# LM head: 256-wide tiles (mgemm.hip cfg 6) halve the X re-reads of the 1002-tile vocab
# sweep -- 281 vs 326 us with the argmax fused at M = 256 (profiles/r2_mgemm_probe_m256_v6.log)
_LM_CFG = int(os.environ.get("DOCQA_LM_HEAD_CFG", "6"))
_GEMV_LM = os.environ.get("DOCQA_GEMV_LM", "1") != "0"


def lm_head_argmax(x, w, n_valid: int, cfg: int = -1, with_values: bool = False, streamed=None, fp8=None,
                   mxfp4=None):
    """Greedy token ids argmax(bf16(x @ w[:n_valid]^T)) with the LM-head GEMM and the argmax
    fused (mgemm.hip EPI_ARGMAX): the [M, vocab] logits never reach HBM.  ``with_values``:
    (ids, picked logit fp32) -- a vocab-parallel shard's candidates for comm.tp_argmax.
    ``streamed``: (format, pair), a :data:`STREAMED` copy of ``w`` (``w`` its exact image): (q, s)
    of :func:`quantize_fp8_rows` or (q, e) of :func:`quantize_mxfp4_rows` -- a one-row step
    streams the codes where the format's GEMV lists the shape, a 2..32-row step where its ring
    kernel does, a 33..128-row step where its wide kernel does (dgemm.hip EPI_ARGMAX); every other
    step runs on ``w``.  ``fp8=pair`` and
    ``mxfp4=pair`` spell the same argument per format."""
    if streamed is None and (fp8 is not None or mxfp4 is not None):
        streamed = ("mxfp4", mxfp4) if mxfp4 is not None else ("fp8-e4m3", fp8)
    if _gpu(x):
        N, K = w.shape
        fmt, pair = streamed or ("", None)
        kind = next((k for k in (_kinds(fmt) if fmt and n_valid > 0 else ())
                     if _streamed_fn(fmt, k, "argmax_ok")(x.numel() // K, N, K)), "")
        if kind:
            # the GEMV takes its (rows, codes per load ...) from the format's EPI table
            f = STREAMED[fmt]
            epi = globals()[f.gemv_epi][K] if kind == "gemv" else ()
            op = getattr(_native(), f"{getattr(f, kind)}_argmax_val")
            ids, vals = op(x.contiguous(), *pair, int(n_valid), *epi)
            return (ids, vals) if with_values else ids
        if (_GEMV_LM and x.numel() == K and N % 16 == 0 and K % 2048 == 0 and K // 2048 <= 2
                and n_valid > 0):
            # one row: the register-streaming GEMV with the argmax in its epilogue
            # (profiles/r6_b1_lm_head_gemv_ab.log)
            ids, vals = _native().gemv_argmax_val(x.contiguous(), w, int(n_valid))
            return (ids, vals) if with_values else ids
        if x.numel() // K <= 32 and N % 64 == 0 and K % 512 == 0:
            # <= 32 rows (batch-1 decode included): the skinny weight-streaming kernel with
            # the argmax in its epilogue (dgemm.hip EPI_ARGMAX) -- 197.6 / 203.4 us at M = 1 /
            # 32 vs hipBLASLt + argmax 190.1 / 201.3; from 33 rows the mid-M kernel's 256-row
            # tiles stream the vocab once (256-275 us flat; profiles/r4_lm_head_probe.log)
            ids, vals = _native().dgemm_argmax_val(x.contiguous(), w, int(n_valid))
            return (ids, vals) if with_values else ids
        if cfg < 0:
            cfg = _LM_CFG if w.shape[0] % 256 == 0 else _MID_CFG
        if with_values:
            return _native().mgemm_argmax_val(x.contiguous(), w, int(n_valid), cfg)
        return _native().mgemm_argmax(x.contiguous(), w, int(n_valid), cfg)
    logits = torch.nn.functional.linear(x, w[:n_valid])
    ids = ref.argmax(logits)
    if with_values:
        return ids, logits.gather(1, ids[:, None])[:, 0].float()
    return ids


def lm_head_logits(x, w):
    """bf16 logits x @ w^T of the LM head for SAMPLED rows (temperature > 0: the Ollama
    API's options), on the hand-written GEMMs at every row count: the skinny
    weight-streaming kernel up to 192 rows (dgemm.hip, one pass over the vocab), the mid-M
    kernel with 256-wide tiles up to 512, the prefill kernels
    beyond -- no library GEMM.  Greedy rows never get here: their
    argmax is fused into the GEMM (:func:`lm_head_argmax`)."""
    if _gpu(x):
        N, K = w.shape
        M = x.numel() // K
        if 0 < M <= 192 and N % 64 == 0 and K % 512 == 0:
            return _native().dgemm(x.contiguous(), w, 1)
        if 0 < M <= MID_M_MAX and N % 128 == 0 and K % 128 == 0 and not _MID_OFF:
            cfg = _LM_CFG if N % 256 == 0 else _MID_CFG
            return _native().mgemm(x.contiguous(), w, 1, cfg)
        return prefill_linear(x, w)
    return torch.nn.functional.linear(x, w)


def lm_head_argmax_shape_ok(N: int, K: int) -> bool:
    return not _MID_OFF and N % 128 == 0 and K % 128 == 0


def lm_head_argmax_ok(M: int, N: int, K: int) -> bool:
    """Fused LM head + argmax at every decode bucket: dgemm.hip up to 32 rows, mgemm.hip
    from 33 to 512 (no [M, vocab] logits, no library GEMM)."""
    if M <= 32 and N % 64 == 0 and K % 512 == 0:
        return M > 0
    return not _MID_OFF and 0 < M <= MID_M_MAX and N % 128 == 0 and K % 128 == 0


def embed_rmsnorm(ids, table, w, eps: float):
    """(h, x): h = table[ids] (the residual stream), x = rmsnorm(h) * w -- the Llama input
    embedding and the first layer's norm in one launch."""
    if _gpu(table):
        return _native().embed_rmsnorm(ids.contiguous(), table, w, float(eps))
    h = embedding(ids, table)
    return h, rmsnorm(h, w, eps)


_XN = os.environ.get("DOCQA_DECODE_XN", "1") != "0"


def xn_ok(M: int, K: int) -> bool:
    """Batch-1 projections that build their own input row (residual add + RMSNorm of the
    previous projection's slabs, in LDS) -- :func:`dgemm_partial_xn`, :func:`dgemm_glu_xn`."""
    return _XN and M == 1 and K <= 4096 and K % 512 == 0


def dgemm_partial_xn(Pin, res_in, res_out, gamma, eps: float, w, splits: int):
    """Split-K slabs of x @ w^T for the one row x = rmsnorm(res_in + bf16(sum Pin)) * gamma,
    built inside the projection (no add_rmsnorm launch); res_out <- res_in + bf16(sum Pin)
    (a second buffer -- every workgroup still reads res_in)."""
    if _gpu(Pin):
        return _native().dgemm_partial_xn(Pin, res_in, res_out, gamma, float(eps), w, int(splits))
    res_out.copy_(res_in)
    x = ref.add_rmsnorm(Pin.sum(0).to(res_out.dtype).view_as(res_out), res_out, gamma, eps)
    return torch.nn.functional.linear(x.float(), w.float())[None].reshape(1, 1, -1).expand(splits, 1, -1) / splits


def dgemm_glu_xn(Pin, res_in, res_out, gamma, eps: float, w_il):
    """silu(x Wg^T) * (x Wu^T) for x = rmsnorm(res_in + bf16(sum Pin)) * gamma (one row, built
    in-kernel); res_out <- res_in + bf16(sum Pin)."""
    if _gpu(Pin):
        return _native().dgemm_glu_xn(Pin, res_in, res_out, gamma, float(eps), w_il)
    res_out.copy_(res_in)
    x = ref.add_rmsnorm(Pin.sum(0).to(res_out.dtype).view_as(res_out), res_out, gamma, eps)
    return silu_mul(torch.nn.functional.linear(x, w_il), interleaved=True)


_GEMV = os.environ.get("DOCQA_GEMV", "1") != "0"


_GEMV_DOWN = os.environ.get("DOCQA_GEMV_DOWN", "1") == "1"
_GEMV_R = int(os.environ.get("DOCQA_GEMV_R", "8"))   # rows per workgroup, K <= 4096 (A/B knob)


def gemv_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the batch-1 register-streaming GEMV
    (dgemm.hip gemv_kernel: every lane issues all its weight loads at once, no LDS ring)
    for a one-row projection; (0, 0) where the ring kernel stays.  Measured at M = 1 on the
    Llama-3-8B projections, weights rotated past the MALL (profiles/r6_gemv_probe.log): O
    7.8 vs 8.8 us for the ring kernel's plan; the QKV with its input row built in-kernel
    (XNormIn: every workgroup runs that prologue, so few wide workgroups win) 13.3 vs 15.4
    at 8 rows per workgroup, no split (17.9 at 4 rows x 2 slices).  The down projection
    (K 14336) alone is 21.3 vs the ring's 20.9 us, but on the GEMV (4 rows, no split) it
    hands the next QKV ONE slab to build its input row from instead of four: with the
    non-temporal weight loads, batch-1 p50 454 -> 431 ms (profiles/r6_b1_nt_down_ab.log;
    DOCQA_GEMV_DOWN=0 keeps the ring).  DOCQA_GEMV=0 disables."""
    if not _GEMV or M != 1 or N % 8 or K % 2048:
        return 0, 0
    if K > 8192:
        # one slab for the next QKV's in-kernel input row instead of the ring's four
        return (1, 4) if _GEMV_DOWN and K // 2048 == 7 else (0, 0)
    return (1, _GEMV_R) if K <= 4096 else ((2, 8) if K % 4096 == 0 else (0, 0))


def gemv_glu_ok(M: int, N: int, K: int) -> bool:
    """The batch-1 gate|up projection with SwiGLU on the GEMV (one 16-row gate|up group per
    workgroup): 41.1 vs 47.6 us for the ring kernel at Llama-3-8B (profiles/r6_gemv_probe.log)."""
    return _GEMV and M == 1 and N % 16 == 0 and K % 2048 == 0 and (K // 2048) in (1, 2)


def gemv_glu(x, w_il):
    """silu(x Wg^T) * (x Wu^T) for one row on the batch-1 GEMV (:func:`gemv_glu_ok`)."""
    if _gpu(x):
        return _native().gemv(x.contiguous(), w_il, 1, 16, True)
    return glu_linear(x, w_il)


def gemv_partial(x, w, splits: int, rows: int):
    """fp32 slabs [S, 1, N] of one row x @ w^T on the batch-1 GEMV (:func:`gemv_plan`)."""
    if _gpu(x):
        return _native().gemv(x.contiguous(), w, int(splits), int(rows), False)
    return dgemm_partial(x, w, splits, 64)


def gemv_partial_xn(Pin, res_in, res_out, gamma, eps: float, w, splits: int, rows: int):
    """:func:`dgemm_partial_xn` (input row built in-kernel) on the batch-1 GEMV."""
    if _gpu(Pin):
        return _native().gemv_xn(Pin, res_in, res_out, gamma, float(eps), w, int(splits), int(rows), False)
    return dgemm_partial_xn(Pin, res_in, res_out, gamma, eps, w, splits)


def gemv_glu_xn(Pin, res_in, res_out, gamma, eps: float, w_il):
    """:func:`dgemm_glu_xn` (input row built in-kernel, SwiGLU epilogue) on the batch-1 GEMV."""
    if _gpu(Pin):
        return _native().gemv_xn(Pin, res_in, res_out, gamma, float(eps), w_il, 1, 16, True)
    return dgemm_glu_xn(Pin, res_in, res_out, gamma, eps, w_il)


# ----------------------------------------------------------------------------- FP8 weights
# Batch-1 GEMV over FP8 weights (dgemm.hip gemv8_kernel): per output row OCP e4m3fn codes q
# and a power-of-two scale s, W' = q * s exactly the model's resident bf16 weights
# (LlamaModel.quantize_fp8), so a one-row step streams half the bytes and computes the same
# products as every other kernel does from W'.
quantize_fp8_rows, dequantize_fp8_rows = ref.quantize_fp8_rows, ref.dequantize_fp8_rows

_GEMV8 = os.environ.get("DOCQA_GEMV8", "1") != "0"
# K -> (split-K count, weight rows per workgroup, codes per lane per load) of the split-K slab
# projections, and K -> (rows, codes per load) of the SwiGLU / LM-head argmax epilogues.  Every
# entry names an instantiation of gemv8_kernel (GEMV8_CASES); shapes that are absent keep the
# bf16 GEMV on W'.  benchmarks/bench_gemv_fp8.py times each entry against the bf16 plan
# (profiles/fp8_gemv_probe.log: QKV 9.9 vs 12.2 us, O 6.9 vs 7.9, gate|up 25.3 vs 39.3, down 13.1
# vs 20.0, LM head 89.2 vs 159.0 at Llama-3-8B -- every shape faster, so every one is listed).
_GEMV8_PLAN = {2048: (1, 8, 8), 4096: (1, 8, 16), 8192: (1, 8, 16), 14336: (1, 4, 8)}
_GEMV8_EPI = {2048: (16, 8), 4096: (16, 16)}
# (rows, chunks per lane, codes per load) instantiated for slabs; XN: also with the in-kernel
# input row (K <= 4096); EPI: the SwiGLU / argmax epilogues
GEMV8_CASES = [(8, 1, 8), (16, 1, 8), (8, 2, 8), (16, 2, 8), (8, 1, 16), (16, 1, 16), (32, 1, 16),
               (4, 4, 8), (8, 4, 8), (4, 7, 8), (8, 2, 16), (16, 2, 16)]
GEMV8_XN_CASES = GEMV8_CASES[:7]
GEMV8_EPI_CASES = [(16, 1, 8), (32, 1, 8), (16, 2, 8), (16, 1, 16), (32, 1, 16)]


def gemv8_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the FP8-weight GEMV for a one-row
    projection; (0, 0) where the kernel has no instantiation or does not beat the bf16 GEMV
    (the caller then streams the bf16 image W').  DOCQA_GEMV8=0 disables."""
    S, R, lb = _GEMV8_PLAN.get(K, (0, 0, 0))
    if not _GEMV8 or M != 1 or not S or N % R or (K // S) % (256 * lb):
        return 0, 0
    if (R, K // S // (256 * lb), lb) not in GEMV8_CASES:
        return 0, 0
    return S, R


def gemv8_lb(K: int, splits: int = 1) -> int:
    """Codes per lane per load (8 | 16) the plan tables use at this K (8 where none)."""
    if K in _GEMV8_PLAN and _GEMV8_PLAN[K][0] == splits:
        return _GEMV8_PLAN[K][2]
    return 8


def gemv8_glu_ok(M: int, N: int, K: int) -> bool:
    """The batch-1 gate|up projection with SwiGLU on the FP8-weight GEMV."""
    R, lb = _GEMV8_EPI.get(K, (0, 0))
    return bool(_GEMV8 and M == 1 and R and N % R == 0 and (R, K // (256 * lb), lb) in GEMV8_EPI_CASES)


def gemv8_argmax_ok(M: int, N: int, K: int) -> bool:
    """The batch-1 LM head + greedy pick on the FP8-weight GEMV."""
    return gemv8_glu_ok(M, N, K)


def gemv8_partial(x, q, s, splits: int, rows: int, lb: int = 0):
    """fp32 slabs [S, 1, N] of one row x @ (q * s)^T on the FP8-weight GEMV (:func:`gemv8_plan`)."""
    if _gpu(x):
        return _native().gemv8(x.contiguous(), q, s, int(splits), int(rows), int(lb) or gemv8_lb(q.shape[1], splits),
                               False)
    return gemv_partial(x, dequantize_fp8_rows(q, s, x.dtype), splits, rows)


def gemv8_partial_xn(Pin, res_in, res_out, gamma, eps: float, q, s, splits: int, rows: int, lb: int = 0):
    """:func:`gemv_partial_xn` (input row built in-kernel) over FP8 weights."""
    if _gpu(Pin):
        return _native().gemv8_xn(Pin, res_in, res_out, gamma, float(eps), q, s, int(splits), int(rows),
                                  int(lb) or gemv8_lb(q.shape[1], splits), False)
    return gemv_partial_xn(Pin, res_in, res_out, gamma, eps, dequantize_fp8_rows(q, s, res_in.dtype), splits, rows)


def gemv8_glu(x, q, s, rows: int = 0, lb: int = 0):
    """silu(x Wg^T) * (x Wu^T) for one row over FP8 8-interleaved gate|up weights."""
    if _gpu(x):
        R, l = _GEMV8_EPI.get(q.shape[1], (16, 8))
        return _native().gemv8(x.contiguous(), q, s, 1, int(rows) or R, int(lb) or l, True)
    return gemv_glu(x, dequantize_fp8_rows(q, s, x.dtype))


def gemv8_glu_xn(Pin, res_in, res_out, gamma, eps: float, q, s, rows: int = 0, lb: int = 0):
    """:func:`gemv_glu_xn` (input row built in-kernel, SwiGLU epilogue) over FP8 weights."""
    if _gpu(Pin):
        R, l = _GEMV8_EPI.get(q.shape[1], (16, 8))
        return _native().gemv8_xn(Pin, res_in, res_out, gamma, float(eps), q, s, 1, int(rows) or R, int(lb) or l,
                                  True)
    return gemv_glu_xn(Pin, res_in, res_out, gamma, eps, dequantize_fp8_rows(q, s, res_in.dtype))


# --------------------------------------------------------------------------- MXFP4 weights
# Batch-1 GEMV over OCP MXFP4 weights (dgemm.hip gemv4_kernel): q [N, K / 2] pairs of e2m1 codes
# and e [N, K / 32] e8m0 block scales, W' = code * 2^(e - 127) exactly the model's resident bf16
# weights (LlamaModel.quantize_mxfp4), so a one-row step streams 4.25 bits per weight and
# computes the same products as every other kernel does from W'.
quantize_mxfp4_rows, dequantize_mxfp4_rows = ref.quantize_mxfp4_rows, ref.dequantize_mxfp4_rows

_GEMV4 = os.environ.get("DOCQA_GEMV4", "1") != "0"
# (N, K) -> (split-K count, weight rows per workgroup, codes per lane per load, waves along K) of
# the split-K slab projections, and K -> (rows, codes per load, waves along K) of the SwiGLU /
# LM-head argmax epilogues.  Every entry names an instantiation of gemv4_kernel (GEMV4_CASES) and
# is listed only where benchmarks/bench_gemv_mxfp4.py measured its median below BOTH the bf16
# GEMV's and the FP8 GEMV's shipped plans with disjoint min..max window ranges
# (profiles/mxfp4_gemv_probe.log, us MXFP4 / FP8 / bf16: QKV 6144 x 4096 7.5 / 9.9 / 12.2, down
# 4096 x 14336 9.7 / 13.3 / 20.2, gate|up 28672 x 4096 16.5 / 25.0 / 39.4, LM head 128256 x 4096
# 48.5 / 89.5 / 159.0, 32768 x 4096 17.5 / 27.7 / 45.5; the test preset: gate|up 16384 x 2048 8.0 / 12.1 / 15.3, LM head 32000 x 2048 11.4 / 17.4 / 26.4).  The
# slab table is keyed by the whole shape because the narrow, latency-bound projections LOST at the
# same K and keep the bf16 GEMV on W': O 4096 x 4096 (6.1 us against FP8's 6.2, ranges overlap),
# and the test preset's QKV 3072 x 2048 (6.2 / 6.4 / 6.8, overlapping), O 2048 x 2048 (5.1 -
# 5.3 against bf16's 4.8) and down 2048 x 8192 (5.2 / 6.0 / 7.9 in the first run of the log, but
# 6.05 against FP8's 6.4 with overlapping ranges in the second).
_GEMV4_PLAN = {(6144, 4096): (1, 8, 32, 2), (4096, 14336): (1, 4, 16, 2)}
_GEMV4_EPI = {2048: (16, 32, 1), 4096: (16, 32, 2)}
# (rows, chunks per lane, codes per load, waves along K) instantiated for slabs -- the smallest K
# an entry takes is chunks x 64 x codes x waves; XN: also with the in-kernel input row
# (K <= 4096); EPI: the SwiGLU / argmax epilogues
GEMV4_CASES = [(16, 1, 32, 1), (32, 1, 32, 1), (8, 1, 32, 2), (16, 1, 32, 2), (16, 2, 32, 1), (8, 1, 16, 4),
               (8, 1, 16, 2), (8, 1, 32, 4), (16, 1, 32, 4), (4, 7, 32, 1), (8, 7, 32, 1), (4, 7, 16, 2)]
GEMV4_XN_CASES = GEMV4_CASES[:7]
GEMV4_EPI_CASES = [(16, 1, 32, 1), (32, 1, 32, 1), (16, 1, 32, 2), (32, 1, 32, 2), (16, 2, 32, 1), (16, 1, 16, 4)]


def gemv4_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the MXFP4-weight GEMV for a one-row
    projection; (0, 0) where the kernel has no instantiation or did not beat the bf16 and FP8
    GEMVs (the caller then streams the bf16 image W').  DOCQA_GEMV4=0 disables."""
    S, R, lb, kw = _GEMV4_PLAN.get((N, K), (0, 0, 0, 0))
    if not _GEMV4 or M != 1 or not S or N % R or (K // S) % (64 * lb * kw):
        return 0, 0
    if (R, K // S // (64 * lb * kw), lb, kw) not in GEMV4_CASES:
        return 0, 0
    return S, R


def gemv4_cfg(N: int, K: int, splits: int = 1) -> tuple[int, int]:
    """(codes per lane per load, waves along K) the plan table uses for this shape; where it lists
    none, whole-block loads with as many waves along K as leave one chunk per lane."""
    if (N, K) in _GEMV4_PLAN and _GEMV4_PLAN[(N, K)][0] == splits:
        return _GEMV4_PLAN[(N, K)][2:]
    ks = K // max(splits, 1)
    return 32, next((w for w in (4, 2, 1) if ks % (2048 * w) == 0), 1)


def gemv4_glu_ok(M: int, N: int, K: int) -> bool:
    """The batch-1 gate|up projection with SwiGLU on the MXFP4-weight GEMV."""
    R, lb, kw = _GEMV4_EPI.get(K, (0, 0, 0))
    return bool(_GEMV4 and M == 1 and R and N % R == 0 and K % (64 * lb * kw) == 0
                and (R, K // (64 * lb * kw), lb, kw) in GEMV4_EPI_CASES)


def gemv4_argmax_ok(M: int, N: int, K: int) -> bool:
    """The batch-1 LM head + greedy pick on the MXFP4-weight GEMV."""
    return gemv4_glu_ok(M, N, K)


def gemv4_partial(x, q, e, splits: int, rows: int, lb: int = 0, kw: int = 0):
    """fp32 slabs [S, 1, N] of one row x @ W'^T on the MXFP4-weight GEMV (:func:`gemv4_plan`)."""
    if _gpu(x):
        l, k = (int(lb), int(kw)) if lb and kw else gemv4_cfg(q.shape[0], q.shape[1] * 2, splits)
        return _native().gemv4(x.contiguous(), q, e, int(splits), int(rows), l, k, False)
    return gemv_partial(x, dequantize_mxfp4_rows(q, e, x.dtype), splits, rows)


def gemv4_partial_xn(Pin, res_in, res_out, gamma, eps: float, q, e, splits: int, rows: int, lb: int = 0,
                     kw: int = 0):
    """:func:`gemv_partial_xn` (input row built in-kernel) over MXFP4 weights."""
    if _gpu(Pin):
        l, k = (int(lb), int(kw)) if lb and kw else gemv4_cfg(q.shape[0], q.shape[1] * 2, splits)
        return _native().gemv4_xn(Pin, res_in, res_out, gamma, float(eps), q, e, int(splits), int(rows), l, k, False)
    return gemv_partial_xn(Pin, res_in, res_out, gamma, eps, dequantize_mxfp4_rows(q, e, res_in.dtype), splits, rows)


def gemv4_glu(x, q, e, rows: int = 0, lb: int = 0, kw: int = 0):
    """silu(x Wg^T) * (x Wu^T) for one row over MXFP4 8-interleaved gate|up weights."""
    if _gpu(x):
        R, l, k = (int(rows), int(lb), int(kw)) if rows and lb and kw else _GEMV4_EPI.get(q.shape[1] * 2, (16, 32, 1))
        return _native().gemv4(x.contiguous(), q, e, 1, R, l, k, True)
    return gemv_glu(x, dequantize_mxfp4_rows(q, e, x.dtype))


def gemv4_glu_xn(Pin, res_in, res_out, gamma, eps: float, q, e, rows: int = 0, lb: int = 0, kw: int = 0):
    """:func:`gemv_glu_xn` (input row built in-kernel, SwiGLU epilogue) over MXFP4 weights."""
    if _gpu(Pin):
        R, l, k = (int(rows), int(lb), int(kw)) if rows and lb and kw else _GEMV4_EPI.get(q.shape[1] * 2, (16, 32, 1))
        return _native().gemv4_xn(Pin, res_in, res_out, gamma, float(eps), q, e, 1, R, l, k, True)
    return gemv_glu_xn(Pin, res_in, res_out, gamma, eps, dequantize_mxfp4_rows(q, e, res_in.dtype))


# 2..DGEMM8_MAX_ROWS-row decode steps over the same (q, s) copies (dgemm.hip dgemm8_kernel: the
# skinny kernel's LDS-DMA ring filled with codes, 256 per weight row per stage -- K slices of
# whole 1024-deep ring turns).  33+ rows are not this kernel's: there every wave of it would widen
# every B fragment, four times redundantly -- 33..128 rows have the dgemm8w family below.
DGEMM8_MAX_ROWS = 32
DGEMM8_K = 1024
_DGEMM8 = os.environ.get("DOCQA_DGEMM8", "1") != "0"
# (N, K) -> decode buckets (powers of two, engine/llm_engine.py:_bucket) whose step takes the FP8
# kernel: slab projections, the fused-SwiGLU gate|up, the LM head + argmax.  A (shape, bucket)
# pair is listed only where benchmarks/bench_dgemm_fp8.py measured the FP8 median below the
# shipped bf16 plan's with disjoint min..max window ranges (profiles/fp8_dgemm_probe.log);
# everything else keeps streaming W'.
# Llama-3-8B / Mistral-7B at M = 2 / 8 / 32, FP8 vs bf16 us: QKV 8.2 / 8.4 / 10.6 vs 11.9 / 12.2 /
# 13.4, O 6.8 / 7.1 / 8.3 vs 8.3 / 8.6 / 9.3, gate|up 25.7 / 25.1 / 30.7 vs 49.4 / 49.0 / 50.8, down
# (S = 7) 13.3 / 13.3 / 18.9 vs 21.0 / 20.5 / 22.0, LM head 94.3 / 96.2 / 122.1 vs 193.9 / 191.4 / 194.9
# (Mistral 31.3 / 32.3 / 39.2 vs 57.1 / 58.1 / 60.9) -- every bucket of every shape won.  The
# llama3-1b-test preset's rows are the suite's model: its 2048-wide QKV and O (3-6 MB of codes,
# at most 96 workgroups) are within 10 % of bf16 either way and change sides between runs --
# both stay on W'.  The (2048, 8192), (16384, 2048) and (32000, 2048) entries below are that
# preset's down, gate|up and LM head: they are listed for the suite's model, no served model has them.
_B8 = (2, 4, 8, 16, 32)
_DGEMM8_SLAB: dict = {(6144, 4096): _B8, (4096, 4096): _B8, (4096, 14336): _B8, (2048, 8192): _B8}
_DGEMM8_GLU: dict = {(28672, 4096): _B8, (16384, 2048): _B8}
_DGEMM8_LM: dict = {(128256, 4096): _B8, (32768, 4096): _B8, (32000, 2048): _B8}


def _ring_listed(on: bool, max_rows: int, granule: int, table: dict, M: int, N: int, K: int) -> bool:
    """A ring kernel's plan table lists this shape at this step's bucket."""
    if not on or not (2 <= M <= max_rows) or N % 64 or K % granule:
        return False
    return (1 << (M - 1).bit_length()) in table.get((N, K), ())


def _ring_splits(N: int, K: int, granule: int, tile: int, min_wgs: int) -> int:
    """:func:`decode_plan`'s split rule on a ring kernel's K granule: the smallest S (slices of
    whole ``granule``-deep ring turns) giving >= ``min_wgs`` workgroups, else the most slices there
    are; 0 where K is not whole ring turns."""
    if N % tile or K % granule or K < granule:
        return 0
    turns = K // granule
    cands = [S for S in range(1, turns + 1) if turns % S == 0]
    return next((S for S in cands if (N // tile) * S >= min_wgs), cands[-1])


def _dgemm8_listed(table: dict, M: int, N: int, K: int) -> bool:
    return _ring_listed(_DGEMM8, DGEMM8_MAX_ROWS, DGEMM8_K, table, M, N, K)


def dgemm8_splits(N: int, K: int, tile: int = 64, min_wgs: int = 192) -> int:
    """:func:`decode_plan`'s split rule on the FP8 ring's K granule: the smallest S (slices of
    whole 1024-deep ring turns) giving >= ``min_wgs`` workgroups, else the most slices there
    are; 0 where K is not whole ring turns."""
    return _ring_splits(N, K, DGEMM8_K, tile, min_wgs)


def dgemm8_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the FP8-weight ring kernel for a 2..32-row
    decode projection; (0, 64) where the shape has no instantiation or the probe did not show it
    faster than the bf16 plan (the caller then streams W').  DOCQA_DGEMM8=0 disables."""
    if not _dgemm8_listed(_DGEMM8_SLAB, M, N, K):
        return 0, 64
    return dgemm8_splits(N, K), 64


def dgemm8_glu_ok(M: int, N: int, K: int) -> bool:
    """The 2..32-row gate|up projection with SwiGLU on the FP8-weight ring kernel."""
    return _dgemm8_listed(_DGEMM8_GLU, M, N, K)


def dgemm8_argmax_ok(M: int, N: int, K: int) -> bool:
    """The 2..32-row LM head + greedy pick on the FP8-weight ring kernel."""
    return _dgemm8_listed(_DGEMM8_LM, M, N, K)


def dgemm8_partial(x, q, s, splits: int, tile_rows: int = 64):
    """fp32 slabs [S, M, N] of x @ (q * s)^T for 2..32 rows on the FP8-weight ring kernel
    (:func:`dgemm8_plan`)."""
    if _gpu(x):
        return _native().dgemm8_partial(x.contiguous(), q, s, int(splits), int(tile_rows))
    return dgemm_partial(x, dequantize_fp8_rows(q, s, x.dtype), splits, tile_rows)


def dgemm8_glu(x, q, s):
    """silu(x Wg^T) * (x Wu^T) for 2..32 rows over FP8 8-interleaved gate|up weights."""
    if _gpu(x):
        return _native().dgemm8_glu(x.contiguous(), q, s)
    return glu_linear(x, dequantize_fp8_rows(q, s, x.dtype))


# 33..DGEMM8W_MAX_ROWS-row decode steps over the same (q, s) copies (dgemm.hip dgemm8w_kernel: waves
# own the n-tiles of a 128-row weight tile, so a code is widened once per workgroup; X staged
# through LDS next to the codes; K slices of whole 512-deep turns).  129+ rows stay on W'.
DGEMM8W_MAX_ROWS = 128
DGEMM8W_K = 512
DGEMM8W_TILE = 128
_DGEMM8W = os.environ.get("DOCQA_DGEMM8W", "1") != "0"
# (N, K) -> decode buckets whose step takes the wide FP8 kernel: slab projections (bucket ->
# (split-K count, weight rows per workgroup), as _DGEMM4_SLAB), the fused-SwiGLU gate|up, the LM
# head + argmax.  A (shape, bucket) pair is listed only where benchmarks/bench_dgemm_fp8_wide.py
# measured the FP8 median below the shipped bf16 plan's (decode_plan / mid_plan, the mid-M LM head +
# argmax; a slab projection whose split count differs from bf16's timed together with its consumer)
# with disjoint min..max window ranges, in BOTH runs of profiles/fp8_wide_dgemm_probe.log.  Served
# model shapes only: the test presets' shapes are never listed (tests patch the tables).
# Llama-3-8B / Mistral-7B at M = 64 / 128, FP8 vs bf16 us (second run): gate|up 30.7 / 46.4 vs 52.8 /
# 61.6 (glu_linear), LM head 132.3 / 192.8 vs 256.0 / 262.2 (Mistral 40.4 / 55.5 vs 108.5 / 110.0; the
# mid-M LM head + argmax), down at S = 7 with add_rmsnorm_splitk 24.8 / 36.1 vs 31.7 / 46.0 (bf16: S = 4,
# 64-row tiles; alone 18.4 / 30.9 vs 26.7 / 39.8), QKV at S = 4: bucket 64 with rope_cache_splitk 17.6 vs
# 20.1 (bf16: S = 2), bucket 128 alone 20.5 vs 22.4 (bf16: S = 4 too).  65..128 rows (eight m-tiles
# per B fragment, a 3-slot ring) are the slower instantiation: 43.2 us at 65 rows against 30.7 at 64 for
# gate|up -- still ahead of bf16 everywhere listed.
# Loser, which stays on W': O 4096 x 4096 at both buckets -- 32 tiles of 128 rows need S = 8 to fill
# the chip, and the consumer then reads twice the slabs: 17.3 / 25.4 us with add_rmsnorm_splitk vs 16.3 /
# 22.7; at bf16's own S = 4 alone 12.1 / 19.2 vs 12.0 / 16.8.
_DGEMM8W_SLAB: dict = {(6144, 4096): {64: (4, 128), 128: (4, 128)},
                       (4096, 14336): {64: (7, 128), 128: (7, 128)}}
_DGEMM8W_GLU: dict = {(28672, 4096): (64, 128)}
_DGEMM8W_LM: dict = {(128256, 4096): (64, 128), (32768, 4096): (64, 128)}


def _dgemm8w_listed(table: dict, M: int, N: int, K: int) -> bool:
    if not _DGEMM8W or not (DGEMM8_MAX_ROWS < M <= DGEMM8W_MAX_ROWS) or N % DGEMM8W_TILE or K % DGEMM8W_K:
        return False
    return (1 << (M - 1).bit_length()) in table.get((N, K), ())


def dgemm8w_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the wide FP8-weight kernel for a 33..128-row
    decode projection; (0, 128) where the shape has no instantiation, the table's split does not
    cut K into whole 512-deep turns, or the probe did not show it faster than the bf16 plan (the
    caller then streams W').  DOCQA_DGEMM8W=0 disables."""
    if not _dgemm8w_listed(_DGEMM8W_SLAB, M, N, K):
        return 0, DGEMM8W_TILE
    S, t = _DGEMM8W_SLAB[(N, K)][1 << (M - 1).bit_length()]
    if S < 1 or t != DGEMM8W_TILE or K % S or (K // S) % DGEMM8W_K:
        return 0, DGEMM8W_TILE
    return S, t


def dgemm8w_glu_ok(M: int, N: int, K: int) -> bool:
    """The 33..128-row gate|up projection with SwiGLU on the wide FP8-weight kernel."""
    return _dgemm8w_listed(_DGEMM8W_GLU, M, N, K)


def dgemm8w_argmax_ok(M: int, N: int, K: int) -> bool:
    """The 33..128-row LM head + greedy pick on the wide FP8-weight kernel."""
    return _dgemm8w_listed(_DGEMM8W_LM, M, N, K)


def dgemm8w_partial(x, q, s, splits: int, tile_rows: int = DGEMM8W_TILE):
    """fp32 slabs [S, M, N] of x @ (q * s)^T for 33..128 rows on the wide FP8-weight kernel
    (:func:`dgemm8w_plan`)."""
    if _gpu(x):
        return _native().dgemm8w_partial(x.contiguous(), q, s, int(splits), int(tile_rows))
    return dgemm_partial(x, dequantize_fp8_rows(q, s, x.dtype), splits, tile_rows)


def dgemm8w_glu(x, q, s):
    """silu(x Wg^T) * (x Wu^T) for 33..128 rows over FP8 8-interleaved gate|up weights."""
    if _gpu(x):
        return _native().dgemm8w_glu(x.contiguous(), q, s)
    return glu_linear(x, dequantize_fp8_rows(q, s, x.dtype))


# 2..DGEMM4_MAX_ROWS-row decode steps over the MXFP4 (q, e) copies (dgemm.hip dgemm4_kernel: the
# same ring, 512 codes per weight row per stage -- K slices of whole 2048-deep ring turns, block
# scales applied while widening; slab tiles of 64, 32 or 16 weight rows).  33+ rows stay on W':
# the wide kernel (dgemm8w) is FP8 only.
DGEMM4_MAX_ROWS = 32
DGEMM4_K = 2048
_DGEMM4 = os.environ.get("DOCQA_DGEMM4", "1") != "0"
# (N, K) -> decode buckets (powers of two, engine/llm_engine.py:_bucket) whose step takes the MXFP4
# ring kernel: slab projections (bucket -> (split-K count, weight rows per workgroup); a plain
# tuple of buckets means ops.dgemm4_splits at 64 rows), the fused-SwiGLU gate|up, the LM head +
# argmax.  A (shape, bucket) pair is listed only where benchmarks/bench_dgemm_mxfp4.py measured the
# listed variant's median below the shipped bf16 plan's with disjoint min..max window ranges, in
# BOTH runs of profiles/mxfp4_dgemm_probe.log.  The comparison is against bf16 only: inside an
# MXFP4 model W' is the only alternative (the log's FP8 column is for the README).  Everything
# else keeps streaming W'.
# Llama-3-8B / Mistral-7B at M = 2 / 8 / 16, MXFP4 vs bf16 us (second run): QKV (32-row tiles, S = 1:
# 192 workgroups where 64-row tiles give 96 x 2) 7.2 / 8.4 / 10.1 vs 12.2 / 12.5 / 12.6, O (32-row
# tiles, S = 2: 256 workgroups, 64-row tiles only 128) 6.2 / 6.7 vs 8.9 / 8.7, gate|up 19.2 /
# 21.0 / 23.3 vs 48.5 / 47.5 / 48.0 (31.7 vs 49.5 at 32), down (S = 7) 13.7 / 15.2 / 19.1 vs 21.2 /
# 21.1 / 20.9, LM head 70.5 / 84.2 / 107.4 vs 190.9 / 187.4 / 188.4 (145.1 vs 192.6 at 32; Mistral
# 24.8 / 28.1 / 33.8 / 43.7 vs 57.3 / 58.0 / 58.7 / 59.9).
# Losers, which stay on W': every slab projection at bucket 32 (two m-tiles: each of the two
# k-groups widens every fragment again; QKV 14.2 vs 13.7, O 10.8 vs 9.7, down 22.8 vs 21.9) and O
# at bucket 16 (7.7 vs 8.9 in the median, but one window of the second run reached into bf16's
# range).  The llama3-1b-test preset's rows are the suite's model, no served model has them: its
# O 2048 x 2048 lost or tied everywhere (5.4 vs 5.4 at 8) and stays on W'; its QKV 3072 x 2048
# won at buckets 4 and 8 only (5.4 / 5.8 vs 6.0 / 6.2), its down 2048 x 8192 at 2, 4 and 16 (bucket
# 8: 7.2 vs 9.3, one outlier window overlapping).
_B4 = (2, 4, 8, 16, 32)
_DGEMM4_SLAB: dict = {(6144, 4096): {b: (1, 32) for b in (2, 4, 8, 16)},
                      (4096, 4096): {b: (2, 32) for b in (2, 4, 8)},
                      (4096, 14336): {b: (7, 64) for b in (2, 4, 8, 16)},
                      (3072, 2048): {b: (1, 32) for b in (4, 8)},
                      (2048, 8192): {b: (4, 32) for b in (2, 4, 16)}}
_DGEMM4_GLU: dict = {(28672, 4096): _B4, (16384, 2048): _B4}
_DGEMM4_LM: dict = {(128256, 4096): _B4, (32768, 4096): _B4, (32000, 2048): _B4}


def _dgemm4_listed(table: dict, M: int, N: int, K: int) -> bool:
    return _ring_listed(_DGEMM4, DGEMM4_MAX_ROWS, DGEMM4_K, table, M, N, K)


def dgemm4_splits(N: int, K: int, tile: int = 64, min_wgs: int = 192) -> int:
    """:func:`dgemm8_splits` on the MXFP4 ring's K granule: the smallest S (slices of whole
    2048-deep ring turns) giving >= ``min_wgs`` workgroups, else the most slices there are; 0
    where K is not whole ring turns."""
    return _ring_splits(N, K, DGEMM4_K, tile, min_wgs)


def dgemm4_plan(M: int, N: int, K: int) -> tuple[int, int]:
    """(split-K count, weight rows per workgroup) of the MXFP4-weight ring kernel for a 2..32-row
    decode projection; (0, 64) where the shape has no instantiation or the probe did not show it
    faster than the bf16 plan (the caller then streams W').  DOCQA_DGEMM4=0 disables."""
    if not _dgemm4_listed(_DGEMM4_SLAB, M, N, K):
        return 0, 64
    entry = _DGEMM4_SLAB[(N, K)]
    if isinstance(entry, dict):      # bucket -> (split-K count, tile rows) the probe picked
        return entry[1 << (M - 1).bit_length()]
    return dgemm4_splits(N, K), 64


def dgemm4_glu_ok(M: int, N: int, K: int) -> bool:
    """The 2..32-row gate|up projection with SwiGLU on the MXFP4-weight ring kernel."""
    return _dgemm4_listed(_DGEMM4_GLU, M, N, K)


def dgemm4_argmax_ok(M: int, N: int, K: int) -> bool:
    """The 2..32-row LM head + greedy pick on the MXFP4-weight ring kernel."""
    return _dgemm4_listed(_DGEMM4_LM, M, N, K)


def dgemm4_partial(x, q, e, splits: int, tile_rows: int = 64):
    """fp32 slabs [S, M, N] of x @ W'^T for 2..32 rows on the MXFP4-weight ring kernel
    (:func:`dgemm4_plan`)."""
    if _gpu(x):
        return _native().dgemm4_partial(x.contiguous(), q, e, int(splits), int(tile_rows))
    return dgemm_partial(x, dequantize_mxfp4_rows(q, e, x.dtype), splits, tile_rows)


def dgemm4_glu(x, q, e):
    """silu(x Wg^T) * (x Wu^T) for 2..32 rows over MXFP4 8-interleaved gate|up weights."""
    if _gpu(x):
        return _native().dgemm4_glu(x.contiguous(), q, e)
    return glu_linear(x, dequantize_mxfp4_rows(q, e, x.dtype))


# ----------------------------------------------------------------- streamed-weight dispatch
class StreamedFormat(NamedTuple):
    """One streamed weight format: a quantized copy (a pair of tensors per weight) next to its exact
    bf16 image W', read by a one-row GEMV, a 2..32-row ring kernel and, where the format has one,
    a wide kernel for the rows above (max_rows: the most rows any of them takes).  Every per-format
    function is named <kernel family>_<role> (gemv8_plan, dgemm4_glu_ok, gemv4_partial_xn ...) and
    looked up on this module when called: tests spy on the wrappers and patch the plan tables."""
    quantize: Callable
    dequantize: Callable
    max_rows: int
    gemv: str          # kernel family of one-row steps
    ring: str          # kernel family of 2..32-row steps
    gemv_epi: str      # table K -> launch arguments of the GEMV's SwiGLU / argmax epilogues
    wide: str = ""     # kernel family of the steps above the ring kernel's rows; "": none


STREAMED = {"fp8-e4m3": StreamedFormat(quantize_fp8_rows, dequantize_fp8_rows, DGEMM8W_MAX_ROWS,
                                       "gemv8", "dgemm8", "_GEMV8_EPI", "dgemm8w"),
            "mxfp4": StreamedFormat(quantize_mxfp4_rows, dequantize_mxfp4_rows, DGEMM4_MAX_ROWS,
                                    "gemv4", "dgemm4", "_GEMV4_EPI")}
_KINDS = ("gemv", "ring", "wide")      # the order they are tried in


def _kinds(fmt: str) -> tuple:
    """The kernel kinds format ``fmt`` has, in the order they are tried."""
    return tuple(k for k in _KINDS if getattr(STREAMED[fmt], k))


def _streamed_fn(fmt: str, kind: str, role: str):
    return globals()[f"{getattr(STREAMED[fmt], kind)}_{role}"]


def streamed_plan(fmt: str, M: int, N: int, K: int) -> tuple[str, int, int]:
    """(kind, split-K count, weight rows per workgroup) of an M-row slab projection over the
    streamed copy, kind "gemv", "ring" or "wide"; ("", 0, 0) where no plan lists the shape (the
    caller then streams the bf16 image W')."""
    for kind in _kinds(fmt):
        S, R = _streamed_fn(fmt, kind, "plan")(M, N, K)
        if S:
            return kind, S, R
    return "", 0, 0


def streamed_glu_kind(fmt: str, M: int, N: int, K: int) -> str:
    """:func:`streamed_plan`'s kind for the gate|up projection with SwiGLU."""
    return next((kind for kind in _kinds(fmt) if _streamed_fn(fmt, kind, "glu_ok")(M, N, K)), "")


def streamed_partial(fmt: str, kind: str, x, w, splits: int, rows: int):
    """fp32 slabs [S, M, N] of x @ W'^T from the streamed pair ``w`` (:func:`streamed_plan`)."""
    return _streamed_fn(fmt, kind, "partial")(x, *w, splits, rows)


def streamed_partial_xn(fmt: str, kind: str, Pin, res_in, res_out, gamma, eps: float, w, splits: int, rows: int):
    """:func:`streamed_partial` with the input row built in-kernel (:func:`gemv_partial_xn`)."""
    return _streamed_fn(fmt, kind, "partial_xn")(Pin, res_in, res_out, gamma, eps, *w, splits, rows)


def streamed_glu(fmt: str, kind: str, x, w):
    """silu(x Wg^T) * (x Wu^T) from the streamed pair ``w`` (:func:`streamed_glu_kind`)."""
    return _streamed_fn(fmt, kind, "glu")(x, *w)


def streamed_glu_xn(fmt: str, kind: str, Pin, res_in, res_out, gamma, eps: float, w):
    """:func:`streamed_glu` with the input row built in-kernel (:func:`gemv_glu_xn`)."""
    return _streamed_fn(fmt, kind, "glu_xn")(Pin, res_in, res_out, gamma, eps, *w)



NORM_FUSE_ROWS = 4
# off by default: the last-workgroup add + RMSNorm tail (one workgroup reading every slab at
# agent scope) costs more than the add_rmsnorm_splitk launch it replaces -- batch-1 p50
# 511.5 ms with it vs 492.0 without (profiles/r4_b1_ab.log)
_NORM_FUSE = os.environ.get("DOCQA_DGEMM_NORM", "0") == "1"


def dgemm_norm_plan(M: int, N: int, K: int) -> int:
    """Split count of the few-row projection with the residual add + RMSNorm fused into its
    last workgroup (dgemm.hip NormArgs), 0 where it does not apply (more than
    NORM_FUSE_ROWS rows, N > 8192, no skinny-kernel plan, DOCQA_DGEMM_NORM=0)."""
    if not _NORM_FUSE or not (0 < M <= NORM_FUSE_ROWS) or N > 8192 or N % 64:
        return 0
    S, t = decode_plan(M, N, K)
    return S if t == 64 else 0


def dgemm_add_rmsnorm(x, w, splits: int, residual, gamma, eps: float, tick):
    """residual <- residual + bf16(x @ w^T); returns rmsnorm(residual) * gamma -- the
    split-K projection and the add + norm in one launch (few rows, :func:`dgemm_norm_plan`).
    ``tick``: one zeroed int32 word (the kernel re-arms it)."""
    if _gpu(x):
        return _native().dgemm_add_rmsnorm(x.contiguous(), w, int(splits), residual, gamma, float(eps), tick)
    y = torch.nn.functional.linear(x.float(), w.float()).to(residual.dtype)
    return ref.add_rmsnorm(y, residual, gamma, eps)


def add_rmsnorm_splitk(P, residual, w, eps: float):
    """residual <- residual + bf16(sum_s P[s]); returns rmsnorm(residual) * w."""
    if _gpu(P):
        return _native().add_rmsnorm_splitk(P, residual, w, eps)
    return ref.add_rmsnorm(P.float().sum(0).to(residual.dtype).view_as(residual), residual, w, eps)


def paged_decode_fused(P, positions, cos_sin, slot_mapping, k_cache, v_cache, block_tables,
                       context_lens, Hq, max_context, scale, order=None, tick=None):
    """Decode attention straight from the QKV projection's split-K partial slabs: RoPE,
    paged-cache write of the new token and attention in one launch (attn_decode.hip ring
    kernel, FUSED mode).  Same result as rope_cache_splitk + paged_decode.
    ``tick``: a zeroed int32 buffer of >= B x Hkv entries (:func:`decode_ticket`) -- split
    context partitions are then merged by their last workgroup, no second launch."""
    if _gpu(P):
        return _native().paged_decode_fused(P, positions, cos_sin, slot_mapping, k_cache, v_cache,
                                            block_tables, context_lens, Hq, max_context, scale, order,
                                            tick)
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    qkv = rope_cache_splitk(P, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)
    return ref.paged_decode(qkv, k_cache, v_cache, block_tables, context_lens, Hq, max_context, scale)


_LAST_MERGE = os.environ.get("DOCQA_DECODE_LAST_MERGE", "1") != "0"


def decode_ticket(n: int, device) -> torch.Tensor | None:
    """Zeroed int32 ticket words for the last-arriver partition merge of the decode
    attention kernels (one per sequence x KV head; the kernel re-arms them).  None when
    DOCQA_DECODE_LAST_MERGE=0 (separate reduce launch)."""
    if not _LAST_MERGE:
        return None
    return torch.zeros(n, dtype=torch.int32, device=device)


KV_FP8 = ref.KV_FP8     # dtype of an FP8 paged KV cache (OCP e4m3 codes, no scales)
kv_fp8_codes = ref.kv_fp8_codes


def kv_is_fp8(k_cache) -> bool:
    return k_cache.dtype == KV_FP8


def kv_fp8_shape_ok(Hq: int, Hkv: int, D: int, BS: int) -> bool:
    """Shapes the FP8-KV kernels cover on the GPU: head_dim 128, 64-token blocks, 4 or 8 query
    heads per KV head."""
    return D == 128 and BS == 64 and Hkv > 0 and Hq in (4 * Hkv, 8 * Hkv)


def fused_decode_ok(k_cache, block_tables) -> bool:
    """Shapes the fused decode attention kernel supports (head_dim 128, 64-token blocks,
    <= 256 blocks per sequence; bf16 caches only -- an FP8 cache takes rope_cache_splitk +
    paged_decode)."""
    if kv_is_fp8(k_cache):
        return False
    return k_cache.shape[2] == 64 and k_cache.shape[3] == 128 and block_tables.shape[1] <= 256


def rope_cache_splitk(P, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D):
    """Packed bf16 QKV <- rope(bf16(sum_s P[s])) with the paged-cache write (rope_cache)."""
    if _gpu(P):
        if slot_mapping is None:
            k_cache = v_cache = P
        return _native().rope_cache_splitk(P, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)
    # the model dtype: bf16 on the GPU path, fp32 for CPU reference models
    dt = k_cache.dtype if slot_mapping is not None and not kv_is_fp8(k_cache) else torch.bfloat16
    qkv = P.float().sum(0).to(dt)
    ref.rope_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)
    return qkv


# ----------------------------------------------------------------------------- embeddings
def embedding(ids, table):
    if _gpu(table):
        return _native().embedding(ids, table)
    return ref.embedding(ids, table)


def bert_embed_ln(ids, pos, token_type, wte, wpe, wtt, gamma, beta, eps):
    if _gpu(wte):
        return _native().bert_embed_ln(ids.contiguous(), pos.contiguous(), token_type, wte, wpe, wtt, gamma, beta,
                                       eps)
    return ref.bert_embed_ln(ids, pos, token_type, wte, wpe, wtt, gamma, beta, eps)


# ----------------------------------------------------------------------------- sampling
def decode_slots(block_tables, positions, valid, BS: int):
    """Paged-cache slot of each decode row's next token, -1 for padded rows."""
    if _gpu(block_tables):
        return _native().decode_slots(block_tables, positions, valid, BS)
    return ref.decode_slots(block_tables, positions, valid, BS)


def decode_advance(nxt, out, tokens, positions, context_lens, valid) -> None:
    """In place: out <- nxt, tokens <- nxt, positions / context_lens += valid."""
    if _gpu(nxt):
        _native().decode_advance(nxt, out, tokens, positions, context_lens, valid)
        return
    ref.decode_advance(nxt, out, tokens, positions, context_lens, valid)


def argmax(logits):
    if _gpu(logits):
        return _native().argmax(logits)
    return ref.argmax(logits)


def token_cls_argmax(h, w, bias, n_valid: int):
    """Fused token-classification head + argmax: argmax_n(h @ w[:n_valid].T + bias)."""
    if _gpu(h):
        return _native().token_cls_argmax(h, w, bias, int(n_valid))
    return ref.token_cls_argmax(h, w, bias, n_valid)


def sample(logits, inv_temp, top_k, top_p, u):
    """One token id per row of ``logits`` [rows, V] from temperature / top-k / top-p sampling.

    ``inv_temp``, ``top_p``, ``u`` are fp32 and ``top_k`` int32, one entry per row (contiguous,
    on the logits' device, at least ``rows`` long: a longer bucket-sized tensor is fine).  Per row,
    with ``x = float32(logit) * inv_temp``:

    * top-k (``0 < top_k < V``) keeps ``x >=`` the k-th largest value; ties at that value are all kept.
    * top-p (``0 < top_p < 1``) then keeps, of the survivors by descending probability, the shortest
      prefix whose mass reaches ``top_p`` of theirs; ties at the cutoff value are all kept.
    * The draw is the inverse CDF of the kept tokens **in vocabulary-index order** at ``u`` in
      [0, 1): the first kept token whose cumulative share exceeds ``u``.  A dropped token is never
      returned.
    * ``top_k == 1`` is an argmax: the lowest index of the maximum of ``x``, whatever ``u`` and
      ``top_p`` are -- the tie rule of every greedy path, so on the same logits a greedy row gets the
      same token inside a sampled batch as alone.

    Logits are expected finite (NaN / inf are not handled: the thresholds are searched over the
    row's [min, max] range) and ``inv_temp`` positive.
    """
    if _gpu(logits):
        return _native().sample(logits.float().contiguous(), inv_temp, top_k, top_p, u)
    return ref.sample(logits, inv_temp, top_k, top_p, u)


def seeded_uniform(seed, index):
    """Counter-based uniforms: fp32 [R] in [0, 1) from ``seed`` int64 [R] and ``index`` int32 [R].
    Philox4x32-10 with key ``(seed & 0xffffffff, seed >> 32)`` and counter ``(index, 0, 0, 0)``;
    of the first output word ``w0``, ``u = float(w0 >> 8) * 2^-24`` (exact in fp32, at most
    ``1 - 2^-24``).  ``index`` is the absolute position, in prompt + output, of the token the
    uniform draws, so a request's stream depends on its seed alone: not on its slot, its
    neighbours, a preemption or the process's generator.  GPU and CPU agree bit for bit."""
    if _gpu(seed):
        return _native().seeded_uniform(seed.contiguous(), index.contiguous())
    return ref.seeded_uniform(seed, index)


def sample_tokens(logits, n_valid: int, inv_temp, top_k, top_p, min_p, *, u=None, seed=None, index=None,
                  valid=None):
    """One token id per row (int64 [R]) of ``logits`` [R, ld], bf16 or fp32, read as they are --
    on a GPU once, with no fp32 copy (csrc/kernels/sample.hip); columns at or past ``n_valid``
    take no part.  Any row stride and alignment is served: bf16 rows that the 16-byte loads cannot
    take (``ld % 8``, a misaligned base, more than 131072 columns) and fp32 rows run the same
    code over memory.

    Temperature, top-k, top-p and the draw are the contract of :func:`sample` with
    ``x = float32(logit) * inv_temp``: ties at a cutoff are all kept, ``top_k == 1`` is the lowest
    index of the maximum whatever the other parameters are, and the draw is the inverse CDF of the
    kept tokens in index order.  ``min_p`` (fp32 [R], or None): ``0 < min_p <= 1`` keeps, in
    addition, only ``x >= max(x) + log(min_p)``, i.e. ``p_i >= min_p * p_max`` -- a ratio no
    other filter changes, as the maximum survives them all; ``min_p <= 0`` is off.

    The row's uniform is exactly one of ``u`` (fp32 [R], the caller's) and ``seed`` int64 [R] +
    ``index`` int32 [R] (:func:`seeded_uniform`, computed inside the kernel).  Rows with
    ``valid == 0`` (int32 [R], padding slots) write token 0 and read nothing.  Per-row tensors
    are contiguous, on the logits' device and at least R long."""
    if (u is None) == (seed is None) or (seed is None) != (index is None):
        raise ValueError("sample_tokens: exactly one of u and seed + index")
    if _gpu(logits):
        return _native().sample_tokens(logits, int(n_valid), inv_temp, top_k, top_p, min_p, u, seed, index, valid)
    return ref.sample_tokens(logits, int(n_valid), inv_temp, top_k, top_p, min_p, u, seed, index, valid)


PENALTY_WINDOW = ref.PENALTY_WINDOW   # capacity W of the per-slot token ring hist [B, W]


def apply_penalties(logits, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid=None) -> None:
    """In place on fp32 logits [R, V]: llama.cpp's repeat / presence / frequency penalties over
    each row's newest min(hist_n, last_n, W) ring tokens -- per distinct token t with count c,
    l = l <= 0 ? l * rp : l / rp, then l -= c * fp + pp (fp32, each operation rounded on its
    own: GPU and reference agree bitwise).  Neutral rows (rp 1, pp 0, fp 0, or last_n 0) and
    rows with valid 0 are left untouched."""
    if _gpu(logits):
        _native().apply_penalties(logits, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid)
        return
    ref.apply_penalties(logits, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid)


def penalized_argmax(logits, n_valid: int, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid=None):
    """Greedy pick under the penalties of :func:`apply_penalties`: int64 [R], the argmax over
    t < n_valid of the penalised bf16 / fp32 logits [R, V], ties to the lowest index.  On a GPU
    the logits are read once, no fp32 copy is made and ``logits`` is CLOBBERED (the window
    tokens' entries are overwritten); logits are expected to be finite."""
    if _gpu(logits):
        return _native().penalized_argmax(logits, int(n_valid), hist, hist_n, last_n, rep_pen, pres_pen,
                                          freq_pen, valid)
    return ref.penalized_argmax(logits, n_valid, hist, hist_n, last_n, rep_pen, pres_pen, freq_pen, valid)


TOP_LOGPROBS_MAX = ref.TOP_LOGPROBS_MAX   # columns of the top list of :func:`token_logprobs`


def token_logprobs(logits, n_valid: int, chosen, top_n, lp=None, top_ids=None, top_lp=None):
    """Per-token log-probabilities of the LM-head logits [R, ld] (bf16 or fp32, read as they are):
    ``logprob(t) = logit[t] - logsumexp(logit[0:n_valid])``; columns at or past ``n_valid`` take
    no part.  ``chosen`` [R] int64 is the picked token of each row, ``top_n`` [R] int32 what the
    row wants: -1 nothing (none of its outputs is written), 0 the chosen token's logprob, 1..20
    also that many most likely tokens.  Returns ``(lp [R] fp32, top_ids [R, 20] int32, top_lp
    [R, 20] fp32)``, written into the caller's buffers where given (a decode graph's static slot
    buffers; fresh ones are filled with the -1 row's sentinels 0 / -1 / -inf).  The top list is
    in descending order, ties to the lower id; entries past ``top_n`` or past the vocabulary are
    (-1, -inf).  On a GPU (csrc/kernels/logprobs.hip) the row stride must be a multiple of 16
    bytes and bf16 logits need ``n_valid % 8 == 0``; logits are expected finite."""
    R, dev = logits.shape[0], logits.device
    if lp is None:
        lp = torch.zeros(R, dtype=torch.float32, device=dev)
    if top_ids is None:
        top_ids = torch.full((R, TOP_LOGPROBS_MAX), -1, dtype=torch.int32, device=dev)
    if top_lp is None:
        top_lp = torch.full((R, TOP_LOGPROBS_MAX), float("-inf"), dtype=torch.float32, device=dev)
    if _gpu(logits):
        _native().token_logprobs(logits, int(n_valid), chosen, top_n, lp, top_ids, top_lp)
    else:
        ref.token_logprobs(logits, int(n_valid), chosen, top_n, lp, top_ids, top_lp)
    return lp, top_ids, top_lp


def grammar_mask(logits, n_valid: int, state, tok_off, tok_bytes, table, eos_id: int, valid=None) -> None:
    """Grammar-constrained decoding (:mod:`docqa_amd.ops.grammar`, csrc/kernels/grammar.hip): in
    place on bf16 / fp32 logits [R, ld], every row with ``state != 0`` (int64 [R], the row's
    automaton state) and ``valid != 0`` gets ``-inf`` in each column ``t < n_valid`` whose token is
    not allowed: allowed is a token with bytes (``tok_off`` int32 [V + 1] into ``tok_bytes``
    uint8) that walk from the state through ``table`` (int16 [states, 256]) without a reject, or
    ``t == eos_id`` in DONE -- EOS is never allowed before DONE, a token without bytes or past
    the byte table never.  Allowed columns, columns at or past ``n_valid`` and skipped rows are
    left bit for bit; no logit is read."""
    if _gpu(logits):
        _native().grammar_mask(logits, int(n_valid), state, tok_off, tok_bytes, table, int(eos_id), valid)
        return
    ref.grammar_mask(logits, int(n_valid), state, tok_off, tok_bytes, table, int(eos_id), valid)


def grammar_advance(state, nxt, tok_off, tok_bytes, table, eos_id: int, valid=None) -> None:
    """In place on ``state`` int64 [R]: the automaton after the bytes of the picked token
    ``nxt`` (int64 [R]).  State 0 stays 0, DONE stays DONE (the extra lagged step of a finished
    request picks EOS again), EOS leaves the state as it is, and so does a token that would be
    rejected (defensive: it cannot occur behind :func:`grammar_mask`).  GPU and CPU agree as
    int64."""
    if _gpu(state):
        _native().grammar_advance(state, nxt, tok_off, tok_bytes, table, int(eos_id), valid)
        return
    ref.grammar_advance(state, nxt, tok_off, tok_bytes, table, int(eos_id), valid)


def schema_mask(logits, n_valid: int, sstate, tok_off, tok_bytes, pool, eos_id: int, valid=None) -> None:
    """JSON-schema structured outputs (:mod:`docqa_amd.ops.json_schema`,
    csrc/kernels/grammar_schema.hip): :func:`grammar_mask`'s contract with a per-row automaton.
    In place on bf16 / fp32 logits [R, ld], every row with ``sstate != 0`` (int64 [R]: DFA state,
    whitespace run and table slot) and ``valid != 0`` gets ``-inf`` in each column ``t < n_valid``
    whose token is not allowed: allowed is a token with bytes that walk from the row's state
    through the ``cls`` / ``trans`` tables of the row's slot of ``pool`` (uint8 [slots,
    json_schema.SLOT_BYTES]) without a reject, or ``t == eos_id`` in DONE.  A slot past the pool
    or with a header out of range allows nothing.  Allowed columns, columns at or past ``n_valid``
    and skipped rows are left bit for bit; no logit is read."""
    if _gpu(logits):
        _native().schema_mask(logits, int(n_valid), sstate, tok_off, tok_bytes, pool, int(eos_id), valid)
        return
    ref.schema_mask(logits, int(n_valid), sstate, tok_off, tok_bytes, pool, int(eos_id), valid)


def schema_advance(sstate, nxt, tok_off, tok_bytes, pool, eos_id: int, valid=None) -> None:
    """In place on ``sstate`` int64 [R]: the word after the bytes of the picked token ``nxt``
    (int64 [R]) walked through the row's slot of ``pool``.  Word 0 stays 0, DONE stays DONE, EOS
    leaves the word as it is, and so does a token that would be rejected or has no bytes.  GPU
    and CPU agree as int64."""
    if _gpu(sstate):
        _native().schema_advance(sstate, nxt, tok_off, tok_bytes, pool, int(eos_id), valid)
        return
    ref.schema_advance(sstate, nxt, tok_off, tok_bytes, pool, int(eos_id), valid)


def decode_advance_hist(nxt, out, tokens, positions, context_lens, valid, hist, hist_n) -> None:
    """:func:`decode_advance`, and the valid rows' new token joins their ring:
    hist[i, hist_n[i] % W] <- nxt[i], hist_n[i] += 1."""
    if _gpu(nxt):
        _native().decode_advance_hist(nxt, out, tokens, positions, context_lens, valid, hist, hist_n)
        return
    ref.decode_advance_hist(nxt, out, tokens, positions, context_lens, valid, hist, hist_n)


# ----------------------------------------------------------------------------- attention
def paged_decode(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context, scale, order=None):
    """``order``: optional int32 permutation of the rows -- the workgroup dispatch order
    (longest context first); results do not depend on it."""
    if _gpu(q):
        return _native().paged_decode(q, k_cache, v_cache, block_tables, context_lens, Hq,
                                      max_context, scale, order)
    return ref.paged_decode(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context, scale)


def cascade_ok(k_cache, block_tables, Hq: int) -> bool:
    """Shapes the cascade (shared-prefix) decode path supports: Llama-3 GQA (4 query heads
    per KV head), head_dim 128, 64-token blocks, <= 256 blocks per sequence (the CPU
    reference path takes any GQA shape)."""
    if not _gpu(k_cache):
        return Hq % k_cache.shape[1] == 0
    if kv_is_fp8(k_cache):
        return False        # the shared-prefix kernels read bf16 caches only
    return (k_cache.shape[2] == 64 and k_cache.shape[3] == 128 and Hq == 4 * k_cache.shape[1]
            and block_tables.shape[1] <= 256)


def paged_decode_cascade_rope(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, block_tables,
                              context_lens, Hq, max_context, scale, prefix_table, prefix_len,
                              nchunk: int = 8, order=None):
    """Cascade decode over the unrotated packed QKV rows of a library GEMM: RoPE, the new
    token's paged-cache write and the attention inside the cascade kernels (the prefix
    kernel rotates queries on load, the ring kernel rotates its queries and writes / attends
    the new K/V from registers).  ``qkv`` may be rotated in place (fallback path)."""
    if _gpu(qkv):
        return _native().paged_decode_cascade_rope(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache,
                                                   block_tables, context_lens, Hq, max_context, scale,
                                                   prefix_table, prefix_len, nchunk, order)
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    ref.rope_cache(qkv, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)
    return ref.paged_decode_cascade(qkv, k_cache, v_cache, block_tables, context_lens, Hq, max_context,
                                    scale, prefix_table, prefix_len, nchunk)


def paged_decode_cascade(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context, scale,
                         prefix_table, prefix_len, nchunk: int = 8, order=None):
    """Decode attention with the batch's shared prompt prefix attended once for all rows
    (csrc/include/docqa_cascade.h): keys [0, prefix_len) from ``prefix_table``, keys
    [prefix_len, L) from each row's block table.  Same result as :func:`paged_decode`
    when the prefix blocks are the ones every row's table starts with."""
    if _gpu(q):
        return _native().paged_decode_cascade(q, k_cache, v_cache, block_tables, context_lens, Hq,
                                              max_context, scale, prefix_table, prefix_len, nchunk, order)
    return ref.paged_decode_cascade(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context,
                                    scale, prefix_table, prefix_len, nchunk)


def paged_decode_cascade_grouped(q, k_cache, v_cache, block_tables, context_lens, Hq, scale,
                                 prefix_table, prefix_len, nchunk: int, groups, defer: bool = False,
                                 tick=None, inline_prefix: bool = False):
    """Cascade decode with the suffix attention of rows that share prefix-cache KV blocks
    done together (csrc/kernels/attn_decode.hip paged_decode_group_kernel): ``groups``
    int32 [ngroups * 4] packs every row into one group of <= 4 (-1 = empty slot), and a
    block shared by k rows of a group is read once instead of k times.  Same result as
    :func:`paged_decode_cascade` for any packing.  ``groups`` may also be a split plan
    int32 [2, cap, 8] from :func:`split_decode_groups` (long groups over several
    workgroups, partials merged by log-sum-exp); ``defer``: that plan was built with
    ``split_decode_groups(defer=True)`` (the prefix kernel then runs on a side stream).
    ``tick``: zeroed int32 ticket words (>= cap x Hkv, :func:`decode_ticket`) -- a split
    plan's groups are then merged by their last work item instead of a merge launch.
    ``inline_prefix``: the split plan's items start at block 0 (built with skip 0), so the
    groups attend the shared prefix themselves -- no prefix kernel."""
    if _gpu(q):
        if groups.dim() == 3:
            return _native().paged_decode_cascade_split(q, k_cache, v_cache, block_tables, context_lens, Hq,
                                                        scale, prefix_table, prefix_len, nchunk, groups,
                                                        defer and groups.shape[0] == 2, tick,
                                                        bool(inline_prefix) and groups.shape[0] == 2)
        return _native().paged_decode_cascade_grouped(q, k_cache, v_cache, block_tables, context_lens, Hq,
                                                      scale, prefix_table, prefix_len, nchunk, groups)
    max_context = block_tables.shape[1] * k_cache.shape[2]
    return ref.paged_decode_cascade(q, k_cache, v_cache, block_tables, context_lens, Hq, max_context,
                                    scale, prefix_table, prefix_len, nchunk)


def paged_decode_grouped_fused(P, positions, cos_sin, slot_mapping, k_cache, v_cache, block_tables, context_lens,
                               Hq, scale, prefix_table, prefix_len, nchunk: int, plan, tick=None):
    """Grouped decode attention straight from the QKV projection's split-K slabs (split plan
    built from block 0, no prefix kernel): each workgroup rotates the query rows it needs and
    the item holding a row's new token writes its rotated K / V to the paged cache first --
    the same result as :func:`rope_cache_splitk` + :func:`paged_decode_cascade_grouped`
    (``inline_prefix``), one launch and the bf16 QKV round trip fewer."""
    if _gpu(P):
        return _native().paged_decode_grouped_fused(P, positions, cos_sin, slot_mapping, k_cache, v_cache,
                                                    block_tables, context_lens, Hq, scale, prefix_table,
                                                    prefix_len, nchunk, plan, tick)
    Hkv, D = k_cache.shape[1], k_cache.shape[3]
    qkv = rope_cache_splitk(P, positions, cos_sin, slot_mapping, k_cache, v_cache, Hq, Hkv, D)
    return paged_decode_cascade_grouped(qkv, k_cache, v_cache, block_tables, context_lens, Hq, scale, prefix_table,
                                        prefix_len, nchunk, plan, False, tick, True)


GROUP_MAX_BLOCKS = 64   # block positions one grouped-decode work item covers (attn_decode.hip kGroupMaxPos)


def grouped_decode_ok(k_cache, block_tables, Hq: int, max_blocks: int | None = None) -> bool:
    """Shapes the grouped cascade kernel supports: cascade shapes and rows of <= 64 blocks --
    ``max_blocks``, the most any row of the batch reaches by the end of its decode, or else
    the block table's width (its capacity)."""
    nb = block_tables.shape[1] if max_blocks is None else max_blocks
    if _gpu(k_cache) and kv_is_fp8(k_cache):
        # FP8 cache: only the wave-parallel split kernel with the plan built from block 0
        # (``inline_prefix``) reads it -- the caller must hold a [2, cap, 8] split plan
        return (k_cache.shape[2] == 64 and k_cache.shape[3] == 128 and Hq == 4 * k_cache.shape[1]
                and block_tables.shape[1] <= 256 and nb <= GROUP_MAX_BLOCKS)
    return cascade_ok(k_cache, block_tables, Hq) and nb <= GROUP_MAX_BLOCKS


def pack_decode_groups(tables: list[list[int]], lens: list[int], skip: int, block_size: int,
                       cap: int) -> list[list[int]]:
    """Pack the rows of a decode batch into groups of <= 4 for the grouped decode kernel:
    rows are sorted by their block ids beyond the ``skip`` cascade-prefix blocks (rows whose
    prompts share prefix-cache blocks become neighbours), clusters of rows sharing their
    first such block stay together where they fit, and the groups are ordered by distinct
    blocks, largest first (LPT).  Falls back to plain consecutive quads when the packing
    would exceed ``cap`` groups."""
    n = len(tables)
    if n == 0:
        return []
    # sort key: block ids relabelled by first occurrence (row-major), so the packing -- and
    # with it each row's split points and partial-merge order -- depends only on which rows
    # share blocks, never on the physical ids the allocator handed out (a pipelined run
    # frees batch i-1 and reserves batch i+1 on two threads in a timing-dependent order)
    label: dict[int, int] = {}
    for t in tables:
        for b in t[skip:]:
            label.setdefault(b, len(label))
    keyed = [[label[b] for b in t[skip:]] for t in tables]
    idx = sorted(range(n), key=lambda i: keyed[i])

    def first(i):
        return tables[i][skip] if len(tables[i]) > skip else -1 - i

    clusters, cur = [], [idx[0]]
    for a, b in zip(idx, idx[1:]):
        if first(a) == first(b) and first(a) >= 0:
            cur.append(b)
        else:
            clusters.append(cur)
            cur = [b]
    clusters.append(cur)
    quads, cur = [], []
    for cl in clusters:
        while len(cl) > 4:
            quads.append(cl[:4])
            cl = cl[4:]
        if len(cur) + len(cl) > 4:
            quads.append(cur)
            cur = []
        cur = cur + cl
    if cur:
        quads.append(cur)
    if len(quads) > cap:
        quads = [idx[i:i + 4] for i in range(0, n, 4)]

    def work(qd):
        blocks = set()
        for r in qd:
            nb = (lens[r] + block_size - 1) // block_size
            blocks.update(tables[r][skip:nb])
        return len(blocks)

    quads.sort(key=work, reverse=True)
    return quads


def kv_copy_rows(pools: list, copies: list, ptrs: torch.Tensor | None = None) -> None:
    """K/V rows [0, m) of block src -> the same rows of block dst in every paged pool
    (``pools``: [(k, v)] per layer, [num_blocks, Hkv, BS, D]; ``copies``: [(src, dst, m)]).
    GPU: one launch of csrc/kernels/rope_cache.hip kv_copy_rows over all pools (``ptrs``:
    int64 device addresses of the pools in (k_0, v_0, k_1, ...) order, built by the
    caller once); CPU: tensor indexing."""
    if not copies:
        return
    k0 = pools[0][0]
    if _gpu(k0):
        if ptrs is None:
            ptrs = torch.tensor([t.data_ptr() for kv in pools for t in kv], dtype=torch.int64, device=k0.device)
        tab = torch.tensor(copies, dtype=torch.int32).pin_memory().to(k0.device, non_blocking=True)
        copy = _native().kv_copy_rows8 if kv_is_fp8(k0) else _native().kv_copy_rows   # 1-byte / bf16 rows
        copy(ptrs, tab, k0.shape[0], k0.shape[1], k0.shape[2], k0.shape[3])
        return
    src = torch.tensor([s for s, _, m in copies for _ in range(m)], dtype=torch.long, device=k0.device)
    dst = torch.tensor([d for _, d, m in copies for _ in range(m)], dtype=torch.long, device=k0.device)
    rows = torch.tensor([i for _, _, m in copies for i in range(m)], dtype=torch.long, device=k0.device)
    for kc, vc in pools:
        if kv_is_fp8(kc):   # an FP8 pool is copied through its code bytes
            kc, vc = kc.view(torch.uint8), vc.view(torch.uint8)
        kc[dst, :, rows] = kc[src, :, rows]
        vc[dst, :, rows] = vc[src, :, rows]


def group_tiles_by_position(tables: list[list[int]], lens: list[int], rows: list[int], skip: int,
                            block_size: int) -> list[tuple[int, int]]:
    """(block position, 32-token K/V tiles) the grouped decode kernel streams for ``rows``
    at each position beyond the ``skip`` cascade-prefix blocks: one or two tiles (by the
    longest length among the rows reading it) per DISTINCT block id at that position."""
    half = block_size // 2
    rl = [(tables[r], lens[r]) for r in rows]
    nb = max((L + block_size - 1) // block_size for _, L in rl)
    out = []
    for pos in range(skip, nb):
        lo = pos * block_size
        live: dict[int, int] = {}
        for t, L in rl:
            if lo < L and pos < len(t):
                b = t[pos]
                if live.get(b, 0) < L:
                    live[b] = L
        if live:
            thr = lo + half
            out.append((pos, len(live) + sum(1 for L in live.values() if L > thr)))
    return out


def remap_plan_rows(plan: torch.Tensor, plan_ids: list, ids: list) -> torch.Tensor | None:
    """A split plan (:func:`split_decode_groups`, [2 or 3, cap, 8]) built for rows with
    request ids ``plan_ids``, re-targeted at rows ``ids`` after requests RETIRED and the
    survivors were compacted: each row id in columns 0..3 of the items and merges becomes
    the survivor's new index, or -1 if it retired.  None if ``ids`` holds a request the plan
    does not know (an admission: re-plan).  Positions and split points stay valid -- they
    depend only on each survivor's blocks and END length -- and every item of a group
    carries the group's rows, so a fully retired group's items all exit before drawing a
    merge ticket."""
    pos = {rid: i for i, rid in enumerate(plan_ids)}
    if not all(rid in pos for rid in ids):
        return None
    n = len(plan_ids)
    m = torch.full((n + 1,), -1, dtype=torch.int32)
    if ids:
        m[torch.tensor([pos[rid] for rid in ids], dtype=torch.long)] = torch.arange(len(ids), dtype=torch.int32)
    out = plan.clone()
    cols = plan[:2, :, :4].long()
    out[:2, :, :4] = torch.where(cols >= 0, m[cols.clamp(min=0, max=n)], torch.full_like(plan[:2, :, :4], -1))
    return out


def persist_bins(cap: int, Hkv: int) -> int:
    """Workgroups per KV head of the persistent grouped decode (attn_decode.hip
    group_persist_bins): ~3 per CU chip-wide, at least one per quad of ``cap`` rows."""
    nb = max(768 // max(1, Hkv), (cap + 3) // 4)
    return min(nb, cap)


BIN_ITEMS, BIN_MAX_TILES = 8, 512    # attn_decode.hip kBinItems / kBinMaxTiles


def split_decode_groups(quads: list[list[int]], tables: list[list[int]], lens: list[int], skip: int,
                        block_size: int, cap: int, tiles_per_item: int = 12, bins: int = 0,
                        defer: bool = False, per_quad: list | None = None) -> torch.Tensor:
    """Split plan for the grouped cascade decode (``paged_decode_cascade_grouped`` with a
    [2, cap, 8] int32 ``groups``): every group of :func:`pack_decode_groups` is cut at block
    positions into work items of about ``tiles_per_item`` K/V tiles (``lens``: the lengths
    at the END of decode, so an item's range stays valid for every step), one workgroup per
    item and KV head.  A group that needs one item finishes in its workgroup; the items of
    a longer group write partials that a merge kernel combines.  Items are ordered largest
    first (LPT).  plan[0]: items (4 rows, first position, end position, slot or -1, 0);
    plan[1]: merges (4 rows, first slot, slots, 0, 0) -- at most (cap + 1) // 2 of them
    (the merge kernel's grid).

    ``bins`` > 0: the PERSISTENT plan [3, cap, 8] instead -- every item writes a partial
    (slot = its index), every group has a merge row, and plan[2] packs the items into
    ``bins`` (:func:`persist_bins`) workgroups of <= 8 items and <= 512 tiles each, greedy
    longest-first onto the least-loaded bin, so each workgroup streams ~total / bins tiles
    through one ring.

    ``defer``: every item writes a partial and every group has a merge row (at most ``cap``),
    as in the persistent plan, so no item reads the cascade-prefix partials and the prefix
    kernel runs on a side stream beside the group kernel (attn_decode.hip, DOCQA_GROUP_DEFER).

    ``per_quad``: :func:`group_tiles_by_position` of each quad, precomputed (a caller that
    tries several budgets for one batch computes them once -- they do not depend on it)."""
    budget = max(1, tiles_per_item)
    all_partial = bool(bins) or defer
    if per_quad is None:
        per_quad = [group_tiles_by_position(tables, lens, list(qd), skip, block_size) for qd in quads]
    while True:
        items, merges, nslot = [], [], 0
        for qd, per in zip(quads, per_quad):
            rows4 = (list(qd) + [-1] * 4)[:4]
            cuts, acc, start = [], 0, skip
            for pos, t in per:
                if acc and acc + t > budget:
                    cuts.append((start, pos, acc))
                    start, acc = pos, 0
                acc += t
            end = max((lens[r] + block_size - 1) // block_size for r in qd)
            cuts.append((start, max(end, start + 1), acc))
            # an item of a merged group carries its merge row (column 7) for the
            # last-arriver merge inside the group kernel
            if all_partial:
                merges.append(rows4 + [nslot, len(cuts), 0, 0])
                for lo, hi, t in cuts:
                    items.append((t, rows4 + [lo, hi, nslot, len(merges) - 1]))
                    nslot += 1
            elif len(cuts) == 1:
                items.append((cuts[0][2], rows4 + [skip, 1 << 20, -1, 0]))
            else:
                merges.append(rows4 + [nslot, len(cuts), 0, 0])
                for lo, hi, t in cuts:
                    items.append((t, rows4 + [lo, hi, nslot, len(merges) - 1]))
                    nslot += 1
        fits = len(items) <= cap and len(merges) <= (cap if all_partial else (cap + 1) // 2)
        if fits and bins:
            nb = min(bins, cap)
            fits = len(items) <= nb * BIN_ITEMS and all(t <= BIN_MAX_TILES for t, _ in items)
        if fits:
            break
        if budget > 1 << 20:
            raise ValueError(f"split_decode_groups: {len(quads)} groups exceed the plan capacity {cap}")
        budget *= 2
    if not bins:
        items.sort(key=lambda it: -it[0])
        plan = torch.full((2, cap, 8), -1, dtype=torch.int32)
        plan[:, :, 4:] = 0
        if items:
            plan[0, :len(items)] = torch.tensor([it[1] for it in items], dtype=torch.int32)
        if merges:
            plan[1, :len(merges)] = torch.tensor(merges, dtype=torch.int32)
        return plan
    nb = min(bins, cap)
    load, members = [0] * nb, [[] for _ in range(nb)]
    for i in sorted(range(len(items)), key=lambda i: -items[i][0]):
        t = items[i][0]
        best = min((b for b in range(nb) if len(members[b]) < BIN_ITEMS and load[b] + t <= BIN_MAX_TILES),
                   key=lambda b: load[b], default=None)
        if best is None:    # every bin full: the plan cannot hold this batch
            raise ValueError("split_decode_groups: items exceed the persistent bins")
        members[best].append(i)
        load[best] += t
    plan = torch.full((3, cap, 8), -1, dtype=torch.int32)
    plan[:2, :, 4:] = 0
    plan[0, len(items):, 6] = -1           # unused item rows: no slot
    if items:
        plan[0, :len(items)] = torch.tensor([it[1] for it in items], dtype=torch.int32)
    if merges:
        plan[1, :len(merges)] = torch.tensor(merges, dtype=torch.int32)
    for b, mem in enumerate(members):
        # a bin streams its items in index order: keep them position-ordered per group
        for j, i in enumerate(sorted(mem)):
            plan[2, b, j] = i
    return plan


def flash_prefill(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, causal=True):
    if _gpu(qkv):
        return _native().flash_prefill(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, causal)
    return ref.flash_prefill(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, causal)


def flash_prefill_paged(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, k_cache, v_cache,
                        block_tables, ctx_start):
    if _gpu(qkv):
        return _native().flash_prefill_paged(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, k_cache,
                                             v_cache, block_tables, ctx_start)
    return ref.flash_prefill_paged(qkv, cu_seqlens, max_len, Hq, Hkv, D, scale, k_cache, v_cache,
                                   block_tables, ctx_start)


# ----------------------------------------------------------------------------- search
def knn(xb, xb_norms, xq, k: int, inner_product: bool = False, id_offset: int = 0):
    if _gpu(xb):
        return _native().knn(xb, xb_norms, xq.float().contiguous(), k, inner_product, id_offset)
    return ref.knn(xb, xb_norms, xq, k, inner_product, id_offset)


def knn_scoped(xb, xb_norms, tags, days, xq, scope, k: int, inner_product: bool = False, id_offset: int = 0):
    """:func:`knn` among the rows whose (tag, day) satisfy the query's scope row: tags / days
    int32 [N], scope int32 [nq, 4] = (tag, alt_tag, day_lo, day_hi), see
    ``reference.knn_scoped`` for the predicate.  GPU: the SCOPED instantiations of the fused
    kernel (csrc/kernels/knn.hip), which skip tiles no query's scope touches.  Shapes outside
    the kernel's envelope (k > 64, d not a multiple of 8 / 16 for fp32 / bf16 storage, query
    staging + 512 B of scope rows over 160 KiB of LDS) and ``DOCQA_KNN_SCOPED=0`` (kill
    switch) take the fp32 reference on the same device instead of failing."""
    if _gpu(xb) and os.environ.get("DOCQA_KNN_SCOPED", "1") != "0":
        bf = xb.dtype == torch.bfloat16
        d = int(xb.shape[1])
        kp = next((p for p in (4, 8, 16, 32, 64) if k <= p), 0)
        lds = max(32 * d * (2 if bf else 4), 32 * 8 * kp * 8) + 512
        if (kp and k >= 1 and (bf or xb.dtype == torch.float32) and d % (16 if bf else 8) == 0
                and lds <= 160 * 1024):
            return _native().knn_scoped(xb, xb_norms, tags.int().contiguous(), days.int().contiguous(),
                                        xq.float().contiguous(), scope.int().contiguous(), k,
                                        inner_product, id_offset)
    return ref.knn_scoped(xb, xb_norms, tags, days, xq, scope, k, inner_product, id_offset)


def bm25_topk(row_ptr, terms, tfs, dl, qterms, qweights, k: int, avgdl: float, k1: float = 1.2, b: float = 0.75,
              tags=None, days=None, scope=None, id_offset: int = 0):
    """BM25 top-k over CSR term columns (index/lexical.py): -> (S fp32 [nq, k] descending, ties
    towards the lower row, I int64 [nq, k]; -FLT_MAX / -1 past the matching rows); see
    ``reference.bm25_topk`` for the arithmetic.  ``tags``, ``days`` and ``scope`` together
    scope every query as in :func:`knn_scoped`.  GPU: the fused scan of
    csrc/kernels/lexical.hip.  Outside its envelope (k > 64, query rows not 32 slots wide,
    2^31 - 512 rows or 2^31 entries, a ``tfs`` that is not uint8, ``qweights`` not shaped like
    ``qterms``) and with ``DOCQA_BM25=0`` (kill switch) the fp32 reference runs on the same
    device instead of failing."""
    scoped = tags is not None and days is not None and scope is not None
    if not scoped:
        tags = days = scope = None
    if _gpu(row_ptr) and os.environ.get("DOCQA_BM25", "1") != "0":
        if (1 <= k <= 64 and qterms.dim() == 2 and qterms.shape[1] == 32 and qweights.shape == qterms.shape
                and tfs.dtype == torch.uint8 and tfs.numel() == terms.numel() and avgdl > 0
                and row_ptr.numel() - 1 < (1 << 31) - 512 and terms.numel() < (1 << 31)):
            i32 = lambda t: None if t is None else t.int().contiguous()  # noqa: E731
            return _native().bm25_topk(row_ptr.long().contiguous(), terms.int().contiguous(), tfs.contiguous(),
                                       dl.int().contiguous(), qterms.int().contiguous(),
                                       qweights.float().contiguous(), k, float(avgdl), float(k1), float(b),
                                       i32(tags), i32(days), i32(scope), id_offset)
    return ref.bm25_topk(row_ptr, terms, tfs, dl, qterms, qweights, k, avgdl, k1, b, tags, days, scope, id_offset)


def rank_fuse(I_dense, I_lex, mode, k: int, c: int = 60):
    """Per query, by ``mode`` int32 [nq]: 0 the first k ids of ``I_dense``, 1 of ``I_lex``, 2
    their reciprocal rank fusion (score = sum of 1 / (c + rank), compared exactly, ties towards
    the lower id); lists of up to 64 ranked ids, negative entries ignored.  -> (F fp32 [nq, k],
    I int64 [nq, k]), 0 / -1 in missing slots.  GPU: one wave per query (lexical.hip), no
    host sync, so a mixed batch is a dense, a lexical and a fuse launch back to back."""
    if _gpu(I_dense):
        if I_dense.shape[1] > 64 or I_lex.shape[1] > 64 or not 0 <= c <= 100000:
            raise ValueError("rank_fuse: lists of at most 64 ids and c in [0, 100000]")
        return _native().rank_fuse(I_dense.long().contiguous(), I_lex.long().contiguous(),
                                   mode.int().contiguous(), k, c)
    return ref.rank_fuse(I_dense, I_lex, mode, k, c)


def mmr_select(xb, xb_norms, xq, cand, ncand, lam, k: int):
    """Maximal marginal relevance re-selection of ranked candidate lists (LangChain's
    ``search_type="mmr"``): per query ``k`` picks out of ``cand`` int64 [nq, F] (best first; the
    first ``ncand[q]`` entries with an id in ``[0, N)``), greedily by ``lam * cos(q, c) -
    (1 - lam) * max cos(c, picked)``, cosines in fp32 whatever the index metric; ``lam`` fp32
    [nq], negative = the row's first k entries pass through.  -> (S fp32, I int64, P int32
    [nq, k]): the winning value, the id and the position in ``cand`` of every pick, 0 / -1 /
    -1 in missing slots; see ``reference.mmr_select``.  GPU: one launch, one workgroup per
    query (csrc/kernels/mmr.hip), no host sync.  Outside its envelope (``1 <= k <= F <= 64``,
    ``d`` a multiple of 8 / 16 for fp32 / bf16 rows, no other row dtype) and with
    ``DOCQA_MMR=0`` (kill switch) the fp32 reference runs on the same device instead of
    failing."""
    if _gpu(xq) and os.environ.get("DOCQA_MMR", "1") != "0":
        bf = xb.dtype == torch.bfloat16
        d, F = int(xb.shape[1]), int(cand.shape[1])
        if (1 <= k <= F <= 64 and (bf or xb.dtype == torch.float32) and d > 0 and d % (16 if bf else 8) == 0
                and xq.shape[0] > 0):
            return _native().mmr_select(xb.contiguous(), xb_norms.float().contiguous(), xq.float().contiguous(),
                                        cand.long().contiguous(), ncand.int().contiguous(),
                                        lam.float().contiguous(), k)
    return ref.mmr_select(xb, xb_norms, xq, cand, ncand, lam, k)


# ----------------------------------------------------------------------------- row compaction
# Deleting rows from the store (csrc/kernels/compact.hip): a masked scan gives every surviving
# row its new position, then each per-row column is gathered out of place.  Exact and
# deterministic; no host sync.  The scan is reduce-then-scan over tiles of SCAN_TILE values with
# SCAN_LEVELS levels at most, so the kernel serves up to SCAN_TILE ** SCAN_LEVELS rows (the
# values csrc/kernels/compact.hip is built with: kScanTile, docqa_compact_scan_levels).
SCAN_TILE = 1024
SCAN_LEVELS = 3
GATHER_MAX_ROW_BYTES = 1 << 20


def _compact_native(t: torch.Tensor) -> bool:
    return _gpu(t) and os.environ.get("DOCQA_COMPACT", "1") != "0"


def masked_scan(keep, w=None):
    """``keep`` uint8 [n] (non-zero = the row survives), ``w`` int64 [n] or None -> ``pos`` int64
    [n+1]: the exclusive prefix sum of ``keep[r] ? w[r] : 0`` (``w`` = 1 without weights), so
    ``pos[r]`` is row r's new position and ``pos[n]`` the surviving total.  GPU: 1 / 3 / 5
    launches by size (per-tile sums, scan of the sums, per-tile finalisation; no workgroup waits
    on another).  CPU tensors, ``DOCQA_COMPACT=0`` (kill switch) and anything outside the
    envelope (uint8 mask, int64 weights, n <= SCAN_TILE ** SCAN_LEVELS) take
    ``reference.masked_scan`` on the same device."""
    n = keep.numel()
    if (_compact_native(keep) and keep.dtype == torch.uint8 and keep.dim() == 1 and n <= SCAN_TILE ** SCAN_LEVELS
            and (w is None or (w.dtype == torch.int64 and w.shape == keep.shape and w.device == keep.device))):
        return _native().masked_scan(keep.contiguous(), None if w is None else w.contiguous())
    return ref.masked_scan(keep, w)


def gather_rows(src, keep, pos, n_out: int | None = None, out=None):
    """Compact the kept rows of ``src`` [n, ...] (any dtype; rows of W bytes): ``out[pos[r]] =
    src[r]``.  ``out`` (given, or ``torch.empty`` of ``n_out`` rows) is a different buffer from
    ``src`` with at least ``pos[n]`` rows; rows past that are left as they are.  GPU: one
    streaming launch on 16-byte lanes when W and both bases allow, else 4-byte lanes, else bytes.
    Returns ``out``.  The reference runs for CPU tensors, ``DOCQA_COMPACT=0``, rows wider than
    ``GATHER_MAX_ROW_BYTES`` and non-contiguous operands."""
    if out is None:
        out = torch.empty((int(n_out),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
    n = src.shape[0]
    W = (src.numel() // n if n else 1) * src.element_size()
    if (_compact_native(src) and keep.dtype == torch.uint8 and pos.dtype == torch.int64 and src.is_contiguous()
            and out.is_contiguous() and keep.is_contiguous() and pos.is_contiguous() and 1 <= W <= GATHER_MAX_ROW_BYTES
            and out.dtype == src.dtype and out.shape[1:] == src.shape[1:] and pos.numel() == n + 1):
        _native().gather_rows(src, keep, pos, out)
        return out
    return ref.gather_rows(src, keep, pos, out)


def csr_gather(row_ptr, keep, pos, epos, terms, tfs, n_out: int, e_out: int):
    """The kept rows of a CSR: ``row_ptr`` int64 [n+1], ``pos`` the row scan, ``epos`` the scan
    weighted by the row lengths, ``terms`` int32 / ``tfs`` uint8 [>= row_ptr[n]] -> (``row_ptr'``
    int64 [n_out+1], ``terms'`` [e_out], ``tfs'`` [e_out]), one launch.  ``n_out`` / ``e_out``
    are ``pos[n]`` / ``epos[n]``, which the caller knows on the host (no sync here)."""
    if (_compact_native(row_ptr) and keep.dtype == torch.uint8 and terms.dtype == torch.int32
            and tfs.dtype == torch.uint8 and terms.numel() == tfs.numel() and 0 <= n_out <= keep.numel()
            and 0 <= e_out <= terms.numel()):
        return tuple(_native().csr_gather(row_ptr.contiguous(), keep.contiguous(), pos.contiguous(),
                                          epos.contiguous(), terms.contiguous(), tfs.contiguous(), n_out, e_out))
    return ref.csr_gather(row_ptr, keep, pos, epos, terms, tfs, n_out, e_out)


def remap_ids(ids, pos):
    """``ids'[j] = pos[ids[j]]`` over a list of row ids that survived (the IVF lists name rows of
    the flat store); an id outside ``[0, n)`` becomes -1."""
    if _compact_native(ids) and ids.dtype == torch.int64 and pos.dtype == torch.int64 and pos.numel() >= 1:
        return _native().remap_ids(ids.contiguous(), pos.contiguous())
    return ref.remap_ids(ids, pos)


def fp32_matmul_nt(x, w):
    """Exact fp32 ``x @ w.T`` on the coarse quantizer's MFMA tiles (coarse.hip) -- the IVF-PQ
    query pre-rotation on the GPU without a library GEMM; torch on the CPU."""
    if _gpu(x) and x.shape[1] % 8 == 0 and x.shape[1] <= 1280:
        return _native().fp32_gemm_nt(x.float().contiguous(), w.float().contiguous())
    return x.float() @ w.float().t()


def coarse_probes(xq, centroids, cnorm, nprobe: int):
    """IVF coarse quantizer: int64 [nq, nprobe] nearest centroids by squared L2, ascending,
    ties to the lower centroid id.  GPU: csrc/kernels/coarse.hip (MFMA fp32 distances +
    radix select, nprobe <= 512); nprobe <= 64 may also use :func:`knn`.  Shapes outside
    the kernel's envelope (nprobe > 512, d > 1280 or d % 8 != 0 -- recall sweeps, wide
    embeddings) take the fp32 reference on the same device instead of failing."""
    d = int(centroids.shape[1])
    nprobe = int(min(int(nprobe), int(centroids.shape[0])))
    if _gpu(xq) and nprobe <= 512 and d % 8 == 0 and d <= 1280:
        return _native().coarse_probes(xq.float().contiguous(), centroids, cnorm, nprobe)
    return ref.coarse_probes(xq, centroids, cnorm, nprobe)


# ----------------------------------------------------------------------------- pooling
def pool_l2(h, cu_seqlens, mean: bool = True, normalize: bool = True):
    if _gpu(h):
        return _native().pool_l2(h.contiguous(), cu_seqlens, mean, normalize)
    return ref.pool_l2(h, cu_seqlens, mean, normalize)


# eager-load when a GPU is present so an import on the box fails loudly if unbuilt
if torch.cuda.is_available() and not _FORCE_REF:
    load_native()
