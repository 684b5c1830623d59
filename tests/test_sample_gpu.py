"""``sample_kernel`` (csrc/kernels/embed_sample.hip) against the fp64 oracle of
tests/sample_oracle.py: top-k, top-p and temperature at every vocabulary shape that changes
the kernel's slicing, per-row parameters in one launch, strided rows, penalised and peaked rows,
ties at the k-th value, the ends of u, and ``top_k == 1`` as an argmax under ties.

Every input's preconditions (threshold gaps against the bisection's resolution, top-p margins
against the mass error) are asserted, and every draw is checked: nothing is excluded.  Each
check prints the largest distance of a draw from its exact CDF interval (``overshoot``), the
figure ``DELTA`` leaves room for.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests.sample_oracle import (CASES, DELTA, VS, build_case, check, make_row, peaked_row, penalised_row,
                                 scaled, tied_kth_row, uniforms)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops.native_loaded()
    return ops


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _launch(logits, it, k, p, u):
    """One launch of the native sampler: ``logits`` a CUDA fp32 [rows, V] tensor (any row
    stride), the per-row parameters numpy arrays -> tokens as numpy."""
    out = torch.ops.docqa.sample(logits, _dev(it, torch.float32), _dev(k, torch.int32), _dev(p, torch.float32),
                                 _dev(u, torch.float32))
    return out.cpu().numpy()


def _draw(row, params, u):
    """One row under one parameter tuple at every u (the row replicated on the device)."""
    n = len(u)
    logits = _dev(row, torch.float32).expand(n, -1).contiguous()
    return _launch(logits, np.full(n, params[0]), np.full(n, params[1]), np.full(n, params[2]), u)


def _checked(tok, u, keep, cdf, what):
    over = check(tok, u, keep, cdf)
    print(f"overshoot {over:.3e} of delta {DELTA:g}: {what}")
    return over


@pytest.mark.parametrize("ci", range(len(CASES)))
@pytest.mark.parametrize("V", VS)
def test_case_matrix(V, ci):
    row = make_row(V, seed=100 * ci + V)
    params, u, keep, cdf, _ = build_case(row, CASES[ci], seed=ci)
    _checked(_draw(row, params, u), u, keep, cdf, f"V={V} case={params}")


@pytest.mark.parametrize("V,case,seed", [(1000, (1.0, 0, 1.0), 11), (32000, (1.25, 40, "p*"), 14)])
def test_u_sweep(V, case, seed):
    """One row at u = (i + 0.5) / 4096: every kept token wider than two steps of u plus the slack
    is returned, and nothing outside the kept set is."""
    row = make_row(V, seed=seed)
    params, _, keep, cdf, _ = build_case(row, case)
    u = ((np.arange(4096) + 0.5) / 4096).astype(np.float32)
    tok = _draw(row, params, u)
    _checked(tok, u, keep, cdf, f"sweep V={V} case={params}")
    mass = np.diff(cdf, prepend=0.0)
    must = set(np.nonzero(keep & (mass > 2 / 4096 + 2 * DELTA))[0].tolist())
    assert len(must) >= 3
    assert must <= set(tok.tolist()) <= set(np.nonzero(keep)[0].tolist())


def test_mixed_launch():
    """300 rows (more workgroups than CUs), each its own logits, parameter tuple and u; greedy
    ``top_k == 1`` rows sit between the sampled ones."""
    V, rows = 1000, 300
    tuples = list(CASES) + [(1.0, 1, 1.0), (1.25, 1, 0.5)]
    logits = np.stack([make_row(V, seed=5000 + r) for r in range(rows)])
    u = uniforms(rows, seed=77)
    par, orc = [], []
    for r in range(rows):
        case = tuples[r % len(tuples)]
        if case[1] == 1:
            par.append(case)
            orc.append(None)
        else:
            params, _, keep, cdf, _ = build_case(logits[r], case)
            par.append(params)
            orc.append((keep, cdf))
    par = np.array(par, dtype=np.float64)
    tok = _launch(_dev(logits, torch.float32), par[:, 0], par[:, 1], par[:, 2], u)
    worst = 0.0
    for r in range(rows):
        if orc[r] is None:
            assert tok[r] == int(np.argmax(scaled(logits[r], par[r, 0]))), f"row {r}: top_k == 1 is an argmax"
        else:
            worst = max(worst, check(tok[r:r + 1], u[r:r + 1], *orc[r]))
    print(f"overshoot {worst:.3e} of delta {DELTA:g}: mixed launch")


@pytest.mark.parametrize("V", [257, 1000])
def test_strided_rows(V):
    """Rows of a wider buffer (ld = V + 8) whose padding would win every draw if it were read."""
    rows = 2 * len(CASES)
    logits = np.stack([make_row(V, seed=6000 + r) for r in range(rows)])
    built = [build_case(logits[r], CASES[r % len(CASES)]) for r in range(rows)]
    par = np.array([b[0] for b in built], dtype=np.float64)
    u = uniforms(rows, seed=78)
    buf = torch.full((rows, V + 8), 1e9, dtype=torch.float32, device="cuda")
    buf[:, :V] = _dev(logits, torch.float32)
    view = buf[:, :V]
    assert view.stride(0) == V + 8 and not view.is_contiguous()
    tok = _launch(view, par[:, 0], par[:, 1], par[:, 2], u)
    assert (tok < V).all()
    assert np.array_equal(tok, _launch(view.contiguous(), par[:, 0], par[:, 1], par[:, 2], u))
    for r in range(rows):
        check(tok[r:r + 1], u[r:r + 1], built[r][2], built[r][3])


@pytest.mark.parametrize("case", [(1.25, 40, 1.0), (1.25, 40, "p*")])
@pytest.mark.parametrize("V", [1000, 128256])
def test_penalised_rows(V, case):
    """64 entries at about -1e4, as presence_penalty = 1e4 leaves them: the bisections start from a
    range of 1e4, so their resolution is ~6e-4 (seed 2 meets the asserted preconditions)."""
    row = penalised_row(V, seed=2)
    params, u, keep, cdf, info = build_case(row, case)
    assert info["res"] > 5e-4 and not keep[row < -5e3].any()
    _checked(_draw(row, params, u), u, keep, cdf, f"penalised V={V} case={params}")


@pytest.mark.parametrize("V", [1000, 32000])
def test_peaked_row(V):
    """One logit 50 above the rest is the answer for every u under every parameter tuple."""
    row, at = peaked_row(V, seed=V)
    u64 = ((np.arange(64) + 0.5) / 64).astype(np.float32)
    built = [build_case(row, c) for c in CASES]
    par = np.repeat(np.array([b[0] for b in built], dtype=np.float64), 64, axis=0)
    u = np.tile(u64, len(CASES))
    logits = _dev(row, torch.float32).expand(len(u), -1).contiguous()
    tok = _launch(logits, par[:, 0], par[:, 1], par[:, 2], u)
    for i, b in enumerate(built):
        check(tok[64 * i:64 * i + 64], u64, b[2], b[3])
    assert (tok == at).all()


def test_ties_at_the_kth_value():
    row = tied_kth_row(V=1000, rank=40, copies=3)
    params, u, keep, cdf, info = build_case(row, (1.25, 40, 1.0))
    assert keep.sum() == 42
    tok = _draw(row, params, u)
    _checked(tok, u, keep, cdf, "ties at the 40th value")


@pytest.mark.parametrize("V", [257, 32000])
def test_u_edges(V):
    """u = 0 is the first kept token whose fp32 probability is non-zero; u = 1 - 2^-24 is a kept
    token.  exp(d) for d = x - max is surely non-zero in fp32 above d = -86 and surely zero below
    -104.5 (2^-150); a kept token in between may or may not count."""
    rows = [make_row(V, seed=7000 + i) for i in range(len(CASES))]
    cases = list(CASES)
    pen = make_row(V, seed=7100)
    pen[:5] -= np.float32(1e4)                      # the first ids: probability exactly 0
    rows.append(pen)
    cases.append((1.0, 0, 1.0))
    for row, case in zip(rows, cases):
        params, _, keep, cdf, info = build_case(row, case)
        u = np.array([0.0, 1.0 - 2.0 ** -24], dtype=np.float32)
        assert u[1] < 1.0
        t0, t1 = _draw(row, params, u)
        d = info["x"] - info["x"].max()
        assert keep[t0] and keep[t1], (params, t0, t1)
        assert d[t0] >= -104.5, f"{params}: u = 0 returned token {t0} of probability 0"
        before = keep[:t0] & (d[:t0] >= -86.0)
        assert not before.any(), f"{params}: u = 0 returned {t0}, but kept token {np.nonzero(before)[0][0]} precedes it"
    assert t0 == 5                                   # the penalised row: the first id that is not at -1e4


@pytest.mark.parametrize("V,copies", [(1000, 2), (1000, 3), (4096, 200), (128256, 3), (128256, 200)])
def test_top_k_1_is_argmax_under_ties(native, V, copies):
    """bf16-rounded logits with several copies of the maximum, on greedy rows among sampled ones:
    ``top_k == 1`` returns the lowest index of the maximum, as ``argmax`` does, whatever u, top_p
    and the temperature are.  (At V = 128256 the copies lie in different threads' slices.)"""
    row = torch.from_numpy(make_row(V, seed=copies)).bfloat16().float().numpy()
    rng = np.random.default_rng(V + copies)
    at = np.sort(rng.choice(np.arange(V // 8, V), size=copies, replace=False))
    if V == 128256:                                  # thread t draws from ids [501 t, 501 t + 501)
        assert len(set((at // 501).tolist())) >= min(copies, 50)
    row[at] = row.max() + np.float32(0.125)
    us = (0.0, 0.5, 0.999999)
    other = make_row(V, seed=99)
    sampled, _, keep, cdf, _ = build_case(other, (1.25, 40, "p*"))
    logits, par, u = [], [], []
    for i, uu in enumerate(us * 2):
        logits += [other, row]
        par += [sampled, (1.0, 1, 1.0) if i < 3 else (1.25, 1, 0.9)]
        u += [0.3, uu]
    logits.append(other)
    par.append(sampled)
    u.append(0.3)
    par = np.array(par, dtype=np.float64)
    u = np.array(u, dtype=np.float32)
    dev = _dev(np.stack(logits), torch.float32)
    tok = _launch(dev, par[:, 0], par[:, 1], par[:, 2], u)
    greedy = native.argmax(dev).cpu().numpy()
    assert greedy[1] == at[0]
    assert tok[1::2].tolist() == [int(at[0])] * 6 == greedy[1::2].tolist()
    check(tok[0::2], u[0::2], keep, cdf)


def test_binding_validates_the_per_row_tensors():
    """A short or misplaced per-row tensor raises before any launch; a longer (bucket-sized) one
    is accepted."""
    rows, V = 4, 256
    x = torch.randn(rows, V, device="cuda")
    it = torch.ones(8, device="cuda")
    tk = torch.zeros(8, device="cuda", dtype=torch.int32)
    tp = torch.ones(8, device="cuda")
    u = torch.full((8,), 0.5, device="cuda")
    assert torch.ops.docqa.sample(x, it, tk, tp, u).shape == (rows,)
    with pytest.raises(RuntimeError, match="u has 3 entries"):
        torch.ops.docqa.sample(x, it, tk, tp, u[:3])
    with pytest.raises(RuntimeError, match="top_p must be on the logits' device"):
        torch.ops.docqa.sample(x, it, tk, tp.cpu(), u)
    with pytest.raises(RuntimeError, match="top_k must be int32"):
        torch.ops.docqa.sample(x, it, tk.long(), tp, u)
    with pytest.raises(RuntimeError, match="inv_temp must be contiguous"):
        torch.ops.docqa.sample(x, torch.ones(16, device="cuda")[::2], tk, tp, u)
