"""Scoped exact search on the GPU (csrc/kernels/knn.hip, SCOPED instantiations) against the
fp32 reference ``ops.reference.knn_scoped`` run on the CPU.

Inputs are made on the CPU with a fixed seed and moved to the device.  Shapes are the smallest
that reach every boundary of the 32-row tile, the 128-row pass, the 512-row block and the
32-query workgroup.  Tolerances are test_knn's: 1e-4 (fp32 storage), 1e-2 (bf16 storage).
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

IMIN, IMAX = -(1 << 31), (1 << 31) - 1
UNDATED = IMIN
FMAX = 3.4028234663852886e38
DAY0 = 737000


@pytest.fixture(scope="module", autouse=True)
def native():
    from docqa_amd import ops

    assert ops.load_native(build_if_missing=True), "native extension failed to load"
    assert ops.native_loaded()
    return ops


def _rows(N: int, g: torch.Generator):
    """tags: contiguous runs of 1..40 rows, every fifth run tag 0; days: 100 distinct values,
    about 20 % UNDATED."""
    tags = []
    run = 0
    while len(tags) < N:
        n = int(torch.randint(1, 41, (1,), generator=g))
        tags += [0 if run % 5 == 4 else run + 1] * n
        run += 1
    tags = torch.tensor(tags[:N], dtype=torch.int32)
    days = (DAY0 + torch.randint(0, 100, (N,), generator=g)).int()
    days[torch.rand(N, generator=g) < 0.2] = UNDATED
    return tags, days


def _scopes(nq: int, tags: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    """per query a random mix of any / one tag / tag + alt 0 / tag 0 only / unknown tag, with
    no window / only lo / only hi / both."""
    pos = tags[tags > 0]
    out = []
    for q in range(nq):
        kind = int(torch.randint(0, 5, (1,), generator=g))
        some = int(pos[int(torch.randint(0, len(pos), (1,), generator=g))]) if len(pos) else 1
        tag, alt = [(-1, -1), (some, -1), (some, 0), (0, -1), (IMAX, -1)][kind]
        win = int(torch.randint(0, 4, (1,), generator=g))
        if q == 0:      # the single-query shapes get a scope that some but not all rows match
            (tag, alt), win = (some, 0), 0
        a = DAY0 + int(torch.randint(0, 100, (1,), generator=g))
        b = DAY0 + int(torch.randint(0, 100, (1,), generator=g))
        lo, hi = [(IMIN, IMAX), (min(a, b), IMAX), (IMIN + 1, max(a, b)), (min(a, b), max(a, b))][win]
        out.append((tag, alt, lo, hi))
    return torch.tensor(out, dtype=torch.int32).reshape(nq, 4)


def _vectors(N, d, nq, dtype, g):
    xb = torch.nn.functional.normalize(torch.randn(N, d, generator=g), dim=1).to(dtype)
    xq = torch.nn.functional.normalize(torch.randn(nq, d, generator=g), dim=1)
    return xb, (xb.float() ** 2).sum(1), xq


@functools.lru_cache(maxsize=None)
def _case(N, d, nq, dtype):
    g = torch.Generator().manual_seed(1000 * N + 10 * nq + d)
    xb, norms, xq = _vectors(N, d, nq, dtype, g)
    tags, days = _rows(N, g)
    return xb, norms, tags, days, xq, _scopes(nq, tags, g)


def _match(tags, days, scope) -> np.ndarray:
    rt, rd = tags.numpy().astype(np.int64)[None, :], days.numpy().astype(np.int64)[None, :]
    s = scope.numpy().astype(np.int64)
    tag, alt, lo, hi = (s[:, j:j + 1] for j in range(4))
    return (rt == alt) | (((tag < 0) | (rt == tag)) & (lo <= rd) & (rd <= hi))


def _run(ops, xb, norms, tags, days, xq, scope, k, ip, id_offset=0):
    dev = [t.cuda() for t in (xb, norms, tags, days, xq, scope)]
    D, I = ops.knn_scoped(*dev, k, ip, id_offset)
    torch.cuda.synchronize()
    return D.cpu(), I.cpu()


def _check(D, I, xb, norms, tags, days, xq, scope, k, ip, id_offset=0):
    """The four checks of the module against the CPU oracle, nothing left out."""
    from docqa_amd.ops import reference as R

    tol = 1e-4 if xb.dtype == torch.float32 else 1e-2
    nq, N = xq.shape[0], xb.shape[0]
    assert D.shape == (nq, k) and I.shape == (nq, k) and D.dtype == torch.float32 and I.dtype == torch.int64
    D2, _ = R.knn_scoped(xb, norms, tags, days, xq, scope, k, ip, 0)
    match = _match(tags, days, scope)
    sent = -FMAX if ip else FMAX
    x64, q64 = xb.double(), xq.double()
    for q in range(nq):
        ids = I[q].tolist()
        want = min(k, int(match[q].sum()))
        real = [i - id_offset for i in ids if i >= 0]
        # 1. distinct, inside the scope (exact)
        assert len(set(real)) == len(real), f"query {q}: duplicate ids {ids}"
        assert all(0 <= i < N and match[q, i] for i in real), f"query {q}: id outside its scope {ids} {scope[q].tolist()}"
        # 2. min(k, matching) hits first, then -1 with the sentinel distance (exact)
        assert len(real) == want and all(i >= 0 for i in ids[:want]), f"query {q}: {ids}, {want} rows match"
        assert all(i == -1 for i in ids[want:]) and all(v == sent for v in D[q, want:].tolist())
        if want == 0:
            continue
        # 3. distances at the oracle's rank
        err = (D[q, :want] - D2[q, :want]).abs().max().item()
        assert err <= tol, f"query {q}: distance error {err} > {tol}"
        # 4. the returned neighbours, recomputed in fp64 from the stored vectors
        sel = x64[torch.tensor(real)]
        rec = (sel @ q64[q]) if ip else ((sel - q64[q][None, :]) ** 2).sum(1)
        err = (rec - D2[q, :want].double()).abs().max().item()
        assert err <= tol, f"query {q}: wrong neighbour, recomputed distance off by {err} > {tol}"


# every N, nq and k in both storage types; d and the metric alternate
SHAPES = [
    (1, 32, 1, 1, False), (1, 384, 33, 3, True),
    (31, 32, 33, 3, False), (31, 384, 70, 64, True),
    (33, 384, 1, 10, False), (33, 32, 70, 1, True),
    (129, 32, 70, 64, False), (129, 384, 33, 10, True),
    (513, 384, 33, 3, False), (513, 32, 1, 1, True),
    (1100, 384, 70, 10, False), (1100, 32, 33, 64, True), (1100, 32, 1, 3, False), (1100, 384, 70, 1, True),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,d,nq,k,ip", SHAPES)
def test_scoped_vs_reference(native, N, d, nq, k, ip, dtype):
    case = _case(N, d, nq, dtype)
    D, I = _run(native, *case, k, ip)
    _check(D, I, *case, k, ip)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
@pytest.mark.parametrize("window", [False, True], ids=["tag", "window"])
def test_decoys(native, dtype, ip, window):
    """Every non-matching row is an exact copy of a query: any leak wins rank 0."""
    N, d, nq, k = 1100, 32, 33, 10
    g = torch.Generator().manual_seed(7)
    xb, _, xq = _vectors(N, d, nq, dtype, g)
    tags, days = _rows(N, g)
    days[days == UNDATED] = DAY0 + 50
    if window:
        scope = torch.tensor([(-1, -1, DAY0 + 20, DAY0 + 60)] * nq, dtype=torch.int32)
    else:
        scope = torch.tensor([(int(tags[600]), -1, IMIN, IMAX)] * nq, dtype=torch.int32)
    inside = torch.from_numpy(_match(tags, days, scope)[0])
    assert 0 < int(inside.sum()) < N
    out = (~inside).nonzero()[:, 0]
    xb[out] = xq[out % nq].to(dtype)
    norms = (xb.float() ** 2).sum(1)
    D, I = _run(native, xb, norms, tags, days, xq, scope, k, ip)
    _check(D, I, xb, norms, tags, days, xq, scope, k, ip)
    assert inside[I[I >= 0]].all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,d,nq,k,ip", [(1100, 384, 70, 10, False), (513, 32, 33, 64, True), (31, 32, 1, 3, False)])
def test_any_scope_equals_knn(native, N, d, nq, k, ip, dtype):
    """The any-scope runs the same arithmetic as the unscoped kernel: bit-equal distances."""
    xb, norms, tags, days, xq, _ = _case(N, d, nq, dtype)
    scope = torch.tensor([(-1, -1, IMIN, IMAX)] * nq, dtype=torch.int32)
    D, I = _run(native, xb, norms, tags, days, xq, scope, k, ip)
    Dk, Ik = native.knn(xb.cuda(), norms.cuda(), xq.cuda(), k, ip, 0)
    assert torch.equal(I, Ik.cpu())
    assert torch.equal(D, Dk.cpu())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("row", [1099, 0])
def test_single_matching_row(native, row, dtype):
    """The only matching row is the last row of the partial last tile / the first row."""
    N, d, nq, k = 1100, 32, 33, 3
    xb, norms, _, days, xq, _ = _case(N, d, nq, dtype)
    tags = torch.ones(N, dtype=torch.int32)
    tags[row] = 7
    scope = torch.tensor([(7, -1, IMIN, IMAX)] * nq, dtype=torch.int32)
    for ip in (False, True):
        D, I = _run(native, xb, norms, tags, days, xq, scope, k, ip)
        _check(D, I, xb, norms, tags, days, xq, scope, k, ip)
        assert (I[:, 0] == row).all() and (I[:, 1:] == -1).all()


def test_per_lane_scopes(native):
    """Thirty-three queries, each scoped to a different single row: scopes are per lane."""
    N, d, nq, k = 1100, 32, 33, 3
    xb, norms, _, days, xq, _ = _case(N, d, nq, torch.float32)
    tags = torch.arange(1, N + 1, dtype=torch.int32)
    rows = (torch.arange(nq) * 33 + 5) % N
    rows[-1] = N - 1
    scope = torch.tensor([(int(tags[r]), -1, IMIN, IMAX) for r in rows], dtype=torch.int32)
    D, I = _run(native, xb, norms, tags, days, xq, scope, k, False)
    _check(D, I, xb, norms, tags, days, xq, scope, k, False)
    assert torch.equal(I[:, 0], rows) and (I[:, 1:] == -1).all()


@pytest.mark.parametrize("ip", [False, True], ids=["l2", "ip"])
def test_empty_scope(native, ip):
    N, d, nq, k = 513, 32, 33, 10
    xb, norms, tags, days, xq, _ = _case(N, d, nq, torch.float32)
    scope = torch.tensor([(IMAX, -1, IMIN, IMAX)] * nq, dtype=torch.int32)
    D, I = _run(native, xb, norms, tags, days, xq, scope, k, ip)
    assert (I == -1).all() and (D == (-FMAX if ip else FMAX)).all()


def test_id_offset(native):
    N, d, nq, k = 129, 32, 70, 64
    case = _case(N, d, nq, torch.float32)
    D0, I0 = _run(native, *case, k, False)
    D1, I1 = _run(native, *case, k, False, id_offset=1000)
    assert (I0 == -1).any() and (I0 >= 0).any()
    assert torch.equal(I1, torch.where(I0 >= 0, I0 + 1000, I0)) and torch.equal(D0, D1)
    _check(D1, I1, *case, k, False, id_offset=1000)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_kill_switch(native, monkeypatch, dtype):
    """DOCQA_KNN_SCOPED=0: GPU calls take the reference on the device, same contract."""
    monkeypatch.setenv("DOCQA_KNN_SCOPED", "0")
    for N, d, nq, k, ip in [(1100, 384, 70, 10, False), (129, 32, 33, 64, True)]:
        case = _case(N, d, nq, dtype)
        D, I = _run(native, *case, k, ip)
        assert D.dtype == torch.float32 and I.dtype == torch.int64
        _check(D, I, *case, k, ip)


def test_outside_envelope_takes_reference(native):
    """d % 8 != 0 and k > 64 are served by the reference on the same device, not refused."""
    g = torch.Generator().manual_seed(3)
    xb, norms, xq = _vectors(129, 20, 5, torch.float32, g)
    tags, days = _rows(129, g)
    scope = _scopes(5, tags, g)
    for k in (3, 70):
        D, I = _run(native, xb, norms, tags, days, xq, scope, k, False)
        _check(D, I, xb, norms, tags, days, xq, scope, k, False)
