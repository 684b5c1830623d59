"""Repeat / presence / frequency penalties on the GPU: the HIP kernels (apply_penalties,
penalized_argmax, decode_advance_hist) against the fp32 reference -- bitwise, the kernels
round every operation on its own in the reference's order -- and the engine / continuous
scheduler with the ``tiny`` model, eager and graph-captured."""
import pytest
import torch

from docqa_amd import ops
from docqa_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

W = ops.PENALTY_WINDOW
PEN = (1.3, 0.5, 0.2)     # rp, pp, fp of the penalised rows unless a scenario says otherwise


@pytest.fixture(scope="module", autouse=True)
def native():
    assert ops.load_native(build_if_missing=True)
    return ops


def _ring(stream, V=None):
    """Ring row + count of a token stream (entry j at index j % W)."""
    row = [0] * W
    for j, t in enumerate(stream):
        row[j % W] = t
    return row, len(stream)


def _scenarios(V):
    """name -> (stream, last_n, rp, pp, fp, valid)."""
    g = torch.Generator().manual_seed(V)
    rnd = lambda n: torch.randint(0, V, (n,), generator=g).tolist()   # noqa: E731
    s = {
        "empty": ([], 64, *PEN, 1),
        "one_token": ([5], 64, *PEN, 1),
        "partly_filled": (rnd(100), 64, *PEN, 1),
        "wrapped": (rnd(W + 37), 64, *PEN, 1),
        "wrapped_all": (rnd(W + 37), W, *PEN, 1),
        "last_n_0": (rnd(100), 0, *PEN, 1),
        "last_n_1": (rnd(100), 1, *PEN, 1),
        "last_n_gt_hist_n": (rnd(20), 200, *PEN, 1),
        "last_n_minus1": (rnd(2 * W + 3), -1, *PEN, 1),
        "last_n_above_capacity": (rnd(W + 90), W + 100, *PEN, 1),
        "five_times": ([7, 3, 7, 7, 9, 7, 7, 1, 2], 64, *PEN, 1),        # count 5, applied once
        "last_token": (rnd(10) + [V - 1, 4, V - 1], 64, *PEN, 1),
        "out_of_range_ids": ([3, -1, V, 8, V + 5, -7, 3], 64, *PEN, 1),  # -1 / V ignored
        "rp_below_1": (rnd(60), 64, 0.8, 0.0, 0.0, 1),
        "only_presence": (rnd(60), 64, 1.0, 0.7, 0.0, 1),
        "only_frequency": (rnd(30) * 3, W, 1.0, 0.0, 0.3, 1),
        "neutral": (rnd(W + 5), 64, 1.0, 0.0, 0.0, 1),
        "invalid_row": (rnd(100), 64, *PEN, 0),
        # round(round(c * fp) + pp) differs from fma(c, fp, pp) at these counts (see
        # test_apply_penalties_rounds_product_and_sum_separately)
        "unfused_6": ([11] * 6 + [12], 64, 1.0, 0.1, 0.1, 1),
        "unfused_13": ([11] * 13 + [12], 64, 1.0, 0.1, 0.1, 1),
        "unfused_20": ([11] * 20 + [12], 64, 1.0, 0.1, 0.1, 1),
    }
    return s


def _state(rows, dev="cuda"):
    hist = torch.tensor([_ring(r[0])[0] for r in rows], dtype=torch.int32, device=dev)
    hn = torch.tensor([len(r[0]) for r in rows], dtype=torch.int32, device=dev)
    ln = torch.tensor([r[1] for r in rows], dtype=torch.int32, device=dev)
    rp, pp, fp = (torch.tensor([r[k] for r in rows], dtype=torch.float32, device=dev) for k in (2, 3, 4))
    valid = torch.tensor([r[5] for r in rows], dtype=torch.int32, device=dev)
    return hist, hn, ln, rp, pp, fp, valid


def _logits(R, V, seed, rows=None):
    """fp32 logits with positive, negative and zero entries; the window tokens of ``rows``
    get a share of exact zeros too."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, V, generator=g) * 4
    x[:, ::7] = 0.0
    x[:, 3::11] = -0.0
    if rows is not None:
        for r, row in enumerate(rows):
            for t in row[0][::3]:
                if 0 <= t < V:
                    x[r, t] = 0.0
    return x


def _check_apply(rows, V, seed=0, ld=None):
    x = _logits(len(rows), V, seed, rows)
    st = _state(rows)
    want = x.clone()
    ref.apply_penalties(want, *[t.cpu() for t in st])
    if ld is None:
        got = x.cuda()
    else:                       # rows of a wider buffer: row stride above V
        got = torch.full((len(rows), ld), 9.0, device="cuda")[:, :V]
        got.copy_(x)
    ops.apply_penalties(got, *st)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), want)
    untouched = [i for i, r in enumerate(rows) if r[5] == 0 or ref.penalty_neutral(r[1], r[2], r[3], r[4])]
    for i in untouched:         # bitwise: not one byte of a neutral / invalid row changes
        assert torch.equal(got[i].cpu().view(torch.int32), x[i].view(torch.int32))
    changed = [i for i, r in enumerate(rows) if i not in untouched and any(0 <= t < V for t in r[0])]
    for i in changed:
        assert not torch.equal(got[i].cpu(), x[i])
    return got


@pytest.mark.parametrize("name", sorted(_scenarios(1000)))
def test_apply_penalties_one_row(name):
    _check_apply([_scenarios(1000)[name]], 1000)


@pytest.mark.parametrize("R", [3, 64])
def test_apply_penalties_rows(R):
    sc = _scenarios(1000)
    names = sorted(sc)
    # a neutral row beside penalised ones, an invalid one among them
    rows = [sc["neutral"], sc["wrapped"], sc["invalid_row"]] + [sc[names[i % len(names)]] for i in range(R - 3)]
    _check_apply(rows[:R], 1000, seed=R)


def test_apply_penalties_wide_rows_and_full_vocab():
    sc = _scenarios(1000)
    got = _check_apply([sc["wrapped"], sc["neutral"], sc["five_times"]], 1000, seed=5, ld=1024)
    assert bool((got._base[:, 1000:] == 9.0).all())       # nothing past V is touched
    V = 128256
    big = _scenarios(V)
    _check_apply([big["wrapped_all"]], V, seed=6)
    _check_apply([big["last_token"]], V, seed=7)


def test_apply_penalties_five_times_counts_once():
    """One token five times in the window: count 5, penalised exactly once."""
    V = 1000
    row = _scenarios(V)["five_times"]
    x = torch.zeros(1, V)
    x[0, 7], x[0, 3] = 6.5, -2.0
    got = x.cuda()
    ops.apply_penalties(got, *_state([row]))
    rp, pp, fp = (torch.tensor(v, dtype=torch.float32) for v in PEN)
    assert got[0, 7].item() == (torch.tensor(6.5) / rp - (torch.tensor(5.0) * fp + pp)).item()
    assert got[0, 3].item() == (torch.tensor(-2.0) * rp - (torch.tensor(1.0) * fp + pp)).item()
    assert got[0, 0].item() == 0.0 and got[0, 1].item() == (torch.tensor(0.0) * rp - (fp + pp)).item()


def test_apply_penalties_rounds_product_and_sum_separately():
    """c * fp + pp must be two roundings, not one fma: with fp = pp = 0.1 the two differ at
    c = 6 (0.70000005 against 0.69999999).  A zero logit at rp = 1 exposes -(c * fp + pp)."""
    V = 1000
    fp = pp = torch.tensor(0.1, dtype=torch.float32)
    differ = 0
    for c in (6, 13, 20):
        row = _scenarios(V)[f"unfused_{c}"]
        got = torch.zeros(1, V, device="cuda")
        ops.apply_penalties(got, *_state([row]))
        two = torch.tensor(float(c), dtype=torch.float32) * fp + pp           # each op rounded to fp32
        one = (torch.tensor(float(c), dtype=torch.float64) * fp.double() + pp.double()).float()   # the fma
        differ += int(two.item() != one.item())
        assert got[0, 11].item() == -two.item(), (c, got[0, 11].item(), two.item(), one.item())
        assert got[0, 12].item() == -(fp + pp).item()
    assert differ >= 1          # the case tells the two apart


# ------------------------------------------------------------------ penalized_argmax
def _check_argmax(x, rows, n_valid, dtype):
    """ids of the kernel == the reference's on the same (dtype-rounded) logits."""
    x = x.to(dtype)
    st = _state(rows)
    want = ref.penalized_argmax(x, n_valid, *[t.cpu() for t in st])
    dev = x.cuda()
    got = ops.penalized_argmax(dev, n_valid, *st)        # clobbers ``dev``
    torch.cuda.synchronize()
    assert got.dtype == torch.long and got.cpu().tolist() == want.tolist()
    return got.cpu().tolist()


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("n_valid", [1000, 900])
def test_penalized_argmax_planted(dtype, n_valid):
    V = 1000
    g = torch.Generator().manual_seed(1)
    base = (torch.randint(-8, 9, (V,), generator=g).float() * 0.5).clamp(max=4.0)   # exact in bf16, max 4.0
    pres = lambda stream: (stream, 64, 1.0, 8.0, 0.0, 1)   # noqa: E731  presence only: l - 8, exact
    rows, xs, want = [], [], []

    def case(row, edits, expect):
        x = base.clone()
        for i, v in edits.items():
            x[i] = v
        rows.append(row)
        xs.append(x)
        want.append(expect)

    case(pres([500, 20]), {500: 10.0, 300: 5.0}, 300)                 # the winner is in the window and loses
    case(pres([500, 20]), {500: 20.0, 300: 5.0}, 500)                 # ... and still wins
    case(pres([500, 20]), {500: 13.0, 300: 5.0}, 300)                 # ties an unpenalised 5.0 at a lower index
    case(pres([500, 20]), {500: 13.0, 700: 5.0}, 500)                 # ... at a higher index
    win = list(range(40, 50))
    case(pres(win), {t: 50.0 + t for t in win}, 49)                   # every window token above all the rest
    case(pres(win), {t: 50.0 for t in win}, 40)                       # ... tied among themselves
    case((win, 64, 1.0, 0.0, 0.0, 1), {45: 30.0}, 45)                 # neutral: the plain argmax
    case((win, 64, *PEN, 0), {45: 30.0}, 45)                          # invalid row: the plain argmax
    # entries (and window tokens) at or past n_valid never win
    case(pres([950, 20]), {950: 60.0, 990: 70.0, 300: 5.0}, 990 if n_valid == 1000 else 300)
    # nothing but the window is finite: the slice winner is an overwritten window entry, which
    # the merge must drop in favour of the penalised values
    case(pres([10, 20, 30]), {10: 1.0, 20: 2.0, 30: 3.0}, 30)
    xs[-1][[i for i in range(V) if i not in (10, 20, 30)]] = float("-inf")
    x = torch.stack(xs)
    got = _check_argmax(x, rows, n_valid, dtype)
    assert got == want
    # neutral rows equal ops.argmax of the same logits
    neutral = [r for r in range(len(rows)) if rows[r][5] == 0 or rows[r][2:5] == (1.0, 0.0, 0.0)]
    # (as fp32: the bf16 argmax kernel takes widths that are multiples of 8 only)
    plain = ops.argmax(x.to(dtype).float().cuda()[:, :n_valid].contiguous()).cpu().tolist()
    assert [got[r] for r in neutral] == [plain[r] for r in neutral]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("R,V", [(1, 1000), (64, 1000), (2, 128256)])
def test_penalized_argmax_random(dtype, R, V):
    sc = _scenarios(V)
    names = sorted(sc)
    rows = [sc[names[(i * 5 + R) % len(names)]] for i in range(R)]
    x = _logits(R, V, seed=R + V, rows=rows)
    # repeated tokens score high, so the penalties decide the winner in many rows
    for r, row in enumerate(rows):
        for t in row[0][-8:]:
            if 0 <= t < V:
                x[r, t] = 14.0 + (t % 5)
    _check_argmax(x, rows, V, dtype)
    _check_argmax(x, rows, V - 8, dtype)


def test_penalized_argmax_rejects_bad_shapes():
    rows = [_scenarios(1000)["wrapped"]]
    st = _state(rows)
    x = torch.zeros(1, 1000, device="cuda")
    assert torch.ops.docqa.penalty_window() == ops.PENALTY_WINDOW == st[0].shape[1]
    with pytest.raises(RuntimeError):
        ops.penalized_argmax(x, 1001, *st)                       # n_valid > V
    with pytest.raises(RuntimeError):
        ops.penalized_argmax(x, 1000, st[0][:, :128].contiguous(), *st[1:])   # ring narrower than W
    with pytest.raises(RuntimeError):
        ops.apply_penalties(x.bfloat16(), *st)                   # fp32 logits only


# ------------------------------------------------------------------ decode_advance_hist
def test_decode_advance_hist_wraps():
    B, steps = 5, 300
    g = torch.Generator().manual_seed(3)
    valid = torch.tensor([1, 1, 0, 1, 1], dtype=torch.int32)
    names = ("out", "tokens", "positions", "context_lens", "hist", "hist_n")
    cpu = {"out": torch.zeros(B, dtype=torch.long), "tokens": torch.zeros(B, dtype=torch.int32),
           "positions": torch.tensor([3, 0, 9, 100, 7], dtype=torch.int32),
           "context_lens": torch.tensor([4, 1, 10, 101, 8], dtype=torch.int32),
           "hist": torch.randint(0, 1000, (B, W), generator=g, dtype=torch.int32),
           "hist_n": torch.tensor([0, 40, 17, W - 1, 3 * W + 5], dtype=torch.int32)}
    dev = {k: v.cuda() for k, v in cpu.items()}
    vd = valid.cuda()
    for s in range(steps):
        nxt = torch.randint(0, 128256, (B,), generator=g)
        ref.decode_advance_hist(nxt, cpu["out"], cpu["tokens"], cpu["positions"], cpu["context_lens"], valid,
                                cpu["hist"], cpu["hist_n"])
        ops.decode_advance_hist(nxt.cuda(), dev["out"], dev["tokens"], dev["positions"], dev["context_lens"], vd,
                                dev["hist"], dev["hist_n"])
        if s in (0, 1, W - 2, W, steps - 1):
            for k in names:
                assert torch.equal(dev[k].cpu(), cpu[k]), (s, k)
    assert cpu["hist_n"].tolist() == [300, 340, 17, W - 1 + 300, 3 * W + 305]


# ------------------------------------------------------------------ engine, tiny model
NEW, WIN = 96, 64


@pytest.fixture(scope="module")
def tiny():
    from docqa_amd.models.llama import LlamaConfig, LlamaModel

    return LlamaModel(LlamaConfig.preset("tiny"), device="cuda", seed=3)


def _prompts():
    out = []
    for seed in range(4):
        g = torch.Generator().manual_seed(seed)
        out.append(torch.randint(3, 4096, (40,), generator=g).tolist())
    return out


def _repeats(prompt, out, window=WIN):
    """Generated positions whose token occurs among the ``window`` tokens before it."""
    seq = prompt + out
    return [i for i in range(len(prompt), len(seq)) if seq[i] in seq[max(0, i - window):i]]


def _pen_params(new=NEW):
    from docqa_amd.engine.llm_engine import SamplingParams

    return SamplingParams(max_new_tokens=new, stop_on_eos=False, temperature=0.0, presence_penalty=1e4,
                          repeat_last_n=WIN)


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_never_repeats_inside_the_window(tiny, graphs, monkeypatch):
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams

    prompts = _prompts()
    eng = LLMEngine(tiny, max_batch=4, max_context=256, use_graphs=graphs)
    plain = eng.generate(prompts, SamplingParams(max_new_tokens=NEW, stop_on_eos=False))
    # the unpenalised greedy decode of these prompts does repeat inside the window
    assert all(_repeats(p, o) for p, o in zip(prompts, plain))
    pen = eng.generate(prompts, _pen_params())
    assert [len(o) for o in pen] == [NEW] * len(prompts)
    for p, o in zip(prompts, pen):
        assert _repeats(p, o) == []
    assert any(g.penalized and g.greedy for g in eng._graphs.values())
    # a batch-1 run (another bucket, other GEMM kernels) does not repeat either
    assert _repeats(prompts[0], eng.generate(prompts[:1], _pen_params(24))[0]) == []


def test_neutral_request_takes_todays_greedy_path(tiny, monkeypatch):
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams

    prompts = _prompts()[:3]
    eng = LLMEngine(tiny, max_batch=4, max_context=256, use_graphs=True)
    today = eng.generate(prompts, SamplingParams(max_new_tokens=24, stop_on_eos=False))
    keys = set(eng._graphs)
    neutral = [SamplingParams(max_new_tokens=24, stop_on_eos=False, repeat_penalty=1.0, repeat_last_n=64),
               SamplingParams(max_new_tokens=24, stop_on_eos=False, repeat_penalty=1.4, presence_penalty=3.0,
                              repeat_last_n=0)]
    for sp in neutral:
        assert sp.neutral and eng.generate(prompts, sp) == today
    assert set(eng._graphs) == keys and not any(g.penalized for g in eng._graphs.values())


def test_engine_penalised_sampling_never_repeats(tiny, monkeypatch):
    """The penalised sampled flavour, eager and captured (apply_penalties on the fp32 copy in
    front of the sampler): with presence 1e4 no token repeats inside the window.  The two runs
    draw their uniforms differently (the capture's warm-up step draws one), so their tokens
    are not compared."""
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams

    prompts = _prompts()[:2]
    sp = SamplingParams(max_new_tokens=32, stop_on_eos=False, temperature=0.8, top_k=40, seed=5,
                        presence_penalty=1e4, repeat_last_n=WIN)
    outs = [LLMEngine(tiny, max_batch=2, max_context=256, use_graphs=gr).generate(prompts, sp) for gr in (False, True)]
    for o in outs:
        for p, t in zip(prompts, o):
            assert _repeats(p, t) == []


def test_scheduler_moves_rings(tiny, monkeypatch):
    monkeypatch.setenv("DOCQA_TUNE_DECODE", "0")
    from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
    from docqa_amd.engine.scheduler import ContinuousEngine

    eng = LLMEngine(tiny, max_batch=4, max_context=256, use_graphs=True, prefix_cache=False)
    ce = ContinuousEngine(eng)
    base = _prompts()
    g = torch.Generator().manual_seed(9)
    prompts = base + [torch.randint(3, 4096, (40,), generator=g).tolist() for _ in range(4)]
    news = [96, 8, 40, 24, 64, 16]                       # the 6 penalised requests
    specs = [(prompts[i], _pen_params(n)) for i, n in enumerate(news)]
    specs.insert(2, (prompts[6], SamplingParams(max_new_tokens=20, stop_on_eos=False)))    # two neutral ones
    specs.insert(5, (prompts[7], SamplingParams(max_new_tokens=12, stop_on_eos=False)))
    futs = []
    for i, (p, sp) in enumerate(specs):
        futs.append(ce.submit(p, sp))
        for _ in range(1 + i % 3):                       # arrivals while others decode
            ce.step()
    while ce.has_work():
        ce.step()
    for (p, sp), f in zip(specs, futs):
        out = f.result()
        assert len(out) == sp.max_new_tokens
        if not sp.neutral:
            assert _repeats(p, out) == [], (sp.max_new_tokens, _repeats(p, out))
    assert any(gr.penalized for gr in ce._graphs.values())
    assert eng.kv.allocator.num_free() == eng.kv.num_blocks
