"""format: a JSON schema, without a GPU: the schema compiler against pydantic and a hand-written
validator, the compiler's properties, the reference ops against a brute-force walk, the engine
(static batcher and the scheduler with the GPU's lagged readback) on the tiny CPU preset, and the
Ollama routes.

All comparisons are exact: sets of allowed ids, int64 state words, token ids."""
from __future__ import annotations

import json
import random

import numpy as np
import pytest
import torch

from docqa_amd import ops
from docqa_amd.config import Settings
from docqa_amd.engine.llm_engine import LLMEngine, SamplingParams
from docqa_amd.engine.scheduler import ContinuousEngine
from docqa_amd.models.llama import LlamaConfig, LlamaModel
from docqa_amd.ops import grammar as G
from docqa_amd.ops import json_schema as J
from tests.format_json_common import EOS_SYN, max_ws_run, mutate
from tests.format_schema_common import (SERVICE_SCHEMA, SMALL_SCHEMA, big_schema, cases, coverage_words,
                                        gen_documents, schema_engine_vocab, schema_vocab)

CASES = list(cases())


# ------------------------------------------------------------------ the compiler against the oracles
@pytest.mark.parametrize("name", CASES)
def test_completeness(name):
    """Every generated document (declared order, the four json.dumps styles, numbers inside the
    caps) is accepted -- and the oracle agrees that it is valid."""
    schema, oracle = cases()[name]
    cs = J.compile_schema(schema)
    docs = gen_documents(schema, 400, seed=1)
    assert len(set(docs)) > 40 or name == "service"
    for d in docs:
        assert max_ws_run(d) <= G.WS_CAP
        assert oracle(d), d
        assert J.accepts(cs, d), d


@pytest.mark.parametrize("name", CASES)
def test_soundness_under_mutations(name):
    """Whatever the automaton accepts validates under the oracle; 20 mutants per document, and a
    non-trivial share of them is rejected by both (the test cannot pass vacuously)."""
    schema, oracle = cases()[name]
    cs = J.compile_schema(schema)
    rng = random.Random(7)
    n = accepted = invalid = 0
    for d in gen_documents(schema, 150, seed=2):
        for _ in range(20):
            m = mutate(d, rng)
            n += 1
            valid = oracle(m)
            invalid += not valid
            if J.accepts(cs, m):
                accepted += 1
                assert valid, m
    assert n == 3000 and invalid >= 0.3 * n and accepted >= 0.03 * n, (n, invalid, accepted)


def test_language_details():
    cs = J.compile_schema(SERVICE_SCHEMA)
    ok = lambda d: J.accepts(cs, d)   # noqa: E731
    assert ok(b'{"verdict":"oui","score":-12,"ok":true}')
    assert ok(b'{ "verdict" :\t"non" ,\n"score": 0 , "ok" : false\r\n}')
    for bad in (b' {"verdict":"oui","score":1,"ok":true}', b'{"verdict":"oui","score":1,"ok":true} ',
                b'{"score":1,"verdict":"oui","ok":true}', b'{"verdict":"oui","score":1}',
                b'{"verdict":"Oui","score":1,"ok":true}', b'{"verdict":"oui","score":01,"ok":true}',
                b'{"verdict":"oui","score":1.0,"ok":true}', b'{"verdict":"oui","score":1,"ok":true,"x":1}',
                b'{"verdict":"oui","score":12345678901234567,"ok":true}', b'{"verdict":"\\u006fui","score":1,"ok":true}',
                b'{"verdict":"oui","score":1,"ok":true' + b' ' * (G.WS_CAP + 1) + b'}'):
        assert not ok(bad), bad
    assert ok(b'{"verdict":"oui","score":1234567890123456,"ok":true' + b' ' * G.WS_CAP + b'}')
    # keys and enum values: the minimal literal, raw UTF-8, no \u spelling
    cs = J.compile_schema({"type": "object", "properties": {"clé\n": {"enum": ["é中", 1.5, None]}}, "required": ["clé\n"]})
    assert J.accepts(cs, '{"clé\\n":"é中"}'.encode()) and J.accepts(cs, '{"clé\\n":1.5}'.encode())
    assert not J.accepts(cs, b'{"cl\\u00e9\\n":null}') and J.accepts(cs, '{"clé\\n":null}'.encode())
    # number caps
    cs = J.compile_schema({"type": "object", "properties": {"x": {"type": "number"}}, "required": ["x"]})
    num = lambda t: J.accepts(cs, b'{"x":' + t + b'}')   # noqa: E731
    assert num(b"-0.5e+10") and num(b"1E-999") and num(b"0." + b"1" * 16) and num(b"9" * 16)
    assert not num(b"0." + b"1" * 17) and not num(b"1e1000") and not num(b"9" * 17) and not num(b"1.") \
        and not num(b"-") and not num(b"+1") and not num(b".5") and not num(b"1e")
    # the finite language's longest document
    cs = J.compile_schema(SERVICE_SCHEMA)
    assert cs.max_document_len() == len(b'{"verdict":"oui","score":-1234567890123456,"ok":false}') + 12 * G.WS_CAP
    assert J.compile_schema(cases()["Answer"][0]).max_document_len() is None


# ------------------------------------------------------------------ compiler properties
@pytest.mark.parametrize("name", CASES + ["big"])
def test_no_dead_state_and_shape(name):
    schema = big_schema() if name == "big" else cases()[name][0]
    cs = J.compile_schema(schema, cache=False)
    assert cs.cls.dtype == np.uint8 and cs.cls.shape == (256,) and cs.trans.dtype == np.uint16
    assert cs.trans.shape == (cs.n_states, cs.n_classes) and int(cs.cls.max()) == cs.n_classes - 1
    assert cs.n_states <= J.MAX_STATES and cs.n_states * cs.n_classes <= J.MAX_CELLS
    t = cs.trans.astype(np.int64)
    assert not t[0].any() and not t[J.DONE].any()
    nxt = t & J.NEXT_MASK
    assert int(nxt.max()) < cs.n_states
    # every state but DONE accepts a byte that is no whitespace (so also at the whitespace cap) ...
    plain = (t != 0) & (t & J.WS_FLAG == 0)
    assert plain[2:].any(axis=1).all()
    # ... and reaches DONE
    live = np.zeros(cs.n_states, dtype=bool)
    live[J.DONE] = True
    for _ in range(cs.n_states):
        grow = live | (live[nxt] & (t != 0)).any(axis=1)
        if (grow == live).all():
            break
        live = grow
    assert live[1:].all()
    # whitespace entries: exactly the four whitespace bytes' classes
    ws_cls = {int(cs.cls[b]) for b in G.WS_BYTES}
    assert set(np.nonzero((t & J.WS_FLAG).any(axis=0))[0].tolist()) <= ws_cls
    # deterministic
    again = J.compile_schema(json.loads(json.dumps(schema)), cache=False)
    assert np.array_equal(again.cls, cs.cls) and np.array_equal(again.trans, cs.trans)
    if name == "big":
        assert cs.n_states * cs.n_classes >= 0.75 * J.MAX_CELLS        # near the cap


def test_cache_is_an_lru_by_canonical_text():
    s = {"type": "object", "properties": {"a": {"type": "null"}}}
    assert J.compile_schema(s) is J.compile_schema(json.loads(json.dumps(s)))
    assert J.compile_schema(s, cache=False) is not J.compile_schema(s)


def test_size_cap_raises():
    many = {"type": "object", "properties": {f"k{i}": {"type": ["number", "string", "null"]} for i in range(200)}}
    with pytest.raises(ValueError, match="schema too large"):
        J.compile_schema(many)
    with pytest.raises(ValueError, match="schema too large"):
        J.compile_schema({"type": "object", "properties": {"a": {"type": "array", "items": {"type": "number"},
                                                                 "maxItems": 100000}}})


def _obj(sub, **kw):
    return {"type": "object", "properties": {"a": sub}, **kw}


UNSUPPORTED = [
    (_obj({"type": "string", "pattern": "^x"}), "#/properties/a/pattern"),
    (_obj({"type": "string", "minLength": 1}), "#/properties/a/minLength"),
    (_obj({"type": "string", "maxLength": 3}), "#/properties/a/maxLength"),
    (_obj({"type": "string", "format": "date"}), "#/properties/a/format"),
    (_obj({"type": "integer", "minimum": 0}), "#/properties/a/minimum"),
    (_obj({"type": "number", "maximum": 1}), "#/properties/a/maximum"),
    (_obj({"type": "number", "multipleOf": 2}), "#/properties/a/multipleOf"),
    (_obj({"type": "object"}), "#/properties/a"),
    (_obj({"type": "object", "properties": {}, "additionalProperties": True}), "#/properties/a/additionalProperties"),
    (_obj({"type": "object", "properties": {}, "additionalProperties": {"type": "string"}}),
     "#/properties/a/additionalProperties"),
    (_obj({"type": "array"}), "#/properties/a"),
    (_obj({"type": "array", "items": {"type": "string"}, "uniqueItems": True}), "#/properties/a/uniqueItems"),
    (_obj({"type": "array", "prefixItems": [{"type": "string"}]}), "#/properties/a/prefixItems"),
    (_obj({}), "#/properties/a"),
    (_obj({"type": "float"}), "#/properties/a/type"),
    (_obj({"enum": [[1]]}), "#/properties/a/enum"),
    (_obj({"const": {"x": 1}}), "#/properties/a/const"),
    (_obj({"allOf": [{"type": "string"}, {"type": "null"}]}), "#/properties/a/allOf"),
    (_obj({"not": {"type": "string"}}), "#/properties/a/not"),
    (_obj({"$ref": "#/$defs/missing"}), "#/properties/a/$ref"),
    (_obj({"$ref": "http://example.com/x.json"}), "#/properties/a/$ref"),
    (_obj({"$ref": "#/$defs/T"}, **{"$defs": {"T": _obj({"$ref": "#/$defs/T"})}}), "#/$defs/T/properties/a/$ref"),
    (_obj({"type": "string"}, additionalProperties=True), "#/additionalProperties"),
    (_obj({"type": "string"}, required=["b"]), "#/required"),
    (_obj({"type": "string"}, patternProperties={"x": {}}), "#/patternProperties"),
    ({"type": "array", "items": {"type": "string"}}, "#"),
    ({"type": "string"}, "#"),
    ({"anyOf": [_obj({"type": "string"}), {"type": "null"}]}, "#"),
]


@pytest.mark.parametrize("schema,pointer", UNSUPPORTED, ids=[p + "-" + str(i) for i, (_, p) in enumerate(UNSUPPORTED)])
def test_unsupported_keywords_raise_with_their_pointer(schema, pointer):
    with pytest.raises(ValueError) as e:
        J.compile_schema(schema)
    assert f"at {pointer}:" in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        SamplingParams(format="json", json_schema=schema)


def test_sampling_params():
    sp = SamplingParams(format="json", json_schema=SERVICE_SCHEMA)
    assert sp.constrained and sp.schema_constrained and not sp.fused_greedy_ok
    assert sp.compiled_schema is J.compile_schema(SERVICE_SCHEMA)
    plain = SamplingParams(format="json")
    assert plain.constrained and not plain.schema_constrained and plain.compiled_schema is None
    with pytest.raises(ValueError):
        SamplingParams(json_schema=SERVICE_SCHEMA)                 # needs format "json"
    # $ref and single allOf resolve, also at the root
    s = {"$ref": "#/definitions/R", "definitions": {"R": {"allOf": [_obj({"$ref": "#/definitions/S"})]},
                                                    "S": {"type": "boolean", "title": "S"}}}
    assert J.accepts(J.compile_schema(s), b'{"a":true}')


# ------------------------------------------------------------------ reference ops
def _pool_with(schemas, n_slots=4):
    pool = J.pool_new(n_slots)
    for slot, cs in schemas.items():
        J.pool_put(pool, slot, cs)
    return pool


def test_reference_mask_and_advance_match_brute_force():
    toks = list(schema_vocab())
    V = len(toks)
    assert 3000 <= V <= 6000 and V % 64 != 0
    off, data = G.vocab_tensors(toks)
    by_slot = {1: J.compile_schema(SERVICE_SCHEMA), 3: J.compile_schema(cases()["arrays"][0])}
    pool = _pool_with(by_slot)
    words, owner = [], []
    for slot, cs in by_slot.items():
        w = coverage_words(cs, slot)
        assert {J.unpack(x)[0] for x in w} == set(range(1, cs.n_states))
        words += w
        owner += [cs] * len(w)
    # a slot that holds nothing, a slot past the pool, a state past the table: nothing is allowed
    nothing = [J.pack(J.START, 0, 2), J.pack(J.START, 0, 9), J.pack(by_slot[1].n_states + 3, 0, 1)]
    R = len(words) + len(nothing) + 2
    x0 = torch.randn(R, V + 5)
    x = x0.clone()
    st = torch.tensor(words + nothing + [0, words[5]], dtype=torch.int64)
    valid = torch.ones(R, dtype=torch.int32)
    valid[-1] = 0
    ops.schema_mask(x, V, st, off, data, pool, EOS_SYN, valid)
    got = (x[:, :V] != -float("inf")).numpy()
    some_multi = 0
    for r, (w, cs) in enumerate(zip(words, owner)):
        want = [J.token_allowed(cs, w, t, toks, EOS_SYN) for t in range(V)]
        assert got[r].tolist() == want, J.unpack(w)
        assert any(want) and want[EOS_SYN] == J.is_done(w)        # no state is left without a token
        some_multi += any(a and len(toks[t]) > 1 for t, a in enumerate(want))
    assert some_multi > len(words) // 4
    assert not got[len(words):len(words) + len(nothing)].any()
    keep = x != -float("inf")
    assert torch.equal(x[keep], x0[keep]) and torch.equal(x[-2:], x0[-2:]) and torch.equal(x[:, V:], x0[:, V:])
    # advance: every (word, token) pair
    for w, cs in zip(words, owner):
        got = torch.full((V,), w, dtype=torch.int64)
        ops.schema_advance(got, torch.arange(V), off, data, pool, EOS_SYN)
        assert got.tolist() == [J.advance_token(cs, w, t, toks, EOS_SYN) for t in range(V)]
    done = J.pack(J.DONE, 0, 1)
    z = torch.tensor([0, words[0], done, nothing[0], nothing[1]], dtype=torch.int64)
    ops.schema_advance(z, torch.tensor([300, 300, EOS_SYN, 3 + 0x7B, 3 + 0x7B]), off, data, pool, EOS_SYN,
                       torch.tensor([1, 0, 1, 1, 1], dtype=torch.int32))
    assert z.tolist() == [0, words[0], done, nothing[0], nothing[1]]
    # replay: token by token from the start word of a slot
    doc = b'{"verdict":"oui","score":12,"ok":true}'
    ids = [toks.index(bytes([b])) for b in doc]
    assert J.is_done(J.replay(by_slot[1], ids + [EOS_SYN], toks, EOS_SYN, J.start_state(1)))
    assert J.unpack(J.replay(by_slot[1], ids[:5], toks, EOS_SYN, J.start_state(1)))[2] == 1


# ------------------------------------------------------------------ engine
def _model(seed=7):
    cfg = LlamaConfig(name="tiny-gqa4", vocab_size=4096, hidden=256, intermediate=512, layers=2,
                      heads=8, kv_heads=2, head_dim=128, max_position=2048, bos_token_id=1, eos_token_id=2)
    return LlamaModel(cfg, device="cpu", dtype=torch.float32, seed=seed)


VOCAB = schema_engine_vocab(4096)
EOS = 2
SCHEMAS = {"A": SERVICE_SCHEMA, "B": SMALL_SCHEMA,
           "C": {"type": "object", "properties": {"v": {"enum": ["x", 1, None]}}, "required": ["v"]}}
ORACLE = {"A": cases()["service"][1]}


def _len(name: str) -> int:
    return J.compile_schema(SCHEMAS[name]).max_document_len()


def _prompts(lens, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(3, 4096, (int(n),), generator=g).tolist() for n in lens]


def _engine(m, **kw):
    e = LLMEngine(m, max_batch=8, max_context=512, block_size=16, use_graphs=False, prefix_cache=False, **kw)
    e.set_vocab_bytes(VOCAB)
    return e


def check_schema_row(out: list, name: str, max_new: int) -> bool:
    """Replay a schema-constrained output token by token; one that ended on EOS validates."""
    cs = J.compile_schema(SCHEMAS[name])
    w = J.start_state()
    for t in out:
        assert J.token_allowed(cs, w, t, VOCAB, EOS), (name, t, VOCAB[t], J.unpack(w))
        w = J.advance_token(cs, w, t, VOCAB, EOS)
    if out[-1] == EOS:
        assert J.is_done(w)
        doc = b"".join(VOCAB[t] for t in out)
        assert J.accepts(cs, doc)
        v = json.loads(doc.decode("utf-8"))
        assert isinstance(v, dict)
        if name in ORACLE:
            assert ORACLE[name](doc), doc
        return True
    assert len(out) == max_new
    return False


def check_json_row(out: list, max_new: int) -> None:
    s = G.START_STATE
    for t in out:
        assert G.token_allowed(s, t, VOCAB, EOS)
        s = G.advance_token(s, t, VOCAB, EOS)
    assert out[-1] == EOS or len(out) == max_new


FLAVOURS = {
    "greedy": dict(),
    "penalised": dict(repeat_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2, repeat_last_n=32),
    "sampled": dict(temperature=4.0, seed=11),
    "logprobs": dict(logprobs=True, top_logprobs=3),
}


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_static_batcher_constrains_every_row(flavour):
    m = _model()
    n = _len("B")
    sp = SamplingParams(max_new_tokens=n + 1, format="json", json_schema=SCHEMAS["B"], **FLAVOURS[flavour])
    eng = _engine(m)
    prompts = _prompts((20, 31, 12))
    if sp.logprobs:
        outs, lps = eng.generate_with_logprobs(prompts, sp)
        assert all(len(o) == len(l) for o, l in zip(outs, lps))
    else:
        outs = eng.generate(prompts, sp)
    assert eng._graphs_schema and not eng._graphs_json and not eng._graphs and not eng._graphs_min_p
    # the language is finite and max_new_tokens covers its longest document: every row closes
    assert all(check_schema_row(o, "B", sp.max_new_tokens) for o in outs)
    assert eng.schema_slots.refs == [0] * eng.schema_slots.n and eng.schema_slots.uploads == 1
    # the plain-JSON flavour of the same engine is still its own
    eng.generate(prompts[:1], SamplingParams(max_new_tokens=4, format="json"))
    assert eng._graphs_json


def _run_mixed(m, which: str, **kw):
    """One scheduler with the GPU's lagged readback: two rows on schema A, two on schema B (greedy,
    penalised, sampled, greedy with logprobs), two plain-JSON rows and two unconstrained ones."""
    pr = _prompts((20, 31, 12, 25, 18, 9, 27, 14))
    nA, nB = _len("A") + 1, _len("B") + 1
    schema = [SamplingParams(max_new_tokens=nA, format="json", json_schema=SCHEMAS["A"]),
              SamplingParams(max_new_tokens=nB, format="json", json_schema=SCHEMAS["B"], **FLAVOURS["penalised"]),
              SamplingParams(max_new_tokens=nA, format="json", json_schema=SCHEMAS["A"], **FLAVOURS["sampled"]),
              SamplingParams(max_new_tokens=nB, format="json", json_schema=SCHEMAS["B"], **FLAVOURS["logprobs"])]
    plain = [SamplingParams(max_new_tokens=24, format="json"),
             SamplingParams(max_new_tokens=24, format="json", **FLAVOURS["sampled"])]
    free = [SamplingParams(max_new_tokens=24, stop_on_eos=False),
            SamplingParams(max_new_tokens=24, stop_on_eos=False, logprobs=True, top_logprobs=2)]
    ce = ContinuousEngine(_engine(m, **kw))
    ce.lag_cpu = True
    fs = []
    if "schema" in which:
        fs = [ce.submit(p, sp) for p, sp in zip(pr[:4], schema)]
        ce.step()
    fp = [ce.submit(p, sp) for p, sp in zip(pr[4:6], plain)] if "plain" in which else []
    ff = [ce.submit(p, sp) for p, sp in zip(pr[6:], free)]
    while ce.has_work():
        ce.step()
    return ce, fs, fp, ff, schema


def test_scheduler_mixed_batch():
    m = _model()
    ce, fs, fp, ff, specs = _run_mixed(m, "schema plain")
    assert any(len(k) == 7 and k[-1] == "schema" for k in ce._graphs)
    for f, sp, name in zip(fs, specs, "ABAB"):
        assert check_schema_row(f.result(), name, sp.max_new_tokens)     # finite languages: all close
    for f in fp:
        check_json_row(f.result(), 24)
    assert ce.eng.schema_slots.refs == [0] * 8 and ce.eng.schema_slots.uploads == 2
    # without the schema rows: the plain-JSON and the free rows get the same tokens, and no graph
    # of the schema flavour exists
    ce0, _, fp0, ff0, _ = _run_mixed(m, "plain")
    assert all(len(k) == 6 or k[-1] == "json" for k in ce0._graphs) and ce0.eng.schema_slots.uploads == 0
    assert [f.result() for f in fp] == [f.result() for f in fp0]
    assert [f.result() for f in ff] == [f.result() for f in ff0]
    assert ff[1].request.logprobs == ff0[1].request.logprobs
    # without any constrained row: the keys of before
    ce1, _, _, ff1, _ = _run_mixed(m, "")
    assert all(len(k) == 6 for k in ce1._graphs)
    assert [f.result() for f in ff] == [f.result() for f in ff1]


def test_step_without_schema_rows_launches_no_schema_op(monkeypatch):
    calls = []
    for name in ("schema_mask", "schema_advance"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _r=real, **k: (calls.append(_n), _r(*a, **k))[1])
    m = _model()
    _run_mixed(m, "plain")
    assert not calls
    _run_mixed(m, "schema")
    assert {"schema_mask", "schema_advance"} <= set(calls)


def test_preempted_schema_request_resumes_its_state():
    m = _model()
    pr = _prompts((28, 20, 35, 9, 50, 17))
    n = _len("A") + 1
    a = SamplingParams(max_new_tokens=n, format="json", json_schema=SCHEMAS["A"], temperature=4.0, seed=5)
    others = [SamplingParams(max_new_tokens=k, stop_on_eos=False) for k in (30, 40, 25, 40, 35)]
    alone = ContinuousEngine(_engine(m)).generate([pr[0]], a)[0]
    ce = ContinuousEngine(_engine(m, num_blocks=20), max_running=8)
    ce.lag_cpu = True
    for p, sp in zip(pr[1:], others):
        ce.submit(p, sp)
    fa = ce.submit(pr[0], a)                      # the latest arrival: the first to be preempted
    while ce.has_work():
        ce.step()
    assert ce.preempted > 0 and fa.request.preemptions > 0
    assert fa.result() == alone and check_schema_row(alone, "A", n)
    assert ce.eng.schema_slots.refs == [0] * 8


def test_third_schema_waits_for_a_table_slot(monkeypatch):
    monkeypatch.setenv("DOCQA_SCHEMA_SLOTS", "2")
    m = _model()
    ce = ContinuousEngine(_engine(m))
    assert ce.eng.schema_slots.n == 2
    ce.lag_cpu = True
    pr = _prompts((20, 31, 12, 16))
    names = ["A", "B", "C", "B"]
    sps = [SamplingParams(max_new_tokens=_len(k) + 1, format="json", json_schema=SCHEMAS[k], temperature=4.0, seed=3)
           for k in names]
    fs = [ce.submit(p, sp) for p, sp in zip(pr, sps)]
    ce.step()
    # A and B hold the two slots; C is queued behind them, and so is the second B (the queue is
    # first in, first out) although its schema is resident
    assert [r.params.schema_key for r in ce.running] == [sp.schema_key for sp in sps[:2]]
    assert len(ce.waiting) == 2 and ce.schema_blocked >= 1 and ce.eng.schema_slots.refs == [1, 1]
    while ce.has_work():
        ce.step()
    for f, sp, k in zip(fs, sps, names):
        assert check_schema_row(f.result(), k, sp.max_new_tokens)
    assert ce.eng.schema_slots.refs == [0, 0] and ce.eng.schema_slots.uploads >= 3
    # the assignment is a function of the request sequence: a second run takes the same slots
    ce2 = ContinuousEngine(_engine(m))
    ce2.lag_cpu = True
    fs2 = [ce2.submit(p, sp) for p, sp in zip(pr, sps)]
    while ce2.has_work():
        ce2.step()
    assert [f.result() for f in fs2] == [f.result() for f in fs]
    assert ce2.eng.schema_slots.keys == ce.eng.schema_slots.keys


def test_schema_request_needs_plain_steps(monkeypatch):
    m = _model()
    monkeypatch.setenv("DOCQA_MIXED_PREFILL", "1")
    ce = ContinuousEngine(_engine(m))
    assert ce.mixed
    with pytest.raises(ValueError):
        ce.submit(_prompts((10,))[0], SamplingParams(max_new_tokens=4, format="json", json_schema=SCHEMAS["B"]))


# ------------------------------------------------------------------ service
def _stack(tmp_path):
    from docqa_amd.services.stack import DocQAStack, StackOptions

    st = Settings()
    st.index_dir = str(tmp_path)
    st.default_data_dir = str(tmp_path / "nodata")
    st.database_url = "sqlite://"
    st.max_new_tokens = 6
    st.serving_mode = "continuous"
    return DocQAStack(StackOptions(llm="tiny", embed="tiny-bert", ner="tiny-bert", device="cpu",
                                   max_batch=4, max_context=1024, use_graphs=False), st)


def test_service_format_schema(tmp_path):
    """The schema is enforced: with num_predict at the finite language's longest document every
    request ends by EOS and its text validates."""
    from fastapi.testclient import TestClient

    oracle = cases()["service"][1]
    longest = J.compile_schema(SERVICE_SCHEMA).max_document_len()
    assert 200 < longest < 300
    s = _stack(tmp_path)
    try:
        qa = TestClient(s.qa_app)
        eng, tok = s.pipeline.engine, s.pipeline.chat_tok
        for seed in range(1, 7):
            opts = {"temperature": 3.0, "seed": seed, "num_predict": longest}
            r = qa.post("/api/chat", json={"model": "mistral", "format": SERVICE_SCHEMA, "stream": False,
                                           "options": opts, "messages": [{"role": "user", "content": "Rate ?"}]})
            assert r.status_code == 200
            d = r.json()
            assert d["done_reason"] == "stop", d
            assert oracle(d["message"]["content"].encode("utf-8")), d["message"]["content"]
            assert list(json.loads(d["message"]["content"])) == ["verdict", "score", "ok"]
            r = qa.post("/api/generate", json={"prompt": "Rate ?", "format": SERVICE_SCHEMA, "stream": True,
                                               "options": opts})
            assert r.status_code == 200
            lines = [json.loads(x) for x in r.text.splitlines() if x]
            text = "".join(x.get("response", "") for x in lines)
            assert lines[-1]["done_reason"] == "stop", lines[-1]
            assert oracle(text.encode("utf-8")), text
        # an unsupported schema: 400, the keyword named
        bad = {"type": "object", "properties": {"a": {"type": "string", "pattern": "^a"}}}
        for route, body in (("/api/chat", {"messages": [{"role": "user", "content": "x"}]}),
                            ("/api/generate", {"prompt": "x"})):
            r = qa.post(route, json={**body, "format": bad, "stream": False})
            assert r.status_code == 400 and "#/properties/a/pattern" in r.json()["error"]
        # "json" is the plain JSON automaton as before; absent / null / "": the engine's own completion
        r = qa.post("/api/generate", json={"prompt": "Rate ?", "format": "json", "stream": False,
                                           "options": {"num_predict": 5}})
        assert r.status_code == 200 and r.json()["response"].lstrip().startswith("{")
        for fmt in ({}, {"format": None}, {"format": ""}):
            r = qa.post("/api/generate", json={"prompt": "Vide de Qi ?", "stream": False,
                                               "options": {"num_predict": 8}, **fmt})
            ids = tok.chat_prompt("Vide de Qi ?")
            want = eng.generate([ids], SamplingParams(max_new_tokens=8))[0]
            assert r.status_code == 200 and r.json()["response"] == tok.decode(want)
    finally:
        s.close()
