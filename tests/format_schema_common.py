"""Shared fixtures of the JSON-schema format tests: the schemas (pydantic models and hand-written
ones), their oracles, a seeded instance generator, vocabularies and the coverage states."""
from __future__ import annotations

import collections
import enum
import functools
import json
import random
from typing import Literal, Optional

from pydantic import BaseModel, ConfigDict, ValidationError

from docqa_amd.ops import json_schema as J
from tests.format_json_common import STYLES, engine_vocab, synthetic_vocab

# the schema of the service test (ISSUE: verdict / score / ok)
SERVICE_SCHEMA = {"type": "object", "properties": {"verdict": {"enum": ["oui", "non"]}, "score": {"type": "integer"},
                                                    "ok": {"type": "boolean"}},
                  "required": ["verdict", "score", "ok"]}
SMALL_SCHEMA = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"type": "null"}}, "required": ["ok"]}


# ------------------------------------------------------------------ pydantic models: the oracle
class _Strict(BaseModel):
    model_config = ConfigDict(strict=True, extra="forbid")


class Level(str, enum.Enum):
    low = "bas"
    mid = "moyen"
    high = "haut"


class Source(_Strict):
    doc: str
    page: int
    score: float | None = None


class Answer(_Strict):
    verdict: Literal["oui", "non"]
    kind: Literal["qa"]
    level: Level
    sources: list[Source]
    note: Optional[str]
    ok: bool
    ratio: float
    tags: list[str] = []        # the deepest level the 4-space style keeps under the whitespace cap


class Patient(_Strict):
    nom: str
    age: int
    actif: bool
    poids: float


class Extraction(_Strict):
    patient: Patient
    diagnostics: list[Literal["a", "b", "c d"]]
    code: Literal[1, 2, 30]
    mixed: int | str
    suivi: None = None


def _pydantic_oracle(model):
    def ok(doc: bytes) -> bool:
        try:
            model.model_validate_json(doc)
            return True
        except ValidationError:
            return False
    return ok


# ------------------------------------------------------------------ hand-written schemas and validator
H_OPTIONAL = {"type": "object", "properties": {"a": {"type": "integer"}, "b": {"type": "string"},
                                                "c": {"type": "boolean"}, "d": {"type": "null"}}, "required": ["b"]}
H_ARRAYS = {"type": "object", "required": ["xs", "ys", "zs"], "additionalProperties": False, "properties": {
    "xs": {"type": "array", "items": {"type": "integer"}, "minItems": 2, "maxItems": 4},
    "ys": {"type": "array", "items": {"type": ["string", "null"]}, "maxItems": 2},
    "zs": {"type": "array", "items": {"enum": [1, "x", None, True, 2.5]}, "minItems": 1}}}
H_TYPES = {"type": "object", "required": ["v"], "properties": {
    "v": {"type": ["integer", "string", "null", "boolean"]},
    "w": {"type": ["number", "array"], "items": {"type": "number"}},
    "o": {"oneOf": [{"type": "object", "properties": {"k": {"const": "x"}}, "required": ["k"]}, {"type": "string"}]}}}


def _is_type(v, t: str) -> bool:
    if t == "null":
        return v is None
    if t == "boolean":
        return isinstance(v, bool)
    if t == "integer":
        return isinstance(v, int) and not isinstance(v, bool)
    if t == "number":
        return isinstance(v, (int, float)) and not isinstance(v, bool)
    if t == "string":
        return isinstance(v, str)
    if t == "array":
        return isinstance(v, list)
    return isinstance(v, dict)


def _same(a, b) -> bool:
    return type(a) is type(b) and a == b


def hand_validate(s: dict, v) -> bool:
    """The hand-written validator of the hand-written schemas (the keywords they use)."""
    for comb in ("oneOf", "anyOf"):
        if comb in s:
            return any(hand_validate(sub, v) for sub in s[comb])
    if "enum" in s:
        return any(_same(x, v) for x in s["enum"])
    if "const" in s:
        return _same(s["const"], v)
    types = [s["type"]] if isinstance(s["type"], str) else s["type"]
    if not any(_is_type(v, t) for t in types):
        return False
    if isinstance(v, dict):
        props = s["properties"]
        return set(s.get("required", [])) <= set(v) <= set(props) and all(hand_validate(props[k], x)
                                                                          for k, x in v.items())
    if isinstance(v, list):
        return s.get("minItems", 0) <= len(v) <= s.get("maxItems", 1 << 30) and all(hand_validate(s["items"], x)
                                                                                    for x in v)
    return True


def _hand_oracle(schema):
    def ok(doc: bytes) -> bool:
        # json.loads keeps the last of duplicate keys: a duplicate would hide a member, so count them
        pairs_ok = [True]

        def hook(pairs):
            if len({k for k, _ in pairs}) != len(pairs):
                pairs_ok[0] = False
            return dict(pairs)
        try:
            v = json.loads(doc.decode("utf-8"), object_pairs_hook=hook)
        except (ValueError, UnicodeDecodeError):
            return False
        return pairs_ok[0] and isinstance(v, dict) and hand_validate(schema, v)
    return ok


@functools.lru_cache(maxsize=1)
def cases() -> dict:
    """name -> (schema, oracle)."""
    out = {m.__name__: (m.model_json_schema(), _pydantic_oracle(m)) for m in (Answer, Extraction)}
    for name, s in (("optional", H_OPTIONAL), ("arrays", H_ARRAYS), ("types", H_TYPES), ("service", SERVICE_SCHEMA)):
        out[name] = (s, _hand_oracle(s))
    return out


# ------------------------------------------------------------------ instances
_BMP = ['"', "\\", "\n", "\t", "\x01", "\x7f", "é", "߿", "中", "￮", "a", "Z", "0", " ", "/", "{", "]", ":", ","]
_ASTRAL = ["\U0001f600", "\U0010ffff"]


def _rand_string(rng: random.Random, raw: bool) -> str:
    pool = _BMP + (_ASTRAL if raw else [])      # no \\uD83D\\uDE00 pairs for a mutation to break apart
    return "".join(rng.choice(pool) for _ in range(rng.randint(0, 8)))


def gen_value(s: dict, root: dict, rng: random.Random, raw: bool):
    """A seeded instance of schema ``s`` (properties in declared order, numbers inside the caps)."""
    while "$ref" in s:
        s = root[s["$ref"].split("/")[1]][s["$ref"].split("/")[2]]
    for comb in ("anyOf", "oneOf"):
        if comb in s:
            return gen_value(rng.choice(s[comb]), root, rng, raw)
    if "enum" in s:
        return rng.choice(s["enum"])
    if "const" in s:
        return s["const"]
    t = rng.choice([s["type"]] if isinstance(s["type"], str) else s["type"])
    if t == "object":
        req = s.get("required", [])
        return {k: gen_value(sub, root, rng, raw) for k, sub in s["properties"].items()
                if k in req or rng.random() < 0.5}
    if t == "array":
        lo = s.get("minItems", 0)
        return [gen_value(s["items"], root, rng, raw) for _ in range(rng.randint(lo, min(s.get("maxItems", lo + 3), lo + 3)))]
    if t == "string":
        return _rand_string(rng, raw)
    if t == "integer":
        return rng.choice([0, -1, 7, rng.randint(-10 ** 15, 10 ** 15), 10 ** 16 - 1, -(10 ** 16 - 1)])
    if t == "number":
        return rng.choice([0.5, -1.25, 1e-7, 2.5e+20, -3.0e-12, 1.0, 123456.789, 3, -12,
                           round(rng.uniform(-1, 1), 6), 1e+100, -2.5e-300])
    if t == "boolean":
        return rng.random() < 0.5
    return None


def gen_documents(schema: dict, n: int, seed: int = 0) -> list[bytes]:
    """``n`` json.dumps documents of ``schema`` cycling through the four styles of format_json_common."""
    rng = random.Random(seed)
    docs = []
    for i in range(n):
        style = STYLES[i % 4]
        obj = gen_value(schema, schema, rng, raw=style.get("ensure_ascii") is False)
        docs.append(json.dumps(obj, **style).encode("utf-8"))
    return docs


# ------------------------------------------------------------------ automaton helpers
def witnesses(cs) -> dict:
    """DFA state -> a shortest byte string that reaches it from START (BFS over the table)."""
    first_byte = {}
    for b in range(255, -1, -1):
        first_byte[int(cs.cls[b])] = b
    seen = {J.START: b""}
    queue = collections.deque([J.START])
    while queue:
        st = queue.popleft()
        for c in range(cs.n_classes):
            e = int(cs.trans[st, c])
            if e and (e & J.NEXT_MASK) not in seen:
                seen[e & J.NEXT_MASK] = seen[st] + bytes([first_byte[c]])
                queue.append(e & J.NEXT_MASK)
    return seen


def coverage_words(cs, slot: int = 0) -> list[int]:
    """Every DFA state (each reachable: witnessed) at whitespace runs 0 and WS_CAP, in ``slot``."""
    w = witnesses(cs)
    assert set(w) == set(range(1, cs.n_states)), "a state has no witness"
    for st, data in w.items():
        got = J.walk(cs, J.start_state(), data)
        assert got >= 0 and J.unpack(got)[0] == st
    return [J.pack(st, ws, slot) for st in range(1, cs.n_states) for ws in (0, J.WS_CAP)]


@functools.lru_cache(maxsize=1)
def big_schema() -> dict:
    """Near the size cap: 80 properties of three types each, half of them required."""
    return {"type": "object", "properties": {f"k{i}": {"type": ["number", "string", "null"]} for i in range(80)},
            "required": [f"k{i}" for i in range(0, 80, 2)]}


def schema_strings(schema: dict) -> list[bytes]:
    """Keys and enum / const strings of a schema as tokens: bare, quoted and with what follows."""
    out = []

    def visit(s):
        if isinstance(s, dict):
            for k, v in s.items():
                if k == "properties" and isinstance(v, dict):
                    for name, sub in v.items():
                        q = J._dumps(name)
                        out.extend([name.encode(), q, q + b":", b'{' + q, b',' + q + b': ', q[:-2]])
                        visit(sub)
                elif k in ("enum", "const"):
                    for x in (v if k == "enum" else [v]):
                        q = J._dumps(x)
                        out.extend([q, q + b",", q + b"}", q[1:], b":" + q])
                else:
                    visit(v)
        elif isinstance(s, list):
            for v in s:
                visit(v)
    visit(schema)
    return [t for t in dict.fromkeys(out) if t]


@functools.lru_cache(maxsize=4)
def schema_vocab(tiles: int = 1) -> tuple:
    """The synthetic vocabulary of format_json_common plus the schemas' keys and enum strings,
    ``tiles`` times over (EOS stays id 2: the copies of ids 0..2 are empty tokens), padded with
    empty tokens to a size that is 8 mod 64."""
    extra = []
    for schema, _ in cases().values():
        extra += schema_strings(schema)
    base = list(synthetic_vocab())
    toks = (base + [t for t in dict.fromkeys(extra) if t not in set(base)]) * tiles
    while len(toks) % 64 != 8:
        toks.append(b"")
    return tuple(toks)


def schema_engine_vocab(n: int) -> list:
    """format_json_common.engine_vocab with tokens of the service schema in empty ids."""
    toks = engine_vocab(n)
    more = [b'"verdict"', b'"oui"', b'"non"', b'"score"', b'"ok"', b'{"verdict":', b'"ok":', b'-1', b'12', b'e}',
            b'true}', b'"n"', b'null}', b',"n":']
    at = max(i for i, t in enumerate(toks) if t) + 1
    toks[at:at + len(more)] = more
    return toks
