"""Shared fixtures of the format-json tests: sample documents, the seeded document generator,
the synthetic vocabulary, a brute-force per-token walk and the coverage states."""
from __future__ import annotations

import functools
import json
import random

import torch

from docqa_amd.ops import grammar as G

SAMPLE_DOCS = [
    b'{}',
    b'{"a":{"b":[{"c":"x"}]},"d":[[],{}]}',
    b'{\n  "name": "Rate",\n  "qi": [1, -2.5e+3, 0.25, 1E-2, 0],\n  "ok": true, "no": false, "nil": null\n}',
    '{"clé":"café 中文 \U0001f600 ퟿ ","esc":"a\\"b\\\\c\\/d\\b\\f\\n\\r\\t\\u00e9\\uD83D\\uDE00"}'.encode(),
    '{"é中\U0001f600\\u0041":{"k":"v"}}'.encode(),
    b'{"n":[0,-0,10,1.5,2e5,3E+7,4e-2,-1.25e10],"s":"\x7f tab\\t"}',
    b'{ "w" :\t[ 1 ,\r\n 2 ] , "x" : { "y" : [ ] } }',
    (b'{"patient":{"id":12345,"nom":"Dupont","age":67,"diagnostics":["Vide de Qi de la Rate","Humidite"],'
     b'"scores":{"langue":0.75,"pouls":-1.5E-3},"suivi":null,"actif":true,"notes":[]}}'),
    (b'{\n    "answer": "Tonifier le Qi",\n    "sources": [\n        {"doc": "a.pdf", "page": 3},\n'
     b'        {"doc": "b.pdf", "page": 14}\n    ],\n    "confidence": 9.5e-1\n}'),
    # every UTF-8 lead class (C2.., E0, E1.., ED, F0, F1.., F4) and \u, in a key and in a value
    ('{"éࠀ中퟿\U0001f600\U00040000\U0010ffff\\u00e9\\n":'
     '"éࠀ中퟿\U0001f600\U00040000\U0010ffff\\u00e9\\n"}').encode(),
]


# ------------------------------------------------------------------ documents
def _rand_string(rng: random.Random) -> str:
    pool = ['"', "\\", "\n", "\t", "\x01", "\x1f", "\x7f", "é", "߿", "中", "￮", "\U0001f600",
            "\U0010ffff", "a", "Z", "0", " ", "/", "{", "]", ":", ","]
    return "".join(rng.choice(pool) for _ in range(rng.randint(0, 8)))


def _rand_value(rng: random.Random, depth: int):
    r = rng.random() * (1.0 if depth < 4 else 2.5)      # containers thin out towards depth 5
    if depth < 5 and r < 0.22:
        return {_rand_string(rng): _rand_value(rng, depth + 1) for _ in range(rng.randint(0, 3))}
    if depth < 5 and r < 0.40:
        return [_rand_value(rng, depth + 1) for _ in range(rng.randint(0, 3))]
    r = rng.random() * 0.6 + 0.4
    if r < 0.55:
        return _rand_string(rng)
    if r < 0.68:
        return rng.randint(-10 ** 6, 10 ** 6)
    if r < 0.85:
        return rng.choice([0.5, -1.25, 1e-7, 2.5e+20, -3.0e-12, 1.0, 123456.789e3, rng.uniform(-1, 1) * 10 ** rng.randint(-30, 30)])
    return rng.choice([True, False, None])


STYLES = (dict(separators=(",", ":")), dict(indent=2), dict(ensure_ascii=False), dict(indent=4, ensure_ascii=False))


def gen_documents(n: int, seed: int = 0) -> list[bytes]:
    """``n`` json.dumps documents (nested objects, depth <= 5) cycling through the four styles."""
    rng = random.Random(seed)
    docs = []
    for i in range(n):
        obj = {_rand_string(rng): _rand_value(rng, 2) for _ in range(rng.randint(0, 4))}
        docs.append(json.dumps(obj, **STYLES[i % 4]).encode("utf-8"))
    return docs


def max_ws_run(doc: bytes) -> int:
    """The longest run of whitespace bytes OUTSIDE strings (json.dumps escapes none inside)."""
    best = run = 0
    in_str = esc = False
    for b in doc:
        if in_str:
            if esc:
                esc = False
            elif b == 0x5C:
                esc = True
            elif b == 0x22:
                in_str = False
            run = 0
            continue
        if b == 0x22:
            in_str, run = True, 0
        elif b in G.WS_BYTES:
            run += 1
            best = max(best, run)
        else:
            run = 0
    return best


MUTATION_ALPHABET = (b'{}[]:,"\\' + b"0123456789" + b"-+.eEtfnu a" + b"\n\t\r"
                     + bytes([0xC3, 0xA9, 0xE4, 0xB8, 0xAD, 0xF0, 0x9F, 0x98, 0x80])       # valid UTF-8 pieces
                     + bytes([0x80, 0xBF, 0xC0, 0xC1, 0xED, 0xA0, 0xF5, 0xFF, 0xE0, 0xF4])  # invalid / restricted
                     + bytes([0x00, 0x01, 0x1F, 0x7F]))


def mutate(doc: bytes, rng: random.Random) -> bytes:
    b = bytearray(doc)
    for _ in range(rng.choice((1, 1, 1, 2))):
        kind = rng.randrange(3)
        pos = rng.randrange(len(b) + (kind == 1)) if b else 0
        c = rng.choice(MUTATION_ALPHABET)
        if kind == 0 and b:
            b[pos] = c
        elif kind == 1:
            b.insert(pos, c)
        elif b:
            del b[pos]
    return bytes(b)


# ------------------------------------------------------------------ vocabulary
EOS_SYN = 2


@functools.lru_cache(maxsize=1)
def synthetic_vocab() -> tuple:
    """~3000 tokens: ids 0..2 empty (pad, bos, EOS = 2), the 256 single bytes, every substring up
    to 6 bytes of the sample documents, 200 random byte strings, a few more empty tokens, two
    tokens of 48 and 64 bytes; padded with empty tokens to a size that is 8 mod 64."""
    rng = random.Random(11)
    toks = [b"", b"", b""] + [bytes([i]) for i in range(256)]
    seen = set(toks)
    for d in SAMPLE_DOCS:
        for n in range(2, 7):
            for i in range(len(d) - n + 1):
                s = d[i:i + n]
                if s not in seen:
                    seen.add(s)
                    toks.append(s)
    for _ in range(200):
        toks.append(bytes(rng.choice(MUTATION_ALPHABET + b'abc"{}: ') for _ in range(rng.randint(1, 9))))
    toks += [b""] * 5
    toks.append((b'"' + b"abcdefgh" * 6)[:48])
    toks.append((b"x" * 30 + b'","k":[1,2,{"z":null}],"y":"' + b"y" * 20)[:64])
    rng2 = random.Random(5)
    head, tail = toks[:259], toks[259:]
    rng2.shuffle(tail)
    toks = head + tail
    while len(toks) % 64 != 8:
        toks.append(b"")
    return tuple(toks)


def engine_vocab(n: int) -> list:
    """A small vocabulary for whole-engine runs on models of ``n`` ids: ids 0..2 empty (EOS = 2),
    the 256 single bytes, a few multi-structural tokens, the rest empty -- few tokens are allowed
    behind ``{``, so a random model closes the object within a test's token budget."""
    multi = [b'{"', b'":', b'",', b'"}', b'":{"', b'"}]}', b',\n  "', b'": "', b'":[', b'],"', b'true', b'false',
             b'null', b'{}', b'[]', b'}}', b'1,', b'0.5', b'-1e', b'\\u00', b'\xc3\xa9', b'\xe4\xb8', b'\xad"', b'\n}', b' }', b'a":']
    toks = [b"", b"", b""] + [bytes([i]) for i in range(256)] + multi
    return toks + [b""] * (n - len(toks))


def vocab_on(device, toks=None):
    """(tok_off, tok_bytes, table) tensors of a vocabulary on ``device``."""
    off, data = G.vocab_tensors(list(toks if toks is not None else synthetic_vocab()))
    return off.to(device), data.to(device), G.table().to(device)


def brute_allowed(state: int, toks, eos_id: int, n_valid: int) -> list[bool]:
    return [G.token_allowed(state, t, toks, eos_id) for t in range(n_valid)]


# ------------------------------------------------------------------ coverage states
@functools.lru_cache(maxsize=1)
def coverage_states() -> tuple:
    """States that hit every lexer state (the sample documents walked byte by byte), plus the
    whitespace run and the depth at their caps, and DONE."""
    by_lex: dict = {}
    extra = []
    docs = list(SAMPLE_DOCS)
    docs.append(b'{"a":' + b" " * G.WS_CAP + b"1}")
    docs.append(b'{"d":' + b"[" * (G.DEPTH_CAP - 1) + b"]" * (G.DEPTH_CAP - 1) + b"}")
    docs.append(b'{"d":' + b'{"k":' * (G.DEPTH_CAP - 1) + b"1" + b"}" * (G.DEPTH_CAP - 1) + b"}")
    for d in docs:
        s = G.START_STATE
        by_lex.setdefault(G.unpack(s)[0], s)
        for b in d:
            s = G.step(s, b)
            assert s >= 0, d
            lex, ws, depth, _ = G.unpack(s)
            by_lex.setdefault(lex, s)
            if ws == G.WS_CAP or depth == G.DEPTH_CAP:
                extra.append(s)
        assert G.is_done(s)
    assert set(by_lex) == set(range(1, G.N_STATES)), sorted(set(range(1, G.N_STATES)) - set(by_lex))
    out = list(by_lex.values())
    for s in extra:
        if s not in out:
            out.append(s)
    return tuple(out)


def states_tensor(states, device) -> torch.Tensor:
    return torch.tensor(list(states), dtype=torch.int64, device=device)
