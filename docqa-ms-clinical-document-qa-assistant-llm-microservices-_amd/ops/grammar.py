"""The JSON-object automaton of ``format: "json"``: ONE definition for the host and the device.

A byte-level pushdown automaton for llama.cpp's ``json.gbnf`` with the root restricted to an
object.  Its lexer is a table ``lexer state x byte -> (next lexer state, op)`` built here once
(:func:`table`); ``ops.reference`` and ``csrc/kernels/grammar.hip`` both walk THAT table, and
only the eight ops below are written twice.  A different grammar later is a different table.

Rules: whitespace (space, tab, LF, CR) between tokens, a run of more than ``WS_CAP`` of them
is rejected; nesting deeper than ``DEPTH_CAP`` is rejected (one stack bit per level: 0 object,
1 array); strings take any byte >= 0x20 but ``"`` and ``\\``, the escapes ``\\" \\\\ \\/ \\b \\f \\n
\\r \\t \\uXXXX`` and strictly valid UTF-8 (lead bytes C2..F4, the restricted second byte behind
E0 / ED / F0 / F4) whose position inside a sequence is part of the state, since byte-level
tokens end mid-sequence; numbers are ``-?(0|[1-9][0-9]*)(\\.[0-9]+)?([eE][+-]?[0-9]+)?`` and end
at the delimiter that follows them (whitespace ``, } ]``), which is processed as that
delimiter in the same step; ``true false null``; after the root object closes the state is
DONE and no byte is accepted.

The per-row state is one int64, 0 meaning "row not constrained":

    bits  0..7   lexer state (1..N_STATES-1)
    bits  8..12  whitespace run so far (0..WS_CAP)
    bits 13..18  depth (0..DEPTH_CAP)
    bits 19..50  stack, bit 19 + level: 1 array, 0 object (bits at and above depth are 0)
"""
from __future__ import annotations

import functools

import numpy as np
import torch

WS_CAP = 16
DEPTH_CAP = 32

# ops of a table entry (entry = next | op << 8)
OP_NONE, OP_WS, OP_PUSH_OBJ, OP_PUSH_ARR, OP_POP_OBJ, OP_POP_ARR, OP_COMMA, OP_REJECT = range(8)

# lexer states the op semantics name have fixed ids (the kernel's constants); the rest follow
DONE, AFTER_VALUE, EXPECT_KEY, EXPECT_VALUE = 1, 2, 3, 4
START, OBJ_OPEN, AFTER_KEY, ARR_OPEN = 5, 6, 7, 8
_NAMES = ["-", "DONE", "AFTER_VALUE", "EXPECT_KEY", "EXPECT_VALUE", "START", "OBJ_OPEN", "AFTER_KEY", "ARR_OPEN",
          "T1", "T2", "T3", "F1", "F2", "F3", "F4", "N1", "N2", "N3",
          "NUM_MINUS", "NUM_ZERO", "NUM_INT", "FRAC0", "FRAC", "EXP0", "EXP_SIGN", "EXP"]
_STR = ["STR", "ESC", "U0", "U1", "U2", "U3", "TAIL1", "TAIL2", "TAIL3", "E0_2", "ED_2", "F0_2", "F4_2"]
_NAMES += ["K_" + s for s in _STR] + ["V_" + s for s in _STR]
STATE_NAMES = tuple(_NAMES)
N_STATES = len(STATE_NAMES)
MAX_STATES = 64          # the kernels' LDS copy of the table holds this many rows
S = {n: i for i, n in enumerate(STATE_NAMES)}

_LEX_BITS, _WS_SHIFT, _DEPTH_SHIFT, _STACK_SHIFT = 8, 8, 13, 19
START_STATE = START      # lexer START, no whitespace, depth 0
WS_BYTES = b" \t\n\r"


def pack(lex: int, ws: int = 0, depth: int = 0, stack: int = 0) -> int:
    return lex | ws << _WS_SHIFT | depth << _DEPTH_SHIFT | stack << _STACK_SHIFT


def unpack(state: int) -> tuple[int, int, int, int]:
    """(lexer state, whitespace run, depth, stack bits) of a state word."""
    return state & 0xFF, state >> _WS_SHIFT & 0x1F, state >> _DEPTH_SHIFT & 0x3F, state >> _STACK_SHIFT & 0xFFFFFFFF


def is_done(state: int) -> bool:
    return state & 0xFF == DONE


@functools.lru_cache(maxsize=1)
def _table_np() -> np.ndarray:
    t = np.full((N_STATES, 256), OP_REJECT << 8, dtype=np.int16)

    def put(state: str, bs, nxt, op: int = OP_NONE) -> None:
        nxt = S[nxt] if isinstance(nxt, str) else nxt
        for b in (bs if isinstance(bs, (bytes, range, list)) else [bs]):
            t[S[state], b] = nxt | op << 8

    def ws(state: str, back: str | None = None) -> None:
        put(state, WS_BYTES, back or state, OP_WS)

    def value_start(state: str) -> None:
        put(state, b'"', "V_STR")
        put(state, b"{", "OBJ_OPEN", OP_PUSH_OBJ)
        put(state, b"[", "ARR_OPEN", OP_PUSH_ARR)
        put(state, b"-", "NUM_MINUS")
        put(state, b"0", "NUM_ZERO")
        put(state, b"123456789", "NUM_INT")
        put(state, b"t", "T1")
        put(state, b"f", "F1")
        put(state, b"n", "N1")

    def delimiters(state: str) -> None:
        """A value has ended (or ends here, a number): whitespace , } ]"""
        ws(state, "AFTER_VALUE")
        put(state, b",", 0, OP_COMMA)
        put(state, b"}", 0, OP_POP_OBJ)
        put(state, b"]", 0, OP_POP_ARR)

    put("START", b"{", "OBJ_OPEN", OP_PUSH_OBJ)
    ws("OBJ_OPEN"); put("OBJ_OPEN", b'"', "K_STR"); put("OBJ_OPEN", b"}", 0, OP_POP_OBJ)
    ws("EXPECT_KEY"); put("EXPECT_KEY", b'"', "K_STR")
    ws("AFTER_KEY"); put("AFTER_KEY", b":", "EXPECT_VALUE")
    ws("EXPECT_VALUE"); value_start("EXPECT_VALUE")
    ws("ARR_OPEN"); value_start("ARR_OPEN"); put("ARR_OPEN", b"]", 0, OP_POP_ARR)
    delimiters("AFTER_VALUE")
    for word in (b"true", b"false", b"null"):
        p = chr(word[0]).upper()
        for i, b in enumerate(word[1:], 1):
            put(f"{p}{i}", b, f"{p}{i + 1}" if i + 1 < len(word) else "AFTER_VALUE")
    digits = b"0123456789"
    put("NUM_MINUS", b"0", "NUM_ZERO"); put("NUM_MINUS", b"123456789", "NUM_INT")
    put("NUM_INT", digits, "NUM_INT")
    for s in ("NUM_ZERO", "NUM_INT"):
        put(s, b".", "FRAC0"); put(s, b"eE", "EXP0"); delimiters(s)
    put("FRAC0", digits, "FRAC")
    put("FRAC", digits, "FRAC"); put("FRAC", b"eE", "EXP0"); delimiters("FRAC")
    put("EXP0", b"+-", "EXP_SIGN"); put("EXP0", digits, "EXP")
    put("EXP_SIGN", digits, "EXP")
    put("EXP", digits, "EXP"); delimiters("EXP")
    for k, closed in (("K_", "AFTER_KEY"), ("V_", "AFTER_VALUE")):
        body = k + "STR"
        put(body, range(0x20, 0x80), body)
        put(body, b'"', closed)
        put(body, b"\\", k + "ESC")
        put(k + "ESC", b'"\\/bfnrt', body); put(k + "ESC", b"u", k + "U0")
        hexd = b"0123456789abcdefABCDEF"
        for i in range(4):
            put(f"{k}U{i}", hexd, f"{k}U{i + 1}" if i < 3 else body)
        # the standard UTF-8 automaton
        put(body, range(0xC2, 0xE0), k + "TAIL1")
        put(body, 0xE0, k + "E0_2"); put(body, list(range(0xE1, 0xED)) + [0xEE, 0xEF], k + "TAIL2")
        put(body, 0xED, k + "ED_2")
        put(body, 0xF0, k + "F0_2"); put(body, range(0xF1, 0xF4), k + "TAIL3"); put(body, 0xF4, k + "F4_2")
        put(k + "TAIL1", range(0x80, 0xC0), body)
        put(k + "TAIL2", range(0x80, 0xC0), k + "TAIL1")
        put(k + "TAIL3", range(0x80, 0xC0), k + "TAIL2")
        put(k + "E0_2", range(0xA0, 0xC0), k + "TAIL1")
        put(k + "ED_2", range(0x80, 0xA0), k + "TAIL1")
        put(k + "F0_2", range(0x90, 0xC0), k + "TAIL2")
        put(k + "F4_2", range(0x80, 0x90), k + "TAIL2")
    t.setflags(write=False)
    return t


def table() -> torch.Tensor:
    """The lexer table, int16 [N_STATES, 256] (row 0 and DONE reject every byte): entry
    ``next | op << 8``.  A fresh CPU tensor; callers keep their device copy."""
    return torch.from_numpy(_table_np().copy())


@functools.lru_cache(maxsize=1)
def _table_list() -> list:
    return _table_np().astype(np.int32).tolist()


def step(state: int, byte: int, tab: list | None = None) -> int:
    """The state after one byte, or -1: rejected.  The op semantics, host side."""
    tab = tab or _table_list()
    lex, ws, depth, stack = unpack(state)
    if lex >= len(tab):
        return -1
    e = tab[lex][byte]
    nxt, op = e & 0xFF, e >> 8
    if op == OP_REJECT:
        return -1
    if op == OP_WS:
        if ws >= WS_CAP:
            return -1
        return pack(nxt, ws + 1, depth, stack)
    if op == OP_PUSH_OBJ or op == OP_PUSH_ARR:
        if depth >= DEPTH_CAP:
            return -1
        return pack(nxt, 0, depth + 1, stack | (op == OP_PUSH_ARR) << depth)
    if op == OP_POP_OBJ or op == OP_POP_ARR:
        if depth == 0 or (stack >> (depth - 1) & 1) != (op == OP_POP_ARR):
            return -1
        depth -= 1
        return pack(DONE if depth == 0 else AFTER_VALUE, 0, depth, stack & ~(1 << depth))
    if op == OP_COMMA:
        if depth == 0:
            return -1
        return pack(EXPECT_VALUE if stack >> (depth - 1) & 1 else EXPECT_KEY, 0, depth, stack)
    return pack(nxt, 0, depth, stack)


def walk(state: int, data: bytes) -> int:
    """The state after ``data``, or -1 as soon as a byte is rejected."""
    tab = _table_list()
    lex, ws, depth, stack = unpack(state)
    if lex >= len(tab):
        return -1
    for b in data:          # :func:`step` with the state kept unpacked
        e = tab[lex][b]
        op = e >> 8
        if op == OP_NONE:
            lex, ws = e, 0
        elif op == OP_REJECT:
            return -1
        elif op == OP_WS:
            if ws >= WS_CAP:
                return -1
            lex, ws = e & 0xFF, ws + 1
        else:
            s = step(pack(lex, ws, depth, stack), b, tab)
            if s < 0:
                return -1
            lex, ws, depth, stack = unpack(s)
    return pack(lex, ws, depth, stack)


def accepts(data: bytes) -> bool:
    """``data`` is a complete document: the walk from the start state ends in DONE."""
    s = walk(START_STATE, data)
    return s >= 0 and is_done(s)


def advance_token(state: int, tok: int, token_bytes: list, eos_id: int) -> int:
    """``ops.grammar_advance`` of one row, host side: 0 and DONE stay, EOS leaves the state as it
    is, and a token that would be rejected (or has no bytes) leaves it unchanged."""
    if state == 0 or is_done(state) or tok == eos_id or not 0 <= tok < len(token_bytes) or not token_bytes[tok]:
        return state
    s = walk(state, token_bytes[tok])
    return state if s < 0 else s


def replay(tokens: list, token_bytes: list, eos_id: int, state: int = START_STATE) -> int:
    """The state of a constrained request that has emitted ``tokens``."""
    for t in tokens:
        state = advance_token(state, t, token_bytes, eos_id)
    return state


def token_allowed(state: int, tok: int, token_bytes: list, eos_id: int) -> bool:
    """``ops.grammar_mask``'s rule for one (constrained) state and token, host side."""
    if tok == eos_id:
        return is_done(state)
    return 0 <= tok < len(token_bytes) and bool(token_bytes[tok]) and walk(state, token_bytes[tok]) >= 0


def vocab_tensors(token_bytes: list) -> tuple[torch.Tensor, torch.Tensor]:
    """``(offsets int32 [V + 1], bytes uint8 [total])`` of a vocabulary's token bytes.  Every one
    of the 256 single-byte strings must be a token: with them and no dead state in the automaton,
    every state but DONE allows some token, so the mask kernel never has to ask whether anything
    is left."""
    have = {b for b in token_bytes if len(b) == 1}
    missing = [i for i in range(256) if bytes([i]) not in have]
    if missing:
        raise ValueError(f"vocabulary lacks single-byte tokens for {len(missing)} bytes "
                         f"(first: 0x{missing[0]:02x}): a constrained row could be left with no token")
    lens = np.fromiter((len(b) for b in token_bytes), dtype=np.int64, count=len(token_bytes))
    if int(lens.sum()) >= 1 << 31:
        raise ValueError("vocabulary bytes exceed int32 offsets")
    off = np.zeros(len(token_bytes) + 1, dtype=np.int32)
    np.cumsum(lens, out=off[1:])
    data = np.frombuffer(b"".join(token_bytes), dtype=np.uint8).copy()
    return torch.from_numpy(off), torch.from_numpy(data)
