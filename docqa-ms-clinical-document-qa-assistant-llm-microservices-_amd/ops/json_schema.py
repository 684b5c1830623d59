"""JSON-schema structured outputs (the Ollama API's ``format``: a schema object): the schema
compiler and the host automaton.  ONE definition for the host and the device, as ops/grammar.py is
for ``format: "json"``.

The supported schemas (below) are non-recursive, have no free-form sub-values and only objects
with declared properties, so the JSON they describe is a REGULAR language: a schema compiles to a
byte-level DFA with no stack.  :func:`compile_schema` builds an NFA from the schema, determinises
it (subset construction), trims it (every state left can still reach DONE: no dead state) and
compresses the bytes into classes.  The result is two arrays that ``ops.reference`` and
``csrc/kernels/grammar_schema.hip`` both walk:

    cls    uint8  [256]                  byte -> class
    trans  uint16 [n_states, n_classes]  entry = next state (bits 0..14) | WS_FLAG (bit 15)

Entry 0 rejects.  State 0 is the reject row, state ``DONE`` (1) rejects every byte and is reached
by the root object's ``}``, the start state is ``START`` (2).  A flagged entry is a whitespace
byte between tokens (space, tab, LF, CR): it counts against ``ops.grammar.WS_CAP``, the only
counter; every other byte resets the run.

Supported subset -- anything else raises ValueError with the JSON pointer of the keyword:
  * ignored annotations: title description default examples $schema $id $comment deprecated
    readOnly writeOnly ($defs / definitions are only looked into through $ref);
  * ``type``: object array string integer number boolean null, or a list of them;
  * ``$ref`` to ``#/$defs/*`` / ``#/definitions/*`` (recursion is an error); ``anyOf`` and
    ``oneOf`` are both a union (oneOf's exclusivity is NOT enforced); ``allOf`` with one member;
  * the root must resolve to an object;
  * object: ``properties`` in DECLARED order, ``required`` ones mandatory, the others may be
    skipped; ``additionalProperties`` absent or false -- no other key is ever generated; keys are
    the minimal JSON string literal (raw UTF-8);
  * array: ``items`` (one schema), ``minItems`` / ``maxItems`` expanded into states;
  * string: ops.grammar's string language (escapes, strictly valid UTF-8, mid-sequence positions
    are states);
  * integer ``-?(0|[1-9][0-9]{0,15})``; number: that plus ``(\\.[0-9]{1,16})?([eE][+-]?[0-9]{1,3})?``
    -- the digit runs are bounded so that a row cannot emit digits for ever;
  * ``enum`` / ``const`` of scalars, each exactly ``json.dumps(v, ensure_ascii=False,
    separators=(",", ":"))``;
  * whitespace where json.gbnf has it: after ``{ [ , :``, before ``} ]``, after a key and after a
    value; not before the root ``{`` nor after its ``}``.
Left out on purpose: free-form sub-values (objects without properties, additionalProperties true
or a schema -- they need the pushdown stack), recursive schemas, minLength / maxLength / pattern /
format, minimum / maximum / multipleOf.

The per-row state is one int64, 0 meaning "row has no schema":

    bits  0..15  DFA state (1..n_states-1; DONE = 1)
    bits 16..20  whitespace run so far (0..WS_CAP)
    bits 21..28  device table slot (0..255)

The device pool (:func:`pool_new`) is uint8 [n_slots, SLOT_BYTES]; a slot is, at fixed offsets,

    0    int32 n_states, int32 n_classes, 8 bytes of zeros
    16   cls   uint8 [256]
    272  trans uint16 [n_states * n_classes]   (room for MAX_CELLS entries)

and a slot whose header is all zero holds no table (its rows allow nothing).
"""
from __future__ import annotations

import collections
import json
import math
import threading

import numpy as np
import torch

from .grammar import WS_BYTES, WS_CAP

DONE, START = 1, 2
WS_FLAG = 0x8000
NEXT_MASK = 0x7FFF
# what a pool slot holds: the caps of the compiler
MAX_STATES = 8192
MAX_CLASSES = 256
MAX_CELLS = 1 << 18
MAX_SLOTS = 256
_HDR, _CLS_OFF, TRANS_OFF = 16, 16, 272
SLOT_BYTES = TRANS_OFF + 2 * MAX_CELLS
_STATE_BITS, _WS_SHIFT, _SLOT_SHIFT = 16, 16, 21

ANNOTATIONS = frozenset(("title", "description", "default", "examples", "$schema", "$id", "$comment", "deprecated",
                         "readOnly", "writeOnly"))
_DEFS = frozenset(("$defs", "definitions"))
_TYPES = ("object", "array", "string", "integer", "number", "boolean", "null")
INT_DIGITS, FRAC_DIGITS, EXP_DIGITS = 16, 16, 3


# ------------------------------------------------------------------ the state word
def pack(state: int, ws: int = 0, slot: int = 0) -> int:
    return state | ws << _WS_SHIFT | slot << _SLOT_SHIFT


def unpack(word: int) -> tuple[int, int, int]:
    """(DFA state, whitespace run, slot) of a state word."""
    return word & 0xFFFF, word >> _WS_SHIFT & 0x1F, word >> _SLOT_SHIFT & 0xFF


def is_done(word: int) -> bool:
    return word & 0xFFFF == DONE


def start_state(slot: int = 0) -> int:
    return pack(START, 0, slot)


# ------------------------------------------------------------------ NFA
def _mask(bs) -> int:
    m = 0
    for b in bs:
        m |= 1 << b
    return m


_WS_MASK = _mask(WS_BYTES)
_DIGITS, _DIGITS19 = _mask(b"0123456789"), _mask(b"123456789")


class _NFA:
    def __init__(self):
        self.eps: list[list[int]] = []
        self.edges: list[list[tuple[int, int, bool]]] = []     # (byte mask, target, whitespace)

    def node(self) -> int:
        self.eps.append([])
        self.edges.append([])
        return len(self.eps) - 1

    def e(self, a: int, b: int) -> None:
        self.eps[a].append(b)

    def edge(self, a: int, bs, b: int | None = None, ws: bool = False) -> int:
        b = self.node() if b is None else b
        self.edges[a].append((bs if isinstance(bs, int) else _mask(bs), b, ws))
        return b

    def lit(self, a: int, data: bytes) -> int:
        for c in data:
            a = self.edge(a, 1 << c)
        return a

    def ws(self, a: int) -> int:
        """``a`` followed by any run of whitespace."""
        b = self.node()
        self.e(a, b)
        self.edge(b, _WS_MASK, b, True)
        return b

    # ---- values
    def string(self, a: int) -> int:
        """ops.grammar's V_STR states, the quotes included."""
        body = self.edge(a, b'"')
        end = self.edge(body, b'"')
        self.edge(body, _mask(range(0x20, 0x80)) & ~_mask(b'"\\'), body)
        esc = self.edge(body, b"\\")
        self.edge(esc, b'"\\/bfnrt', body)
        u = self.edge(esc, b"u")
        for i in range(4):
            u = self.edge(u, b"0123456789abcdefABCDEF", body if i == 3 else None)
        t1, t2, t3 = self.node(), self.node(), self.node()
        cont = range(0x80, 0xC0)
        self.edge(t1, cont, body)
        self.edge(t2, cont, t1)
        self.edge(t3, cont, t2)
        self.edge(body, range(0xC2, 0xE0), t1)
        self.edge(body, list(range(0xE1, 0xED)) + [0xEE, 0xEF], t2)
        self.edge(body, range(0xF1, 0xF4), t3)
        self.edge(self.edge(body, [0xE0]), range(0xA0, 0xC0), t1)
        self.edge(self.edge(body, [0xED]), range(0x80, 0xA0), t1)
        self.edge(self.edge(body, [0xF0]), range(0x90, 0xC0), t2)
        self.edge(self.edge(body, [0xF4]), range(0x80, 0x90), t2)
        return end

    def _digits(self, a: int, lo: int, hi: int) -> int:
        """Between ``lo`` and ``hi`` digits."""
        end = self.node()
        for i in range(hi):
            if i >= lo:
                self.e(a, end)
            a = self.edge(a, _DIGITS)
        self.e(a, end)
        return end

    def integer(self, a: int) -> int:
        m = self.node()
        self.e(a, m)
        self.edge(a, b"-", m)
        end = self.edge(m, b"0")
        self.e(self._digits(self.edge(m, _DIGITS19), 0, INT_DIGITS - 1), end)
        return end

    def number(self, a: int) -> int:
        i = self.integer(a)
        f = self.node()
        self.e(i, f)
        self.e(self._digits(self.edge(i, b"."), 1, FRAC_DIGITS), f)
        end = self.node()
        self.e(f, end)
        x = self.edge(f, b"eE")
        s = self.node()
        self.e(x, s)
        self.edge(x, b"+-", s)
        self.e(self._digits(s, 1, EXP_DIGITS), end)
        return end


def _dumps(v) -> bytes:
    return json.dumps(v, ensure_ascii=False, separators=(",", ":")).encode("utf-8")


def _type_of(v) -> tuple:
    if v is None:
        return ("null",)
    if isinstance(v, bool):
        return ("boolean",)
    if isinstance(v, int):
        return ("integer", "number")
    if isinstance(v, float):
        return ("number", "integer") if v == int(v) else ("number",)
    return ("string",)


class _Builder:
    def __init__(self, root: dict):
        self.root = root
        self.nfa = _NFA()
        self.active: list[str] = []

    def fail(self, ptr: str, why: str):
        raise ValueError(f"unsupported JSON schema at {ptr if ptr.startswith('#') else '#' + ptr}: {why}")

    def resolve(self, s, ptr: str, enter: bool = True):
        """Follow ``$ref`` and one-member ``allOf``.  -> (schema, pointer, refs entered)."""
        entered = 0
        while True:
            if not isinstance(s, dict):
                self.fail(ptr, "a schema must be an object")
            if "$ref" in s:
                ref = s["$ref"]
                for k in s:
                    if k != "$ref" and k not in ANNOTATIONS and k not in _DEFS:
                        self.fail(f"{ptr}/{k}", "keyword beside $ref")
                parts = ref.split("/") if isinstance(ref, str) else []
                if len(parts) != 3 or parts[0] != "#" or parts[1] not in _DEFS or \
                        not isinstance(self.root.get(parts[1]), dict) or parts[2] not in self.root[parts[1]]:
                    self.fail(f"{ptr}/$ref", f"only #/$defs/NAME and #/definitions/NAME that exist, got {ref!r}")
                if ref in self.active:
                    self.fail(f"{ptr}/$ref", f"recursive $ref {ref!r}")
                self.active.append(ref)
                entered += 1
                s, ptr = self.root[parts[1]][parts[2]], ref
                continue
            if "allOf" in s:
                for k in s:
                    if k != "allOf" and k not in ANNOTATIONS and k not in _DEFS:
                        self.fail(f"{ptr}/{k}", "keyword beside allOf")
                if not isinstance(s["allOf"], list) or len(s["allOf"]) != 1:
                    self.fail(f"{ptr}/allOf", "allOf with exactly one member only")
                s, ptr = s["allOf"][0], f"{ptr}/allOf/0"
                continue
            return s, ptr, entered

    def leave(self, n: int) -> None:
        if n:
            del self.active[-n:]

    def value(self, s, ptr: str, a: int) -> int:
        """The fragment of one value of schema ``s`` from node ``a``; returns its end node."""
        s, ptr, entered = self.resolve(s, ptr)
        try:
            return self._value(s, ptr, a)
        finally:
            self.leave(entered)

    def _value(self, s: dict, ptr: str, a: int) -> int:
        nfa = self.nfa
        for comb in ("anyOf", "oneOf"):
            if comb in s:
                for k in s:
                    if k != comb and k not in ANNOTATIONS and k not in _DEFS:
                        self.fail(f"{ptr}/{k}", f"keyword beside {comb}")
                if not isinstance(s[comb], list) or not s[comb]:
                    self.fail(f"{ptr}/{comb}", "a non-empty list of schemas")
                end = nfa.node()
                for i, sub in enumerate(s[comb]):
                    b = nfa.node()
                    nfa.e(a, b)
                    nfa.e(self.value(sub, f"{ptr}/{comb}/{i}", b), end)
                return end
        types = s.get("type")
        if types is not None:
            types = [types] if isinstance(types, str) else types
            if not isinstance(types, list) or not types or any(t not in _TYPES for t in types):
                self.fail(f"{ptr}/type", f"type must be one or a list of {', '.join(_TYPES)}")
        if "enum" in s or "const" in s:
            for k in s:
                if k not in ("enum", "const", "type") and k not in ANNOTATIONS and k not in _DEFS:
                    self.fail(f"{ptr}/{k}", "keyword beside enum / const")
            kw = "const" if "const" in s else "enum"
            if "const" in s and "enum" in s:
                self.fail(f"{ptr}/enum", "enum beside const")
            vals = [s["const"]] if kw == "const" else s["enum"]
            if not isinstance(vals, list) or not vals:
                self.fail(f"{ptr}/{kw}", "a non-empty list of scalars")
            for v in vals:
                if not (v is None or isinstance(v, (bool, int, str)) or (isinstance(v, float) and math.isfinite(v))):
                    self.fail(f"{ptr}/{kw}", "values must be strings, finite numbers, booleans or null")
            if types is not None:
                vals = [v for v in vals if any(t in types for t in _type_of(v))]
                if not vals:
                    self.fail(f"{ptr}/{kw}", "no value has the schema's type")
            end = nfa.node()
            for lit in sorted({_dumps(v) for v in vals}):
                nfa.e(nfa.lit(a, lit), end)
            return end
        if types is None:
            if "properties" in s:
                types = ["object"]
            elif "items" in s:
                types = ["array"]
            else:
                for k in s:
                    if k not in ANNOTATIONS and k not in _DEFS:
                        self.fail(f"{ptr}/{k}", "keyword not supported")
                self.fail(ptr, "a schema without type, enum, const, $ref or anyOf is a free-form value")
        allowed = set(ANNOTATIONS) | _DEFS | {"type"}
        if "object" in types:
            allowed |= {"properties", "required", "additionalProperties"}
        if "array" in types:
            allowed |= {"items", "minItems", "maxItems"}
        for k in s:
            if k not in allowed:
                self.fail(f"{ptr}/{k}", "keyword not supported" + (" for this type" if k in (
                    "properties", "required", "additionalProperties", "items", "minItems", "maxItems") else ""))
        end = nfa.node()
        for t in dict.fromkeys(types):
            b = nfa.node()
            nfa.e(a, b)
            if t == "object":
                b = self.object(s, ptr, b)
            elif t == "array":
                b = self.array(s, ptr, b)
            elif t == "string":
                b = nfa.string(b)
            elif t == "integer":
                b = nfa.integer(b)
            elif t == "number":
                b = nfa.number(b)
            elif t == "boolean":
                c = nfa.node()
                nfa.e(nfa.lit(b, b"true"), c)
                nfa.e(nfa.lit(b, b"false"), c)
                b = c
            else:
                b = nfa.lit(b, b"null")
            nfa.e(b, end)
        return end

    def object(self, s: dict, ptr: str, a: int) -> int:
        nfa = self.nfa
        ap = s.get("additionalProperties", False)
        if ap is not False:
            self.fail(f"{ptr}/additionalProperties", "must be absent or false (free-form members need a stack)")
        props = s.get("properties")
        if not isinstance(props, dict):
            self.fail(f"{ptr}/properties" if "properties" in s else ptr,
                      "an object needs declared properties (a free-form object needs a stack)")
        req = s.get("required", [])
        if not isinstance(req, list) or any(not isinstance(k, str) or k not in props for k in req):
            self.fail(f"{ptr}/required", "a list of declared property names")
        # none: no member yet, some: at least one (the next takes a comma); both after whitespace
        none = nfa.ws(nfa.edge(a, b"{"))
        some = None
        for key, sub in props.items():
            if not isinstance(key, str):
                self.fail(f"{ptr}/properties", "property names are strings")
            k = nfa.node()                      # in front of the key's quote
            if none is not None:
                nfa.e(none, k)
            if some is not None:
                nfa.e(nfa.ws(nfa.edge(some, b",")), k)
            v = nfa.ws(nfa.edge(nfa.ws(nfa.lit(k, _dumps(key))), b":"))
            after = nfa.ws(self.value(sub, f"{ptr}/properties/{key.replace('~', '~0').replace('/', '~1')}", v))
            if key in req:
                none, some = None, after
            else:
                if some is not None:
                    nfa.e(some, after)
                some = after
        end = nfa.node()
        for n in (none, some):
            if n is not None:
                nfa.edge(n, b"}", end)
        return end

    def array(self, s: dict, ptr: str, a: int) -> int:
        nfa = self.nfa
        if "items" not in s:
            self.fail(ptr, "an array needs items (free-form items need a stack)")
        lo, hi = s.get("minItems", 0), s.get("maxItems")
        if not isinstance(lo, int) or isinstance(lo, bool) or lo < 0:
            self.fail(f"{ptr}/minItems", "a non-negative integer")
        if hi is not None and (not isinstance(hi, int) or isinstance(hi, bool) or hi < lo):
            self.fail(f"{ptr}/maxItems", "an integer >= minItems")
        iptr = f"{ptr}/items"
        cur = nfa.ws(nfa.edge(a, b"["))        # k items so far, after whitespace
        end = nfa.node()
        k = 0
        while True:
            if k >= lo:
                nfa.edge(cur, b"]", end)
            if hi is not None and k >= hi:
                return end
            if len(nfa.eps) > 64 * MAX_STATES:
                raise ValueError(f"schema too large: the array at {ptr or '#'} expands past the table pool")
            start = cur if k == 0 else nfa.ws(nfa.edge(cur, b","))
            if hi is None and k >= max(lo, 1):
                nfa.e(nfa.ws(self.value(s["items"], iptr, start)), cur)      # the loop
                return end
            cur = nfa.ws(self.value(s["items"], iptr, start))
            k += 1


# ------------------------------------------------------------------ compile
class CompiledSchema:
    """``cls`` uint8 [256], ``trans`` uint16 [n_states, n_classes] (read-only numpy arrays) and
    ``key``, the canonical text of the schema."""

    def __init__(self, cls: np.ndarray, trans: np.ndarray, key: str):
        self.cls, self.trans, self.key = cls, trans, key
        self.n_states, self.n_classes = trans.shape
        self._cls_l = cls.tolist()
        self._trans_l = trans.astype(np.int32).tolist()

    def image(self) -> torch.Tensor:
        """The bytes of a pool slot that holds this table (header, cls, trans): uint8."""
        hdr = np.zeros(4, dtype=np.int32)
        hdr[0], hdr[1] = self.n_states, self.n_classes
        return torch.from_numpy(np.concatenate([hdr.view(np.uint8), self.cls, self.trans.reshape(-1).view(np.uint8)]))

    def max_document_len(self) -> int | None:
        """Bytes of the longest accepted document (whitespace runs at the cap), None: unbounded."""
        def succ(node):
            st, ws = node
            out = set()
            for e in set(self._trans_l[st]):
                if e and not (e & WS_FLAG and ws >= WS_CAP):
                    out.add((e & NEXT_MASK, ws + 1 if e & WS_FLAG else 0))
            return sorted(out)

        best: dict = {}           # node -> longest tail; None while the node is on the path
        stack = [((START, 0), None)]
        while stack:
            node, it = stack.pop()
            if it is None:
                if node in best:
                    continue
                best[node] = None
                it = iter(succ(node))
            for nxt in it:
                if nxt not in best:
                    stack.append((node, it))
                    stack.append((nxt, None))
                    break
                if best[nxt] is None:
                    return None        # a cycle: the language is infinite
            else:
                best[node] = max((1 + best[n] for n in succ(node)), default=0)
        return best[(START, 0)]


def _compile(schema: dict, key: str) -> CompiledSchema:
    if not isinstance(schema, dict):
        raise ValueError("unsupported JSON schema at #: the schema must be an object")
    b = _Builder(schema)
    root, ptr, _ = b.resolve(schema, "")
    rt = root.get("type")
    if any(k in root for k in ("anyOf", "oneOf", "enum", "const")) or not (
            rt == "object" or rt == ["object"] or (rt is None and "properties" in root)):
        raise ValueError(f"unsupported JSON schema at {ptr or '#'}: the root must be an object")
    nfa = b.nfa
    first = nfa.node()
    accept = b._value(root, ptr, first)
    # byte classes of the NFA: bytes no edge tells apart
    masks = sorted({m for es in nfa.edges for m, _, _ in es})
    sig: dict = {}
    byte_cls = []
    for byte in range(256):
        key_b = tuple(m >> byte & 1 for m in masks)
        byte_cls.append(sig.setdefault(key_b, len(sig)))
    n0 = len(sig)
    cls_mask = [0] * n0
    for byte, c in enumerate(byte_cls):
        cls_mask[c] |= 1 << byte
    # per node: (classes, target, ws)
    of_mask = {m: [c for c in range(n0) if cls_mask[c] & m] for m in masks}
    node_edges = [[(of_mask[m], t, w) for m, t, w in es] for es in nfa.edges]
    closure_memo: dict = {}

    def closure(nodes) -> frozenset:
        out, stack = set(nodes), list(nodes)
        while stack:
            n = stack.pop()
            got = closure_memo.get(n)
            if got is not None:
                out |= got
                continue
            for t in nfa.eps[n]:
                if t not in out:
                    out.add(t)
                    stack.append(t)
        return frozenset(out)

    for n in range(len(nfa.eps)):
        closure_memo[n] = closure([n])
    done_set = frozenset([accept])
    ids = {done_set: DONE, closure([first]): START}
    order = [None, done_set, closure([first])]
    rows: list = [[0] * n0, [0] * n0]
    i = START
    while i < len(order):
        tgt: list = [None] * n0
        flag = [None] * n0
        for n in order[i]:
            for cs, t, w in node_edges[n]:
                for c in cs:
                    if tgt[c] is None:
                        tgt[c], flag[c] = {t}, w
                    else:
                        tgt[c].add(t)
                        if flag[c] != w:
                            raise AssertionError("a byte is whitespace and not whitespace in one state")
        row = [0] * n0
        for c in range(n0):
            if tgt[c] is None:
                continue
            d = closure(tgt[c])
            j = ids.get(d)
            if j is None and accept in d:
                # behind the root's `}`: nothing follows
                if any(node_edges[n] for n in d):
                    raise AssertionError("DONE shares a state")
                j = ids[d] = DONE
            if j is None:
                j = ids[d] = len(order)
                order.append(d)
                if j >= MAX_STATES:
                    raise ValueError(f"schema too large: more than {MAX_STATES} automaton states")
            row[c] = j | (WS_FLAG if flag[c] else 0)
        rows.append(row)
        i += 1
    t = np.array(rows, dtype=np.int64)
    # trim: keep the states that DONE is reachable from (all of them are reachable from START)
    nxt = t & NEXT_MASK
    live = np.zeros(len(rows), dtype=bool)
    live[DONE] = True
    while True:
        grow = live | (live[nxt] & (t != 0)).any(axis=1)
        if (grow == live).all():
            break
        live = grow
    if not live[START]:
        raise ValueError("unsupported JSON schema at #: no document satisfies it")
    t = np.where(live[nxt], t, 0)
    keep = np.nonzero(live)[0]
    keep = np.concatenate([[0], keep]) if not live[0] else keep
    renum = np.zeros(len(rows), dtype=np.int64)
    renum[keep] = np.arange(len(keep))
    t = t[keep]
    t = np.where(t != 0, renum[t & NEXT_MASK] | (t & WS_FLAG), 0)
    assert renum[DONE] == DONE and renum[START] == START
    # byte-class compression: classes with the same column are one (class 0: the first byte's)
    col_ids: dict = {}
    remap = [col_ids.setdefault(t[:, c].tobytes(), len(col_ids)) for c in range(n0)]
    cols = [None] * len(col_ids)
    for c, r in enumerate(remap):
        if cols[r] is None:
            cols[r] = t[:, c]
    trans = np.ascontiguousarray(np.stack(cols, axis=1).astype(np.uint16))
    cls = np.array([remap[c] for c in byte_cls], dtype=np.uint8)
    n_states, n_classes = trans.shape
    if n_states > MAX_STATES or n_classes > MAX_CLASSES or n_states * n_classes > MAX_CELLS:
        raise ValueError(f"schema too large: {n_states} states x {n_classes} byte classes "
                         f"(caps: {MAX_STATES} states, {MAX_CLASSES} classes, {MAX_CELLS} entries)")
    cls.setflags(write=False)
    trans.setflags(write=False)
    return CompiledSchema(cls, trans, key)


_CACHE: "collections.OrderedDict[str, CompiledSchema]" = collections.OrderedDict()
_CACHE_MAX = 64
_LOCK = threading.Lock()


def canonical(schema: dict) -> str:
    return json.dumps(schema, sort_keys=True)


def compile_schema(schema: dict, cache: bool = True) -> CompiledSchema:
    """The automaton of ``schema`` (module docstring).  Deterministic; compiled schemas are kept in
    an LRU keyed by the canonical ``json.dumps(schema, sort_keys=True)`` -- with the schema's own
    spelling behind it, since the declared property order is part of the generated language and
    sorting the keys loses it."""
    if not isinstance(schema, dict):
        raise ValueError("unsupported JSON schema at #: the schema must be an object")
    try:
        key = canonical(schema) + "\n" + json.dumps(schema)
    except (TypeError, ValueError) as e:
        raise ValueError(f"unsupported JSON schema at #: not JSON ({e})") from None
    if cache:
        with _LOCK:
            got = _CACHE.get(key)
            if got is not None:
                _CACHE.move_to_end(key)
                return got
    cs = _compile(schema, key)
    if cache:
        with _LOCK:
            _CACHE[key] = cs
            while len(_CACHE) > _CACHE_MAX:
                _CACHE.popitem(last=False)
    return cs


# ------------------------------------------------------------------ the host automaton
def step(cs: CompiledSchema, word: int, byte: int) -> int:
    """The state word after one byte, or -1: rejected."""
    st, ws, slot = unpack(word)
    if st >= cs.n_states:
        return -1
    e = cs._trans_l[st][cs._cls_l[byte]]
    if e == 0:
        return -1
    if e & WS_FLAG:
        if ws >= WS_CAP:
            return -1
        return pack(e & NEXT_MASK, ws + 1, slot)
    return pack(e, 0, slot)


def walk(cs: CompiledSchema, word: int, data: bytes) -> int:
    """The state word after ``data``, or -1 as soon as a byte is rejected."""
    st, ws, slot = unpack(word)
    if st >= cs.n_states:
        return -1
    tr, cl = cs._trans_l, cs._cls_l
    for b in data:
        e = tr[st][cl[b]]
        if e == 0:
            return -1
        if e & WS_FLAG:
            if ws >= WS_CAP:
                return -1
            st, ws = e & NEXT_MASK, ws + 1
        else:
            st, ws = e, 0
    return pack(st, ws, slot)


def accepts(cs: CompiledSchema, data: bytes) -> bool:
    """``data`` is a complete document: the walk from the start state ends in DONE."""
    s = walk(cs, start_state(), data)
    return s >= 0 and is_done(s)


def advance_token(cs: CompiledSchema, word: int, tok: int, token_bytes: list, eos_id: int) -> int:
    """``ops.schema_advance`` of one row, host side: 0 and DONE stay, EOS leaves the word as it
    is, and a token that would be rejected (or has no bytes) leaves it unchanged."""
    if word == 0 or is_done(word) or tok == eos_id or not 0 <= tok < len(token_bytes) or not token_bytes[tok]:
        return word
    s = walk(cs, word, token_bytes[tok])
    return word if s < 0 else s


def replay(cs: CompiledSchema, tokens: list, token_bytes: list, eos_id: int, word: int | None = None) -> int:
    """The state word of a schema-constrained request that has emitted ``tokens``."""
    word = start_state() if word is None else word
    for t in tokens:
        word = advance_token(cs, word, t, token_bytes, eos_id)
    return word


def token_allowed(cs: CompiledSchema, word: int, tok: int, token_bytes: list, eos_id: int) -> bool:
    """``ops.schema_mask``'s rule for one (non-zero) state word and token, host side."""
    if tok == eos_id:
        return is_done(word)
    return 0 <= tok < len(token_bytes) and bool(token_bytes[tok]) and walk(cs, word, token_bytes[tok]) >= 0


# ------------------------------------------------------------------ the pool
def pool_new(n_slots: int, device="cpu") -> torch.Tensor:
    """An empty table pool: uint8 [n_slots, SLOT_BYTES] of zeros."""
    if not 1 <= n_slots <= MAX_SLOTS:
        raise ValueError(f"schema slots must be in [1, {MAX_SLOTS}], got {n_slots}")
    return torch.zeros(n_slots, SLOT_BYTES, dtype=torch.uint8, device=device)


def pool_put(pool: torch.Tensor, slot: int, cs: CompiledSchema) -> None:
    """Write ``cs`` into ``pool[slot]`` (on the pool's device, in stream order)."""
    img = cs.image()
    pool[slot, :img.numel()].copy_(img.to(pool.device, non_blocking=True))


def pool_tables(pool_np: np.ndarray, slot: int):
    """(cls uint8 [256], trans uint16 [n_states, n_classes]) of a slot of a pool held as a numpy
    uint8 array, or None: the slot index or its header is out of range."""
    if not 0 <= slot < pool_np.shape[0]:
        return None
    row = pool_np[slot]
    ns, nc = (int(v) for v in row[:8].view(np.int32))
    if ns < 2 or ns > MAX_STATES or nc < 1 or nc > MAX_CLASSES or ns * nc > MAX_CELLS:
        return None
    return row[_CLS_OFF:_CLS_OFF + 256], row[TRANS_OFF:TRANS_OFF + 2 * ns * nc].view(np.uint16).reshape(ns, nc)
