"""Ollama-compatible generation API on the llm-qa service.

The reference's llm-qa does not generate itself: ``ChatOllama(model="mistral",
temperature=0)`` (llm-qa/main.py:66-69) posts every prompt to an external Ollama server
at ``OLLAMA_BASE_URL`` (``/api/chat``, llm-qa/main.py:117; SURVEY §2.4 message-site
table).  Serving the same wire API from this service's engine makes it a drop-in for that
external dependency: a LangChain ``ChatOllama`` / ``ollama`` client pointed at this
service's URL gets its completions from the MI355X engine (continuous batching with every
other request in flight) instead of a llama.cpp process.

  POST /api/chat      {"model", "messages": [{"role", "content"}], "stream" (default true),
                       "options": {"temperature", "num_predict", "top_k", "top_p", "min_p",
                                   "seed", "repeat_penalty", "repeat_last_n", "presence_penalty",
                                   "frequency_penalty", "stop"},
                       "logprobs" (default false), "top_logprobs" (0..20),
                       "format": "json" | a JSON-schema object (absent / null / "": off)}
                      -> {"model", "created_at", "message": {"role": "assistant", "content"},
                          "done": true, "done_reason": "stop" | "length", "total_duration",
                          "load_duration", "prompt_eval_count", "prompt_eval_duration",
                          "eval_count", "eval_duration"}
                      stream: application/x-ndjson, one line per text piece
                      ({"message": {..., "content": piece}, "done": false}) then the final
                      line above with an empty content
                      logprobs: the response gains "logprobs", one {"token", "logprob", "bytes",
                      "top_logprobs": [{"token", "logprob", "bytes"} x top_logprobs]} per generated
                      token -- the log-probability of the model's own distribution (the LM head's
                      logits before penalties, temperature, top-k and top-p; engine/llm_engine.py).
                      Streamed, each line carries the entries of the tokens whose text it releases
                      (a token held back for an incomplete UTF-8 sequence or a possible stop string
                      travels with the line that releases it, or with the final line); over all
                      lines they are the non-streamed list.  Tokens a stop string cuts off are
                      dropped from it like their text: a token wholly behind the cut goes, a token
                      whose text straddles it (part of it is in the response) keeps its entry.  "top_logprobs" outside 0..20, or above 0
                      without "logprobs", is a 400 {"error"}.
  POST /api/generate  {"model", "prompt", "system", "raw", "stream", "options"} -> the same
                      with "response" instead of "message"
  GET  /api/tags      the one model this process serves; GET /api/version

Deviations, by design: one model per process (the request's "model" is echoed, not used to
pick weights); "temperature" defaults to the service's TEMPERATURE (0, the reference's
setting) rather than Ollama's 0.8, and the penalties to the service's neutral REPEAT_PENALTY /
REPEAT_LAST_N / PRESENCE_PENALTY / FREQUENCY_PENALTY rather than Ollama's 1.1 over 64 tokens
(docs/CONFIG.md); "keep_alive", "images" and "tools" are ignored.  "format": "json" constrains
the completion to ONE JSON object on the device (ops/grammar.py, csrc/kernels/grammar.hip: every
step masks the tokens that would leave llama.cpp's json.gbnf with an object root, EOS is allowed
only once the object has closed), so whenever done_reason is "stop" by EOS the text parses with
json.loads; "length" means num_predict cut the object short, as with Ollama.  Two caps keep a
model from looping: a run of more than 16 whitespace characters outside strings and nesting deeper
than 32 are not generated.  A JSON-schema OBJECT as "format" (what ChatOllama's
with_structured_output and format=Model.model_json_schema() send) is compiled to a byte-level
automaton of its own (ops/json_schema.py, csrc/kernels/grammar_schema.hip) and ENFORCED the same
way: whenever done_reason is "stop" by EOS the text parses and validates against the schema;
"length" means num_predict cut it short.  Supported: type (object array string integer number
boolean null, or a list), properties / required (additionalProperties absent or false), items /
minItems / maxItems, enum / const of scalars, $ref into #/$defs or #/definitions, anyOf / oneOf,
allOf with one member, and the annotations title description default examples $schema $id
$comment deprecated readOnly writeOnly.  Anything else -- free-form sub-values (an object without
properties, additionalProperties true or a schema), recursive $ref, minLength / maxLength /
pattern / format, minimum / maximum / multipleOf -- is a 400 {"error"} that names the keyword by
its JSON pointer, as is a schema too large for a table slot.  Deviations: the root must be an
object; properties are generated in DECLARED order (required ones always, the others may be
skipped) and no other key; oneOf is a union (exclusivity is not enforced); integers have at most
16 digits, fractions 16 and exponents 3, so a row cannot emit digits for ever; whitespace runs
<= 16 as above.  At most DOCQA_SCHEMA_SLOTS (8) distinct schemas decode at once: a request whose
schema finds every table slot in use waits in the queue.  Any other "format" is a 400 {"error"}.
"logprobs" stay the model's own distribution, from the logits before the grammar mask.  "stop" (a string
or a list) ends the text just before the earliest match with done_reason "stop"; a streamed
tail that could still grow into a stop string is held back until it is resolved.
Temperature comes FIRST: top_k, top_p and min_p filter the distribution at the request's
temperature (x = logit / temperature), where llama.cpp's default sampler chain applies the
temperature after those filters.  top_k does not notice; a top_p or min_p cutoff at
temperature != 1 keeps a different set than llama.cpp would.  "min_p" (0..1, default 0: off)
keeps the tokens with p >= min_p * p_max; a value outside [0, 1] is a 400 {"error"}.
"seed": on the continuous scheduler a sampled request (temperature > 0) with a non-zero seed
returns the same completion for the same prompt, options and seed, whatever else is in flight,
at any TP degree: each token is drawn from a counter-based stream keyed by (seed, position)
(ops.seeded_uniform).  Seed 0 or none: a fresh random seed per request.  The static batcher
(DOCQA_SERVING=static) reproduces per batch only.
Durations are nanoseconds like Ollama's.  Streaming is token by token on the continuous
scheduler (DOCQA_SERVING=continuous, the default); the static batcher returns the whole
completion as one piece.
"""
from __future__ import annotations

import asyncio
import json
import time
from datetime import datetime, timezone

from fastapi import FastAPI
from fastapi.responses import JSONResponse, StreamingResponse
from pydantic import BaseModel

from ..engine.llm_engine import SamplingParams

_DONE = object()


class OllamaMessage(BaseModel):
    role: str = "user"
    content: str = ""


class OllamaChatRequest(BaseModel):
    model: str = ""
    messages: list[OllamaMessage] = []
    stream: bool = True
    options: dict | None = None
    logprobs: bool = False
    top_logprobs: int = 0
    format: object = None


class OllamaGenerateRequest(BaseModel):
    model: str = ""
    prompt: str = ""
    system: str | None = None
    raw: bool = False
    stream: bool = True
    options: dict | None = None
    logprobs: bool = False
    top_logprobs: int = 0
    format: object = None


def schema_from_request(fmt) -> dict | None:
    """The request's ``format`` as ``SamplingParams.json_schema``: a JSON-schema object is passed
    through (``SamplingParams.set_json_schema`` compiles it and raises ValueError with the
    keyword that is not supported), anything else is no schema."""
    return fmt if isinstance(fmt, dict) else None


def format_from_request(fmt) -> str:
    """The request's ``format`` as ``SamplingParams.format``: absent / null / "" is off, "json"
    and a JSON-schema object (:func:`schema_from_request`) constrain the output.  Raises
    ValueError (the routes answer 400) on anything else."""
    if fmt is None or fmt == "":
        return ""
    if fmt == "json" or isinstance(fmt, dict):
        return "json"
    raise ValueError('format must be "json" or a JSON schema object')


def _now() -> str:
    return datetime.now(timezone.utc).isoformat().replace("+00:00", "Z")


def sampling_from_options(options: dict | None, settings, max_context: int, prompt_len: int) -> SamplingParams:
    """Ollama ``options`` -> SamplingParams: num_predict (-1 / -2: up to the context) caps
    the new tokens, temperature 0 is greedy; the penalties default to the service settings.
    Raises ValueError (the routes answer 400) on a ``min_p`` outside [0, 1]."""
    o = options or {}
    n = int(o.get("num_predict", settings.max_new_tokens))
    room = max(1, max_context - prompt_len)
    n = room if n < 0 else max(1, min(n, room))
    min_p = float(o.get("min_p", 0.0) or 0.0)
    if not 0.0 <= min_p <= 1.0:      # also refuses NaN
        raise ValueError("min_p must be between 0 and 1")
    return SamplingParams(max_new_tokens=n, temperature=float(o.get("temperature", settings.temperature)),
                          top_k=int(o.get("top_k", 0) or 0), top_p=float(o.get("top_p", 1.0) or 1.0),
                          min_p=min_p, stop_on_eos=True, seed=int(o.get("seed", 0) or 0),
                          repeat_penalty=float(_opt(o, "repeat_penalty", settings.repeat_penalty)),
                          repeat_last_n=int(_opt(o, "repeat_last_n", settings.repeat_last_n)),
                          presence_penalty=float(_opt(o, "presence_penalty", settings.presence_penalty)),
                          frequency_penalty=float(_opt(o, "frequency_penalty", settings.frequency_penalty)))


def _opt(o: dict, name: str, default):
    v = o.get(name)
    return default if v is None else v


def stop_strings(options: dict | None) -> list[str]:
    """``options.stop``: a string or a list of strings (empty ones dropped)."""
    s = (options or {}).get("stop")
    if isinstance(s, str):
        s = [s]
    return [x for x in (s or []) if isinstance(x, str) and x]


def find_stop(text: str, stops: list[str]) -> int:
    """Index of the earliest occurrence of any stop string in ``text``, -1 if none."""
    hits = [i for i in (text.find(s) for s in stops) if i >= 0]
    return min(hits) if hits else -1


def held_back(text: str, stops: list[str]) -> int:
    """Length of the longest tail of ``text`` that is a proper prefix of a stop string: it
    may still grow into one, so a stream does not send it yet."""
    best = 0
    for s in stops:
        for k in range(min(len(s) - 1, len(text)), best, -1):
            if text.endswith(s[:k]):
                best = k
                break
    return best


TOP_LOGPROBS_MAX = 20   # Ollama's limit, and ops.TOP_LOGPROBS_MAX


def logprobs_error(logprobs: bool, top_logprobs: int) -> str | None:
    """Why the request's logprob fields are refused (HTTP 400), or None."""
    if not 0 <= top_logprobs <= TOP_LOGPROBS_MAX:
        return f"top_logprobs must be between 0 and {TOP_LOGPROBS_MAX}"
    if top_logprobs > 0 and not logprobs:
        return "top_logprobs requires logprobs to be true"
    return None


def logprob_entries(tok, ids: list[int], lps: list) -> list[dict]:
    """Ollama's per-token objects from token ids and the engine's (logprob, [(id, logprob), ...])
    of each: ``token`` is the tokenizer's decoding of that single id, ``bytes`` its UTF-8 bytes."""
    def one(i: int, lp: float) -> dict:
        t = tok.decode([i])
        return {"token": t, "logprob": max(float(lp), -3.4028234663852886e38), "bytes": list(t.encode("utf-8"))}

    return [{**one(i, lp), "top_logprobs": [one(j, v) for j, v in top]} for i, (lp, top) in zip(ids, lps)]


def visible_tokens(tok, ids: list[int], start: int, length: int) -> int:
    """The smallest n >= ``start`` whose tokens ids[:n] decode to at least ``length`` characters
    (a trailing incomplete UTF-8 sequence not counted): the tokens a text of that length shows,
    wholly or in part -- a token that straddles a stop string's cut keeps its entry, since part of
    its text is in the response.  len(ids) when even all of them do not.  Trailing U+FFFD are taken
    for an incomplete sequence, as the streaming loop takes them: a model that really emits U+FFFD
    as the last character of a prefix has that token counted one piece late (with the next
    character or the final line), never dropped.  Each call decodes a few growing prefixes, which
    is fine at num_predict sizes."""
    n = start
    while n < len(ids) and len(tok.decode(ids[:n]).rstrip("\ufffd")) < length:
        n += 1
    return n


def register(app: FastAPI, settings, metrics) -> None:
    """Add the Ollama routes to the llm-qa app (``app.state.pipeline`` / ``app.state.batcher``)."""

    def _prompt_ids(pipe, ids: list[int]) -> list[int]:
        lim = pipe.max_prompt_tokens
        return ids if not lim or len(ids) <= lim else ids[: lim // 2] + ids[-(lim // 2):]

    async def _run(kind: str, model: str, ids: list[int], options: dict | None, stream: bool,
                   logprobs: bool = False, top_logprobs: int = 0, fmt=None):
        pipe, batcher = app.state.pipeline, app.state.batcher
        if pipe is None or batcher is None:
            return JSONResponse(status_code=503, content={"error": "model not loaded"})
        bad = logprobs_error(logprobs, top_logprobs)
        if bad:
            return JSONResponse(status_code=400, content={"error": bad})
        tok = pipe.chat_tok
        ids = _prompt_ids(pipe, ids)
        try:
            params = sampling_from_options(options, settings, pipe.engine.max_context, len(ids))
            params.format = format_from_request(fmt)
            params.set_json_schema(schema_from_request(fmt))
            if params.constrained:
                if getattr(getattr(batcher, "engine", None), "mixed", False):
                    raise ValueError('format "json" is not served with mixed steps (DOCQA_MIXED_PREFILL=1)')
                pipe.engine.require_grammar(params)
        except ValueError as e:
            return JSONResponse(status_code=400, content={"error": str(e)})
        params.logprobs, params.top_logprobs = bool(logprobs), int(top_logprobs)
        metrics.inc(f"ollama_{kind}_requests")
        loop = asyncio.get_running_loop()
        q: asyncio.Queue = asyncio.Queue()
        t0 = time.perf_counter()
        first = [0.0]

        def on_token(_rid, t, lp=None):     # the scheduler adds the token's logprobs when asked
            if not first[0]:
                first[0] = time.perf_counter()
            loop.call_soon_threadsafe(q.put_nowait, (t, lp))

        stops = stop_strings(options)
        # the scheduler retires the request at the token that completes a stop string (the
        # static batcher has no per-token hook: it runs to num_predict, the text is cut below)
        stop_check = (lambda out: find_stop(tok.decode(out), stops) >= 0) if stops else None
        fut = batcher.submit("gen", {"ids": ids, "params": params, "on_token": on_token if stream else None,
                                     "stop_check": stop_check})
        fut.add_done_callback(lambda f: loop.call_soon_threadsafe(q.put_nowait, _DONE))

        def body(text: str) -> dict:
            if kind == "chat":
                return {"message": {"role": "assistant", "content": text}}
            return {"response": text}

        def cut(text: str) -> tuple[str, bool]:
            i = find_stop(text, stops) if stops else -1
            return (text[:i], True) if i >= 0 else (text, False)

        def final(out: list[int], text: str, stopped: bool = False) -> dict:
            t1 = time.perf_counter()
            tf = first[0] or t1
            eos = bool(out) and out[-1] == pipe.engine.model.cfg.eos_token_id
            d = {"model": model or settings.llm_model, "created_at": _now(), **body(text), "done": True,
                 "done_reason": "stop" if eos or stopped else "length", "total_duration": int((t1 - t0) * 1e9),
                 "load_duration": 0, "prompt_eval_count": len(ids), "prompt_eval_duration": int((tf - t0) * 1e9),
                 "eval_count": len(out), "eval_duration": int((t1 - tf) * 1e9)}
            if kind == "generate":
                d["context"] = []
            return d

        def entries(out: list[int], lps: list, lo: int, hi: int) -> list[dict]:
            return logprob_entries(tok, out[lo:hi], lps[lo:hi])

        if not stream:
            res = await asyncio.wrap_future(fut)
            text, stopped = cut(tok.decode(res["ids"]))
            d = final(res["ids"], text, stopped)
            if logprobs:
                # a stop string's cut drops the tokens whose text it drops
                n = visible_tokens(tok, res["ids"], 0, len(text)) if stopped else len(res["ids"])
                d["logprobs"] = entries(res["ids"], res["logprobs"], 0, n)
            return JSONResponse(d)

        async def lines():
            got: list[int] = []
            glp: list = []   # logprobs: each token's (logprob, top list), parallel to ``got``
            sent = ""
            shown = 0        # tokens whose logprob entries have gone out
            while True:
                item = await q.get()
                if item is _DONE:
                    break
                got.append(item[0])
                glp.append(item[1])
                text = tok.decode(got)
                if text.endswith("\ufffd"):     # an incomplete UTF-8 sequence: wait for its bytes
                    continue
                if stops:
                    text, stopped = cut(text)
                    if not stopped:
                        text = text[:len(text) - held_back(text, stops)]
                    if len(text) < len(sent) or not text.startswith(sent):
                        continue
                piece, sent = text[len(sent):], text
                if piece:
                    d = {"model": model or settings.llm_model, "created_at": _now(), **body(piece), "done": False}
                    if logprobs:
                        # the entries of the tokens this piece makes visible
                        n = visible_tokens(tok, got, shown, len(sent))
                        d["logprobs"], shown = entries(got, glp, shown, n), n
                    yield json.dumps(d) + "\n"
            try:
                res = fut.result()
                out = res["ids"]
            except Exception as e:  # noqa: BLE001 - the stream is already open: report in-band
                yield json.dumps({"error": f"{type(e).__name__}: {e}"}) + "\n"
                return
            text, stopped = cut(tok.decode(out))
            rest = text[len(sent):] if text.startswith(sent) else text
            if rest:     # the static batcher (no per-token callback) or a held-back tail
                d = {"model": model or settings.llm_model, "created_at": _now(), **body(rest), "done": False}
                if logprobs:
                    n = visible_tokens(tok, out, shown, len(text))
                    d["logprobs"], shown = entries(out, res["logprobs"], shown, n), n
                yield json.dumps(d) + "\n"
            d = final(out, "", stopped)
            if logprobs:
                n = visible_tokens(tok, out, shown, len(text)) if stopped else len(out)
                d["logprobs"] = entries(out, res["logprobs"], shown, n)
            yield json.dumps(d) + "\n"

        return StreamingResponse(lines(), media_type="application/x-ndjson")

    @app.post("/api/chat")
    async def ollama_chat(req: OllamaChatRequest):
        pipe = app.state.pipeline
        if pipe is None:
            return JSONResponse(status_code=503, content={"error": "model not loaded"})
        ids = pipe.chat_tok.chat_messages([m.model_dump() for m in req.messages])
        return await _run("chat", req.model, ids, req.options, req.stream, req.logprobs, req.top_logprobs,
                          req.format)

    @app.post("/api/generate")
    async def ollama_generate(req: OllamaGenerateRequest):
        pipe = app.state.pipeline
        if pipe is None:
            return JSONResponse(status_code=503, content={"error": "model not loaded"})
        tok = pipe.chat_tok
        if req.raw:
            ids = tok.encode(req.prompt)
        else:
            ids = tok.chat_prompt(req.prompt, system=req.system)
        return await _run("generate", req.model, ids, req.options, req.stream, req.logprobs, req.top_logprobs,
                          req.format)

    @app.get("/api/tags")
    def ollama_tags():
        pipe = app.state.pipeline
        models = []
        if pipe is not None:
            m = pipe.engine.model
            models.append({"name": settings.llm_model, "model": settings.llm_model, "modified_at": _now(),
                           "size": int(m.weight_bytes()), "digest": "",
                           "details": {"format": "safetensors", "family": "llama", "families": ["llama"],
                                       "parameter_size": f"{m.cfg.num_params() / 1e9:.1f}B",
                                       "quantization_level": {"fp8-e4m3": "F8_E4M3", "mxfp4": "MXFP4"}.get(
                                           getattr(m, "weight_format", "bf16"), "BF16"),
                                       # the paged KV format (DOCQA_KV_CACHE); not an Ollama field
                                       "kv_cache_type": ("fp8_e4m3" if getattr(pipe.engine, "kv_fp8", False)
                                                         else "bf16")}})
        return {"models": models}

    @app.get("/api/version")
    def ollama_version():
        return {"version": "0.0.0-docqa-mi355x"}
