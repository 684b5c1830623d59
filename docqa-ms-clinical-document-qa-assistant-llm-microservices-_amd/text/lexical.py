"""Text analysis of the lexical (BM25) search: text -> ``(term, tf)`` pairs.

Deterministic and vocabulary-free, so the indexer, a follower in another process and a
query analysed years later agree on every term without a shared file:

* NFKD, combining marks dropped, casefold (``Éphédra`` == ``ephedra`` == ``EPHEDRA``);
* tokens are the maximal runs of ``str.isalnum()`` characters;
* dropped: tokens longer than ``MAX_TOKEN_CHARS``, one-character tokens that are not
  digits, and the French / English stop words below (articles, prepositions, auxiliaries);
* no stemming;
* ``term`` = FNV-1a 32-bit of the token's UTF-8 bytes, ``0xFFFFFFFF`` remapped to
  ``0xFFFFFFFE``: ``PAD_TERM`` (0xFFFFFFFF) pads query rows and is never a real term;
* ``tf`` = occurrences in the text, stored capped at ``TF_CAP``; the document length is the
  uncapped number of kept tokens.

The hash values are the on-device format (index/lexical.py, csrc/kernels/lexical.hip):
tests/test_lexical_cpu.py pins some.
"""
from __future__ import annotations

import unicodedata

PAD_TERM = 0xFFFFFFFF
MAX_TOKEN_CHARS = 64
TF_CAP = 255

STOP_WORDS = frozenset("""
au aux avec ce ces cet cette dans de des du elle elles en et eux il ils je la le les leur leurs lui ma mais me
mes moi mon ne nos notre nous on ou par pas pour qu que qui sa se ses son sur ta te tes toi ton tu un une vos
votre vous est sont ete etre etait etaient sera seront soit suis es sommes etes ai as avons avez ont avait
avaient aura auront avoir eu eue eus ayant etant chez vers sans sous entre depuis pendant comme donc car ni si
the an and or of to in on at by for from with as is are was were be been being am has have had having do does
did this that these those it its he she they them his her their we you your our not but if then than so into
over under about between during which who whom what when where will would can could shall should may might
""".split())


def fnv1a32(data: bytes) -> int:
    h = 0x811C9DC5
    for b in data:
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h


def term_of(token: str) -> int:
    h = fnv1a32(token.encode("utf-8"))
    return 0xFFFFFFFE if h == PAD_TERM else h


def tokens(text: str) -> list[str]:
    """The kept tokens of ``text`` in order (their count is the document length)."""
    norm = unicodedata.normalize("NFKD", text or "")
    norm = "".join(c for c in norm if not unicodedata.combining(c)).casefold()
    out, cur = [], []
    for c in norm + " ":
        if c.isalnum():
            cur.append(c)
            continue
        if cur:
            t = "".join(cur)
            cur = []
            if len(t) > MAX_TOKEN_CHARS or (len(t) == 1 and not t.isdigit()) or t in STOP_WORDS:
                continue
            out.append(t)
    return out


def analyze_full(text: str) -> tuple[list[tuple[int, int]], int]:
    """(``(term, tf)`` pairs ascending by term with tf capped at ``TF_CAP``, document length)."""
    toks = tokens(text)
    cnt: dict[int, int] = {}
    for t in toks:
        h = term_of(t)
        cnt[h] = cnt.get(h, 0) + 1
    return [(h, min(c, TF_CAP)) for h, c in sorted(cnt.items())], len(toks)


def analyze(text: str) -> list[tuple[int, int]]:
    return analyze_full(text)[0]
