"""Row attributes and query scopes of the scoped exact search (``ops.knn_scoped``).

Every index row carries two int32 values, held beside the vectors (never inside the FAISS
file -- they are derived from the metadata list, which is persisted and travels in the
write-ahead log):

* ``tag``: 0 for a row that is not a patient-file chunk (the knowledge base), else a
  positive ordinal of the row's ``patient_id``;
* ``day``: the proleptic Gregorian day number of the record's ``note_date`` (ISO string,
  text/dates.py), ``UNDATED`` when it has none.

A query's scope is one int32 row ``(tag, alt_tag, day_lo, day_hi)``; a row matches iff

    row_tag == alt_tag || ((tag < 0 || row_tag == tag) && day_lo <= row_day && row_day <= day_hi)

================  =======================  ===============================================
``tag``           ``-1``                   any tag
``alt_tag``       ``-1``                   no alternative tag (row tags are >= 0)
``alt_tag``       ``0``                    also the knowledge base, exempt from the window
``day_lo/hi``     ``(INT32_MIN, MAX)``     no window: undated rows pass
``day_lo``        ``INT32_MIN + 1``        only an upper bound: undated rows are excluded
``tag``           ``INT32_MAX``            an unknown patient: no row carries this tag
================  =======================  ===============================================

The date rule is ``text.dates.in_window``'s: a window with any bound excludes undated rows.
"""
from __future__ import annotations

import calendar
import datetime

import torch

from ..text.dates import parse_date

INT32_MIN = -(1 << 31)
INT32_MAX = (1 << 31) - 1
UNDATED = INT32_MIN
ANY_SCOPE = (-1, -1, INT32_MIN, INT32_MAX)
UNKNOWN_TAG = INT32_MAX


def day_number(iso: str | None) -> int:
    """Day number of an ISO ``YYYY-MM-DD`` date, ``UNDATED`` for none.  ``parse_date`` lets a
    day past the month's end through (``2021-02-31``); it is clamped to the month's last day,
    which keeps the order of the ISO strings ``in_window`` compares."""
    if not iso:
        return UNDATED
    try:
        y, m, d = int(iso[0:4]), int(iso[5:7]), int(iso[8:10])
        return datetime.date(y, m, min(d, calendar.monthrange(y, m)[1])).toordinal()
    except (ValueError, IndexError):
        return UNDATED


def _bound(s, name: str) -> str | None:
    if s is None or str(s).strip() == "":
        return None
    iso = parse_date(s)
    if iso is None:
        raise ValueError(f"{name}: unparseable date {s!r}")
    return iso


def scope_request(patient_id=None, from_date=None, to_date=None, include_knowledge_base: bool = True):
    """The scope request of a wire message's four optional fields: ``None`` when none of them
    restricts anything (the request then takes the unscoped path), else the dict
    :meth:`ScopeColumns.scope_rows` takes.  Raises ``ValueError`` on an unparseable date and on
    a request that excludes the knowledge base without naming a patient or a window."""
    lo, hi = _bound(from_date, "from_date"), _bound(to_date, "to_date")
    if patient_id is None and lo is None and hi is None:
        if not include_knowledge_base:
            raise ValueError("include_knowledge_base=false needs a patient_id or a date window")
        return None
    return {"patient_id": None if patient_id is None else str(patient_id), "from_date": lo, "to_date": hi,
            "include_knowledge_base": bool(include_knowledge_base)}


class ScopeColumns:
    """Capacity-doubling int32 ``tags`` / ``days`` on the index's device for the first ``n``
    rows of a metadata list, plus the host map patient key -> tag."""

    def __init__(self, device="cuda", capacity: int = 1024):
        self.device = torch.device(device)
        self._tags = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self._days = torch.zeros(capacity, dtype=torch.int32, device=self.device)
        self._tag_of: dict[str, int] = {}
        self.n = 0          # metadata rows covered so far

    # ------------------------------------------------------------------ rows
    @property
    def tags(self) -> torch.Tensor:
        return self._tags[: self.n]

    @property
    def days(self) -> torch.Tensor:
        return self._days[: self.n]

    def tag(self, patient_id) -> int:
        """The tag of a patient key, ``UNKNOWN_TAG`` when no row carries it."""
        return self._tag_of.get(str(patient_id), UNKNOWN_TAG)

    def _row(self, m: dict) -> tuple[int, int]:
        if m.get("type") != "patient_file":
            tag = 0
        else:
            pid = m.get("patient_id")
            key = str(pid if pid is not None else m.get("doc_id"))
            tag = self._tag_of.get(key)
            if tag is None:
                tag = self._tag_of[key] = len(self._tag_of) + 1
        return tag, day_number(parse_date(m.get("note_date")))

    def _sync(self) -> None:
        # searches may run on another stream (the QA prep stream): rows are complete on the
        # device before ``n`` makes them visible
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()

    def extend(self, metadata: list[dict]) -> None:
        """Cover rows ``n..len(metadata)`` (one small host-to-device copy)."""
        start, end = self.n, len(metadata)
        if end <= start:
            return
        host = torch.tensor([self._row(metadata[i]) for i in range(start, end)], dtype=torch.int32).t().contiguous()
        cap = self._tags.shape[0]
        if end > cap:
            new = max(end, cap * 2)
            tags = torch.zeros(new, dtype=torch.int32, device=self.device)
            days = torch.zeros(new, dtype=torch.int32, device=self.device)
            tags[:start] = self._tags[:start]
            days[:start] = self._days[:start]
            self._tags, self._days = tags, days
        dev = host.to(self.device)
        self._tags[start:end] = dev[0]
        self._days[start:end] = dev[1]
        self._sync()
        self.n = end

    def rebuild(self, metadata: list[dict]) -> None:
        self._tag_of, self.n = {}, 0
        self.extend(metadata)

    def remove(self, keep: torch.Tensor, pos: torch.Tensor, n_out: int) -> None:
        self.prepare_remove(keep, pos, n_out)()

    def prepare_remove(self, keep: torch.Tensor, pos: torch.Tensor, n_out: int):
        """Two-step :meth:`remove`: everything that can fail (the check, the device buffers) happens
        here and changes nothing; the returned ``commit()`` only swaps references.

        Drop the rows a delete removes: ``keep`` uint8 [n], ``pos`` its ``ops.masked_scan``,
        ``n_out`` the surviving count (``index.flat.removal_mask``).  New buffers, complete on
        the device before they become visible; ``_tag_of`` stays as it is (a patient whose rows
        are all gone keeps a tag that no row carries)."""
        from .. import ops

        if keep.numel() != self.n:
            raise ValueError(f"scope columns cover {self.n} rows, the mask {keep.numel()}")
        cap = max(1024, n_out)
        tags = torch.zeros(cap, dtype=torch.int32, device=self.device)
        days = torch.zeros(cap, dtype=torch.int32, device=self.device)
        ops.gather_rows(self._tags[: self.n], keep, pos, out=tags)
        ops.gather_rows(self._days[: self.n], keep, pos, out=days)
        self._sync()

        def commit() -> None:
            self._tags, self._days, self.n = tags, days, n_out

        return commit

    # ------------------------------------------------------------------ queries
    def scope_row(self, req) -> tuple[int, int, int, int]:
        if req is None:
            return ANY_SCOPE
        pid = req.get("patient_id")
        lo, hi = _bound(req.get("from_date"), "from_date"), _bound(req.get("to_date"), "to_date")
        kb = bool(req.get("include_knowledge_base", True))
        tag = -1 if pid is None else self.tag(pid)
        if lo is None and hi is None:
            if pid is None and kb:
                return ANY_SCOPE
            if pid is None:
                raise ValueError("include_knowledge_base=false needs a patient_id or a date window")
            day_lo, day_hi = INT32_MIN, INT32_MAX
        else:
            day_lo = day_number(lo) if lo is not None else INT32_MIN + 1
            day_hi = day_number(hi) if hi is not None else INT32_MAX
        return tag, 0 if kb else -1, day_lo, day_hi

    def scope_rows(self, requests: list) -> torch.Tensor:
        """int32 [nq, 4] on the device; ``None`` entries become the any-scope row, so a mixed
        batch is one launch."""
        rows = [self.scope_row(r) for r in requests]
        return torch.tensor(rows, dtype=torch.int32).reshape(len(rows), 4).to(self.device)
