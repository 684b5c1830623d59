"""Wire contracts (pydantic) of every service -- the API-compatibility surface.

Reference sources: llm-qa/main.py:108-122 (Query / ask response),
synthese-comparative/models/requests.py:6-21 and models/responses.py:6-38,
synthese-comparative/core/llm_client.py:42-54 (summarize contract),
synthese-comparative/core/retrieval_client.py:72-91 (patient-snippets contract),
doc-ingestor/models.py:5-12 (document row), AMQP messages.
"""
from __future__ import annotations

from typing import List, Literal, Optional

from pydantic import BaseModel, Field

# retrieval mode of a question: the dense kNN hits, the BM25 hits or their reciprocal rank
# fusion; None = the service default (RETRIEVAL_MODE).  Any other value is a 422.
SearchMode = Optional[Literal["dense", "lexical", "hybrid"]]
# LangChain's retriever arguments (the reference's retriever is vector_store.as_retriever):
# search_type "mmr" re-selects the k hits for diversity out of the first fetch_k (clamped to
# k..64) with lambda_mult in [0, 1]; None = the service defaults (RETRIEVAL_SEARCH_TYPE,
# MMR_LAMBDA, MMR_FETCH_K).  Anything else is a 422.
SearchType = Optional[Literal["similarity", "mmr"]]


# ---------------------------------------------------------------- llm-qa
class Query(BaseModel):
    question: str
    # optional retrieval scope: one patient's chunks (inside the window, if any) plus the
    # knowledge base unless excluded; a request without them is served as before
    patient_id: Optional[str] = None
    from_date: Optional[str] = None
    to_date: Optional[str] = None
    include_knowledge_base: bool = True
    search_mode: SearchMode = None
    search_type: SearchType = None
    lambda_mult: Optional[float] = Field(default=None, ge=0.0, le=1.0)
    fetch_k: Optional[int] = Field(default=None, ge=1)


AskRequest = Query      # the reference's name for the /ask/ body is Query


class AskResponse(BaseModel):
    answer: str
    sources: List[Optional[str]]


class SummarizeRequest(BaseModel):
    prompt: str


class SummarizeResponse(BaseModel):
    summary: str


# ---------------------------------------------------------------- semantic-indexer
class Snippet(BaseModel):
    doc_id: str
    text: str


class SearchHit(BaseModel):
    id: int
    score: float
    text: str
    source: Optional[str] = None
    type: Optional[str] = None
    doc_id: Optional[str] = None


class SearchRequest(BaseModel):
    query: str
    k: int = 3
    patient_id: Optional[str] = None
    from_date: Optional[str] = None
    to_date: Optional[str] = None
    include_knowledge_base: bool = True
    search_mode: SearchMode = None
    search_type: SearchType = None
    lambda_mult: Optional[float] = Field(default=None, ge=0.0, le=1.0)
    fetch_k: Optional[int] = Field(default=None, ge=1)


# ---------------------------------------------------------------- synthese-comparative
class PatientSummaryRequest(BaseModel):
    patient_id: str
    from_date: Optional[str] = None
    to_date: Optional[str] = None
    focus: Optional[str] = None
    language: str = "fr"


class PatientComparisonRequest(BaseModel):
    patient_ids: List[str]
    from_date: Optional[str] = None
    to_date: Optional[str] = None
    focus: Optional[str] = None
    language: str = "fr"


class SourceSnippet(BaseModel):
    doc_id: str
    snippet: str


class Section(BaseModel):
    title: str
    content: str


class SinglePatientSummaryResponse(BaseModel):
    type: str = "single_patient_summary"
    patient_alias: str
    time_range: Optional[dict]
    sections: List[Section]
    key_points: List[str]
    sources: List[SourceSnippet]


class ComparisonRow(BaseModel):
    dimension: str
    patient_1: str
    patient_2: str


class MultiPatientComparisonResponse(BaseModel):
    type: str = "multi_patient_comparison"
    patients: List[str]
    time_range: Optional[dict]
    summary: str
    comparison_table: List[ComparisonRow]
    key_risks: List[str]
    sources: List[SourceSnippet]


# ---------------------------------------------------------------- doc-ingestor
class DocumentOut(BaseModel):
    id: int
    filename: Optional[str]
    upload_date: Optional[str]
    status: Optional[str]
    doc_type: Optional[str]


# ---------------------------------------------------------------- queue messages
class RawDocumentMessage(BaseModel):
    doc_id: int
    text: str
    metadata: dict = Field(default_factory=dict)


class CleanDocumentMessage(BaseModel):
    doc_id: object
    original_text_masked: str
    metadata: dict = Field(default_factory=dict)
    processed_at: float
