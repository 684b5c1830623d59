from pathlib import Path

# the reference's shipped index files (data its indexer wrote), stored with the suite
GOLDEN = Path(__file__).resolve().parent / "golden"
REFERENCE_FAISS = GOLDEN / "vector_store.faiss"
REFERENCE_META = GOLDEN / "metadata_store.pkl"
# sizes and SHA-256 digests of the reference's prompt templates (UTF-8)
REFERENCE_PROMPTS = GOLDEN / "reference_prompts.json"
