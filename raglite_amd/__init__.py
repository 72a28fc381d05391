"""raglite_amd -- MI355X-native retrieval / rerank hot path for RAGLite.

Hand-written HIP (gfx950) kernels behind a C ABI (`include/raglite_hip.h`, `libraglite_hip.so`)
and a Python host layer that mirrors the reference's own entry points for this path:
`embed_strings()`, `vector_search()`, `keyword_search()`, `hybrid_search()`, `rerank_chunks()` and the `RAGLiteConfig.search_method` /
`.reranker` plugin objects.  There is no CPU fallback: without the shared library (or a gfx950
GPU) the calls raise.
"""

from raglite_amd._chunking import (
    partition_chunks,
    partition_cost,
    partition_similarities,
    solve_partition_dp,
    split_chunks,
    split_chunks_batch,
)
from raglite_amd._chunklets import (
    chunklet_dp,
    compute_num_statements,
    markdown_chunklet_boundaries,
    partition_chunklets,
    split_chunklets,
    split_chunklets_batch,
    split_documents_batch,
)
from raglite_amd._sentences import (
    markdown_sentence_boundaries,
    partition_sentences,
    propagate_whitespace,
    sentence_dp,
    sentence_partition,
    split_sentences,
    split_sentences_batch,
    split_texts_batch,
    whitespace_mask,
)
from raglite_amd._config import HotPathConfig
from raglite_amd._markdown import MARKDOWN_OK, MARKDOWN_UNDECIDED, markdown_blocks_batch
from raglite_amd._embed import (
    embed_strings,
    embed_strings_batch,
    embed_strings_with_late_chunking,
    embed_strings_without_late_chunking,
    embedding_type,
    set_embedder_factory,
)
from raglite_amd._ops import (
    DeviceIndex,
    KeywordAnalyzer,
    KeywordIndex,
    KeywordStore,
    adapter_apply,
    merge_topk,
    pack_bits,
    rerank_order,
    SpanTable,
    rrf_fuse,
    shard_hybrid_fuse,
    get_default_option,
    pool_norm,
    set_default_option,
    set_device,
    synth_fill,
    topk,
)
from raglite_amd._keyword import analyze_texts_batch
from raglite_amd._search import (
    GpuIndex,
    hybrid_search,
    hybrid_search_batch,
    keyword_search,
    keyword_search_batch,
    reciprocal_rank_fusion,
    GpuVectorSearch,
    MaxSimRanker,
    attach_index,
    detach_index,
    rerank_chunks,
    rerank_chunks_batch,
    search_and_rerank_chunks,
    search_and_rerank_chunks_batch,
    ChunkSpan,
    retrieve_chunk_spans,
    retrieve_chunk_spans_batch,
    search_and_rerank_chunk_spans,
    search_and_rerank_chunk_spans_batch,
    retrieve_context,
    select_reranker,
    set_language_detector,
    vector_search,
    vector_search_batch,
)
from raglite_amd._cross_encoder import CrossEncoderShape, TorchCrossEncoderRanker
from raglite_amd._torch_embedder import EncoderShape, HashTokenizer, SentencePieceTokenizer, TorchTokenEmbedder
from raglite_amd._query_adapter import optimize_query_target_active_set, optimize_query_targets, update_query_adapter
from raglite_amd._comm import Communicator
from raglite_amd._attention import attention_varlen
from raglite_amd._encoder import NativeEncoder
from raglite_amd._wordpiece import DeviceWordPiece, WordPieceTables
from raglite_amd._sentencepiece import DeviceSentencePiece, UnigramTables
from raglite_amd._sharded import ShardedIndex, merge_topk_host, shard_bounds_by_chunk

__all__ = [
    "SentencePieceTokenizer",
    "set_default_option",
    "get_default_option",
    "partition_cost",
    "partition_similarities",
    "split_chunks",
    "split_chunks_batch",
    "partition_chunks",
    "solve_partition_dp",
    "split_chunklets", "split_chunklets_batch", "split_documents_batch", "partition_chunklets", "chunklet_dp",
    "markdown_chunklet_boundaries", "compute_num_statements",
    "split_sentences", "split_sentences_batch", "split_texts_batch", "partition_sentences", "sentence_dp", "sentence_partition",
    "markdown_sentence_boundaries", "whitespace_mask", "propagate_whitespace",
    "markdown_blocks_batch", "MARKDOWN_OK", "MARKDOWN_UNDECIDED",
    "hybrid_search",
    "hybrid_search_batch",
    "keyword_search",
    "keyword_search_batch",
    "vector_search_batch",
    "KeywordAnalyzer",
    "KeywordIndex",
    "KeywordStore",
    "analyze_texts_batch",
    "reciprocal_rank_fusion",
    "optimize_query_target_active_set",
    "optimize_query_targets",
    "update_query_adapter",
    "EncoderShape",
    "HashTokenizer",
    "TorchTokenEmbedder",
    "TorchCrossEncoderRanker",
    "CrossEncoderShape",
    "pack_bits",
    "rrf_fuse",
    "rerank_order",
    "rerank_chunks_batch",
    "search_and_rerank_chunks_batch",
    "ChunkSpan", "SpanTable", "retrieve_chunk_spans", "retrieve_chunk_spans_batch", "search_and_rerank_chunk_spans",
    "search_and_rerank_chunk_spans_batch", "retrieve_context",
    "shard_hybrid_fuse",
    "Communicator", "DeviceIndex", "GpuIndex", "GpuVectorSearch", "HotPathConfig", "MaxSimRanker", "ShardedIndex",
    "adapter_apply", "attach_index", "detach_index", "embed_strings", "embed_strings_with_late_chunking",
    "embed_strings_without_late_chunking", "embedding_type", "merge_topk", "merge_topk_host", "pool_norm",
    "rerank_chunks", "search_and_rerank_chunks", "select_reranker", "set_language_detector", "set_device", "set_embedder_factory", "shard_bounds_by_chunk",
    "synth_fill", "topk", "vector_search",
    "attention_varlen", "embed_strings_batch", "NativeEncoder",
    "DeviceWordPiece", "WordPieceTables",
    "DeviceSentencePiece", "UnigramTables",
]
__version__ = "0.1.0"
