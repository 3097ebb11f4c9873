"""ugrep_amd -- MI355X-native engine for ugrep's RE/flex DFA buffer-scan hot path.

The C ABI (include/ugpu.h, libugrep_amd.so) is the product boundary; this
package mirrors the reference's Pattern/Matcher FIND interface on top of it and
holds the multi-GPU shard stitching (dist.py).
"""
from ._lib import (ENC_LATIN1, ENC_NULL_DATA, ENC_PAGE, ENC_PLAIN, ENC_UTF8, ENC_UTF16BE, ENC_UTF16LE, ENC_UTF32BE,  # noqa: F401
                   ENC_UTF32LE)
from ._lib import (GEN_CODE, GEN_PLANTED, GEN_UTF8, GEN_WORDS, MODE_COUNT, MODE_OFFSETS, UgpuError,  # noqa: F401
                   Unsupported, lib)
from .matcher import (compile_regex, Matcher, Pattern, Records, Scanner, Stream, check_utf8, find_all, find_all_multi, find_nul, gen,  # noqa: F401
                      host_plan, host_prefilter, host_tables, host_transducer, is_binary, isutf8, lines,
                      LineResult, context_lines, grep_lines, line_spans, select_lines,
                      PositionResult, columns, find_positions,
                      IndexResult, index_batch, index_chunk, index_directory, index_inputs, index_tables,
                      parse_index_store, write_index_store,
                      IndexQuery, find_indexed, query_index_store,
                      ENCODINGS, decode_input, detect_bom, find_encoded, transcode, transcode_bound,
                      grep_bool, host_newline, host_ngram, host_ngram_candidates, parse_bool_query, select_lines_bool,
                      BatchResult, find_batch, host_batch_plan, split_matches)

__all__ = ["compile_regex", "Pattern", "Matcher", "Records", "Scanner", "Stream", "find_all", "find_all_multi", "gen", "host_tables", "host_plan", "host_prefilter", "Unsupported",
           "UgpuError", "lines", "isutf8", "check_utf8", "find_nul", "is_binary", "select_lines", "line_spans", "context_lines",
           "grep_lines", "LineResult", "select_lines_bool", "parse_bool_query", "grep_bool", "host_newline",
           "host_ngram", "host_ngram_candidates", "BatchResult", "find_batch", "host_batch_plan", "split_matches",
           "columns", "find_positions", "PositionResult",
           "detect_bom", "transcode", "transcode_bound", "decode_input", "find_encoded", "ENCODINGS",
           "IndexResult", "index_batch", "index_chunk", "index_directory", "index_inputs", "index_tables",
           "parse_index_store", "write_index_store", "IndexQuery", "find_indexed", "query_index_store"]
