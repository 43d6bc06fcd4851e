"""Decode-step driver: per-step metadata, the token-attention KV pool and the hipGraph-captured
decode step.  Counterpart of lite_llama/executor/{attention_metadata.py:19-44,
kv_cache_manager.py:197-299, model_runner.py:153-218,310-330, cuda_graph.py:54-249} and of the
one-shot decode loop engine/llm_engine.py:137-213 (greedy, no EOS stop, lockstep batch).

MI355X-first differences from the reference (extensions, not parity changes):
  * the WHOLE step -- forward, greedy argmax, KV-row bump, ``b_seq_len += 1``,
    ``update_kv_index`` and feeding the sampled token back -- is captured in one hipGraph, so a
    decode step is a single ``hipGraphLaunch`` with no host work in between (the reference
    replays only the forward and does 5 host-issued copies + sampler + index update per step);
  * the graph is also captured under tensor parallelism (RCCL all-reduces are capturable);
    the reference disables graphs for TP>1 (model_runner.py:260-266);
  * the reference's loop has no EOS stop; ``decode(stop=StopCriteria(...))`` ends rows at stop ids, stop sequences and
    per-row ``max_tokens`` -- the decision is taken on the device inside the captured step (csrc/decode_stop.hip in
    ``ll_decode_advance``'s place, executor/stopping.py), finished rows are frozen, the results say where and why each
    row ended (``last_lengths`` / ``last_finish_reasons``) and the loop ends early once every row has, without a host
    synchronisation per step.  Without ``stop`` the loop is the reference's: lockstep, ``max_new_tokens`` steps;
  * the reference emits one token per row per forward; ``decode(speculate=Speculation(...))`` verifies up to ``k`` drafted
    tokens per row in one forward over a ``[B, k + 1]`` grid on the paged pool (drafts from the row's own n-grams and from a
    caller's prediction, greedy acceptance, csrc/speculative.hip + executor/speculative.py): the tokens are those of the same
    grid with empty drafts, a row advances by every accepted draft plus one.
"""

from .. import _lib as L  # noqa: F401
from ..kernels import update_kv_index  # noqa: F401
from ..sampling import (MAX_TOP_LOGPROBS, Sampler, TokenLogprobs, apply_repetition_penalty, greedy_argmax,  # noqa: F401
                        sample_with_filters, token_logprobs)
from .chunking import ChunkPlan, plan_prefill_chunks  # noqa: F401
from .constraints import (ConstrainedRows, TokenAutomaton, constrained_argmax, constraint_advance, constraint_mask,  # noqa: F401
                          from_choices, from_transitions, union)
from .engine import SCORE_GEMM_ROWS, SCORE_LOGITS_BYTES, DecodeEngine, _check_logprobs, _Span  # noqa: F401
from .kv_cache_manager import KVCacheManager  # noqa: F401
from .kv_pool import KVPool  # noqa: F401
from .metadata import AttentionMetadata  # noqa: F401
from .slots import DEFAULT_BATCH_SIZES, DEFAULT_SEQ_LEN_BUCKETS, SlotBatch, SlotRunner, StepGraphs, slot_advance  # noqa: F401
from .speculative import (LDS_HISTORY_TOKENS, MAX_DRAFT_TOKENS, MAX_NGRAM, SpecState, Speculation, SpeculationStats,  # noqa: F401
                          spec_accept, spec_draft)
from .stopping import (MAX_STOP_SEQUENCE_LEN, MAX_STOP_SEQUENCES, MAX_STOP_TOKEN_IDS, RunningWatch, StopCriteria,  # noqa: F401
                       StopState, redirect_finished, stop_advance)
