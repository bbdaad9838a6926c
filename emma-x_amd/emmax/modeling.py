"""
modeling.py -- `AutoModelForVision2Seq`-compatible model object over the MI355X engine.

Keeps the surface of the reference's HF classes and of the native Emma-X entry point:
  * PrismaticForConditionalGeneration.forward / OpenVLAForActionPrediction.predict_action
        prismatic/extern/hf/modeling_prismatic.py:291-447, 492-566
  * PrismaticVLM.generate_actions(image, prompt_text, type, **kw)        prismatic/models/vlms/prismatic.py:627-696
  * README form  generate_actions(inputs, tokenizer, do_sample=False, max_new_tokens=512) -> (action, reasoning)
        README.md:27-50 (hub-only in the reference; rebuilt from the two sources above)
Same argument meaning and error behaviour; all device math runs in libemmax_hip.so.  The reference is batch-size-1 for
generation (modeling_prismatic.py:460-463); here rows of a batch (<= 64 per GPU) are independent and each equals the
reference's bs=1 result for that row.
"""

from __future__ import annotations

import dataclasses
import json
import os
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from .actions import ActionTokenizer, action_bin_token_ids, token_ids_to_actions, unnormalize
from .config import EmmaXConfig, check_decode_weight_dtype, default_norm_stats
from . import taps as _taps
from .engine import EmmaxEngine
from .policy_parser import Solver
from .processing import BatchFeature, EmmaXImageProcessor
from .scoring import IGNORE_INDEX, EmmaXScoreOutput, targets_for
from .sampling import MAX_DECODE_BATCH, BeamParams, LogitsProcessing, SamplingParams, check_top_logprobs, draw_seed, fold_bad_words
from .prompting import PurePromptBuilder
from .tokenizer_stub import StubTokenizer
from .weights import load_hf_state_dict, remap_native_state_dict, synthetic_state_dict, validate_state_dict

PREFIX_TOKEN_ID = 29871   # '▁' appended before action tokens (modeling_prismatic.py:513-516)


def load_tokenizer(path: Optional[str], cfg: EmmaXConfig):
    """The LLaMA-2 tokenizer of a checkpoint directory (tokenizer.json / tokenizer.model), right-padded, capped at
    llm_max_length (prismatic/models/backbones/llm/base_llm.py:146-171); None when the directory holds no tokenizer files."""
    if path and any(os.path.isfile(os.path.join(path, f)) for f in ("tokenizer.json", "tokenizer.model")):
        from transformers import AutoTokenizer   # host side only

        return AutoTokenizer.from_pretrained(path, model_max_length=cfg.llm.max_position, padding_side="right")
    return None


@dataclass
class EmmaXCausalLMOutputWithPast:
    """Field-compatible with PrismaticCausalLMOutputWithPast (modeling_prismatic.py:162-173)."""

    loss: Optional[torch.Tensor] = None
    logits: Optional[torch.Tensor] = None
    past_key_values: Optional[Any] = None
    hidden_states: Optional[Tuple[torch.Tensor, ...]] = None
    attentions: Optional[Tuple[torch.Tensor]] = None
    projector_features: Optional[torch.Tensor] = None


@dataclass
class EmmaXGenerateOutput:
    """generate(..., return_dict_in_generate=True): the fields of HF's GenerateDecoderOnlyOutput this model fills.  scores / logits: one
    fp32 [B, vocab] device tensor per generated position (output_scores / output_logits), NaN past a row's length; else None."""
    sequences: torch.Tensor
    scores: Optional[Tuple[torch.Tensor, ...]] = None
    logits: Optional[Tuple[torch.Tensor, ...]] = None
    # beam search (num_beams > 1; HF's GenerateBeamDecoderOnlyOutput): the returned hypotheses' scores [B * num_return_sequences] and, per
    # generated position, the row (group * num_beams + beam) each token was continued from, -1 behind the end; `logits` rows are then
    # [B * num_beams, vocab]: the rows the running beams read at each step
    sequences_scores: Optional[torch.Tensor] = None
    beam_indices: Optional[torch.Tensor] = None
    # top_logprobs=N / watch_ids=[...]: per generated position the N most likely ids and their log-probabilities, int32 / fp32 [B, T, N], and
    # the log-probabilities of the watched ids, fp32 [B, T, W] -- log_softmax of the RAW logits; past a row's length ids are -1, values NaN
    top_token_ids: Optional[torch.Tensor] = None
    top_logprobs: Optional[torch.Tensor] = None
    watch_logprobs: Optional[torch.Tensor] = None
    # what the call left cached (a KVHandle; its lengths are read back from the session): generate(..., past_key_values=it) continues from there
    past_key_values: Optional[Any] = None
    # output_hidden_states / output_attentions: HF's tuples over the generated tokens (TapsOutput describes them)
    hidden_states: Optional[Tuple] = None
    attentions: Optional[Tuple] = None

    def __getitem__(self, key: str):
        return getattr(self, key)


@dataclass
class TopLogprobsOutput:
    """The trailing object of generate_ids(..., top_logprobs=N, watch_ids=[...]): device tensors over the B result rows.  top_ids int32 /
    top_logprobs fp32 [B, max_new, N]: per emitted token the N most likely ids, best first (equal values by the lower id), and their
    log-probabilities; watch_logprobs fp32 [B, max_new, W]: those of the watched ids; logprobs fp32 [B, max_new]: the emitted tokens' own.
    All are log_softmax of the RAW logits (T = 1, unprocessed, unfiltered).  Entries past a row's length: ids -1, top / watched values
    NaN, logprobs 0."""
    top_ids: torch.Tensor
    top_logprobs: torch.Tensor
    watch_logprobs: torch.Tensor
    logprobs: torch.Tensor


@dataclass
class TapsOutput:
    """The trailing object of generate_ids(..., hidden=[...], attentions=[...]): HF generate's hidden_states / attentions -- a tuple over the
    generated tokens (T = the longest row's count); element 0 is the prompt pass, a tuple over the selected entries of fp32 [B, S, H] /
    [B, Hq, S, S] device tensors (a continuation: the new rows, [B, n, H] / [B, Hq, n, L]); element t >= 1 the decode step that emitted token t,
    [B, 1, H] / [B, Hq, 1, L + t].  Rows of different lengths: a list per row in place of the stacked tensor.  Entries of tokens a finished row
    did not emit are zeros.  None: not asked for."""
    hidden_states: Optional[Tuple] = None
    attentions: Optional[Tuple] = None


class KVHandle:
    """Opaque stand-in for HF `past_key_values`: the cache lives in the engine's paged KV memory.  lengths: the rows' cached lengths (patch rows
    included: n_patches of them per row, 0 behind a language-only forward); session: which session of the engine holds them -- a handle of a
    session that was re-created since names nothing."""

    def __init__(self, engine: EmmaxEngine, lengths: List[int], n_patches: int = 0):
        self.engine, self.lengths, self.n_patches = engine, list(lengths), int(n_patches)
        self.session = getattr(engine, "session_epoch", 0)


class EmmaXForActionPrediction:
    config_class = EmmaXConfig

    def __init__(self, config: EmmaXConfig, state_dict: Optional[Dict[str, torch.Tensor]] = None) -> None:
        self.config = config
        self.norm_stats = config.norm_stats
        self.bins = np.linspace(-1, 1, config.n_action_bins)
        self.bin_centers = (self.bins[:-1] + self.bins[1:]) / 2.0
        self.vocab_size = config.llm.vocab_size - config.pad_to_multiple_of   # modeling_prismatic.py:504
        self._state_dict = state_dict
        self.engine: Optional[EmmaxEngine] = None
        self.device = torch.device("cpu")
        self.dtype = torch.bfloat16
        self.training = False
        self.image_transform = EmmaXImageProcessor(config)
        self.tokenizer = None          # set by from_pretrained / from_synthetic, or assign one (`model.tokenizer = ...`)
        self.cache_reserve = 512       # KV room reserved behind a `forward(use_cache=True)` prefill for cached steps

    # ------------------------------------------------------------------------------------------------------------------
    # construction
    # ------------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path: str, torch_dtype: torch.dtype = torch.bfloat16, attn_implementation: Optional[str] = None,
                        low_cpu_mem_usage: bool = True, trust_remote_code: bool = True, load_in_8bit: bool = False,
                        load_in_4bit: bool = False, dtype: Optional[torch.dtype] = None, decode_weight_dtype: Optional[str] = None,
                        **_) -> "EmmaXForActionPrediction":
        """HF directory (config.json + *.safetensors [+ dataset_statistics.json]) or a native Prismatic `.pt` file.
        (`dtype=` is the transformers >= 5 spelling of `torch_dtype=`; `config=` passed by the Auto classes is ignored: the
        directory is re-read through EmmaXConfig.from_pretrained.)  `decode_weight_dtype`: "bf16" | "fp8" | "mxfp4" | "mxfp6", the format the decode
        step streams the LLM projections in (None: the config's, bf16)."""
        if load_in_8bit or load_in_4bit:
            raise NotImplementedError("bitsandbytes quantised loading (int8 / NF4 code books) is outside the MI355X hot path and no other format is "
                                      "substituted for it; the native quantised decode weights are decode_weight_dtype=\"fp8\", \"mxfp4\" or \"mxfp6\"")
        if decode_weight_dtype is not None:
            check_decode_weight_dtype(decode_weight_dtype)
        torch_dtype = dtype if dtype is not None else torch_dtype
        if torch_dtype not in (torch.bfloat16, None, "bfloat16", "auto"):
            raise ValueError("the MI355X path computes in bf16 (fp32 accumulate); pass torch_dtype=torch.bfloat16")
        path = str(path)
        if os.path.isfile(path) and path.endswith(".pt"):
            # native Prismatic checkpoint `<run_dir>/checkpoints/<step>.pt` (prismatic/models/load.py:133-144): the run directory
            # must hold `config.json` and `dataset_statistics.json` -- the reference asserts both, and so do we (no made-up
            # un-normalisation statistics)
            ckpt_dir = os.path.dirname(os.path.abspath(path))
            if os.path.basename(ckpt_dir) != "checkpoints":
                raise ValueError(f"Invalid checkpoint! expected `<run_dir>/checkpoints/<name>.pt`, got {path}")
            run_dir = os.path.dirname(ckpt_dir)
            cfg_json, stats_json = os.path.join(run_dir, "config.json"), os.path.join(run_dir, "dataset_statistics.json")
            if not os.path.isfile(cfg_json):
                raise FileNotFoundError(f"Missing `config.json` for run_dir = {run_dir}")
            if not os.path.isfile(stats_json):
                raise FileNotFoundError(f"Missing `dataset_statistics.json` for run_dir = {run_dir}")
            with open(cfg_json) as f:
                raw = json.load(f)
            cfg = EmmaXConfig.from_native_dict(raw)
            with open(stats_json) as f:
                cfg.norm_stats = json.load(f)
            sd = remap_native_state_dict(torch.load(path, map_location="cpu")["model"])
            tok_dir = run_dir
        else:
            cfg = EmmaXConfig.from_pretrained(path)
            sd = load_hf_state_dict(path)
            tok_dir = path
        validate_state_dict(sd, cfg)
        if decode_weight_dtype is not None:
            cfg.decode_weight_dtype = decode_weight_dtype
        model = cls(cfg, sd)
        model.tokenizer = load_tokenizer(tok_dir, cfg)   # the native class owns its tokenizer (prismatic.py:630); None if no files
        return model

    @classmethod
    def from_synthetic(cls, config: Optional[EmmaXConfig] = None, seed: int = 0, device: str = "cuda:0", planted: bool = False,
                       decode_weight_dtype: Optional[str] = None, **engine_kw) -> "EmmaXForActionPrediction":
        """Random-init weights with the real names/shapes, generated directly on `device` (no checkpoint offline).
        `decode_weight_dtype`: "bf16" | "fp8" | "mxfp4" | "mxfp6" (None: the config's)."""
        config = config or EmmaXConfig.emma_x_7b()
        if decode_weight_dtype is not None:
            config.decode_weight_dtype = check_decode_weight_dtype(decode_weight_dtype)
        if engine_kw.get("mxfp4_wide") and config.decode_weight_dtype != "mxfp4":   # (before the weights are generated on the device)
            raise ValueError(f"mxfp4_wide serves MXFP4 decode weights at 17-64 rows: this config has decode_weight_dtype={config.decode_weight_dtype!r}")
        if not config.norm_stats:   # synthetic weights come with synthetic (made-up) statistics; a checkpoint never does
            config.norm_stats = default_norm_stats()
        sd = synthetic_state_dict(config, seed=seed, device=device, dtype=torch.bfloat16, planted=planted)
        m = cls(config, sd)
        m.tokenizer = StubTokenizer()
        return m.to(device, **engine_kw)

    def to(self, device: Union[str, torch.device], max_batch: int = 1, max_prompt: int = 512,
           max_ctx: Optional[int] = None, exact: Optional[bool] = None, mxfp4_wide: Optional[bool] = None) -> "EmmaXForActionPrediction":
        """`exact=True`: exact numerics -- the reference's fp32 CPU arithmetic (prismatic.py:659-663 on CPU) instead of bf16 operands
        (include/emmax.h, tuning switch `exact`; 8 rows per launch, larger batches in chunks; None = the library's switch, EMMAX_EXACT).
        `mxfp4_wide=True`: MXFP4 decode weights serve 17-64 rows too (tuning switch `mx4_wide`, frozen into the model when it is created; opt-in;
        None = the library's switch, EMMAX_MX4_WIDE); a ValueError on any other decode_weight_dtype."""
        if mxfp4_wide and self.config.decode_weight_dtype != "mxfp4":
            raise ValueError(f"mxfp4_wide serves MXFP4 decode weights at 17-64 rows: this config has decode_weight_dtype={self.config.decode_weight_dtype!r}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("EmmaXForActionPrediction runs on MI355X (cuda:N) only; there is no CPU execution path")
        if self.engine is None:
            if self._state_dict is None:
                raise RuntimeError("no weights to load")
            self.engine = EmmaxEngine(self.config, self._state_dict, device=str(device), max_batch=max_batch,
                                      max_prompt=max_prompt, max_ctx=max_ctx, free_state_dict=True, exact=exact, mxfp4_wide=mxfp4_wide)
            self._state_dict = None
        elif device != self.device:
            raise RuntimeError("moving an already-materialised engine between devices is not supported")
        self.device = device
        return self

    def eval(self):
        return self

    def _need_engine(self) -> EmmaxEngine:
        if self.engine is None:
            raise RuntimeError("model is not on a HIP device yet: call .to('cuda:0') (no CPU fallback exists)")
        return self.engine

    # ------------------------------------------------------------------------------------------------------------------
    # stats helpers (modeling_prismatic.py:539-566, prismatic/models/vlas/openvla.py:128-137)
    # ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_unnorm_key(norm_stats: Dict[str, Dict[str, Any]], unnorm_key: Optional[str]) -> str:
        if unnorm_key is None and len(norm_stats) != 1:
            raise ValueError(
                "Your model was trained on more than one dataset. Please pass a `unnorm_key` from the following options to "
                f"choose the statistics used for de-normalizing actions: {norm_stats.keys()}")
        unnorm_key = unnorm_key if unnorm_key is not None else next(iter(norm_stats.keys()))
        if unnorm_key not in norm_stats:
            raise ValueError(f"The `unnorm_key` you chose ({unnorm_key = }) is not in the available statistics. "
                             f"Please choose from: {norm_stats.keys()}")
        return unnorm_key

    def get_action_dim(self, unnorm_key: Optional[str] = None) -> int:
        return len(self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]["q01"])

    def get_action_stats(self, unnorm_key: Optional[str] = None) -> Dict[str, Any]:
        return self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["action"]

    def get_proprio_stats(self, unnorm_key: Optional[str] = None) -> Dict[str, Any]:
        return self.norm_stats[self._check_unnorm_key(self.norm_stats, unnorm_key)]["proprio"]

    def get_prompt_builder(self, system_prompt: Optional[str] = None) -> PurePromptBuilder:
        return PurePromptBuilder("prismatic", system_prompt)

    # ------------------------------------------------------------------------------------------------------------------
    # core: vision + prefill (+ greedy loop)
    # ------------------------------------------------------------------------------------------------------------------
    def _rows(self, input_ids, attention_mask=None) -> List[List[int]]:
        """[B,P] tensor (+ optional right-padding mask) or ragged lists -> list of per-row id lists."""
        if isinstance(input_ids, torch.Tensor):
            ids = input_ids.detach().to("cpu", torch.long)
            if ids.ndim == 1:
                ids = ids[None]
            if attention_mask is not None:
                lens = attention_mask.detach().to("cpu").long().sum(-1).tolist()
            else:
                lens = [ids.shape[1]] * ids.shape[0]
            return [ids[b, : lens[b]].tolist() for b in range(ids.shape[0])]
        return [list(map(int, r)) for r in input_ids]

    def _encode_images(self, pixel_values=None, frames_u8=None) -> torch.Tensor:
        """`pixel_values` is the model input (reference contract).  `frames_u8` (the uint8 frame the processor ALSO emits) is
        only a faster route to the same numbers -- normalisation fused into the patch gather -- and is used when it is given
        alone, or when the caller's `pixel_values` still carries the processor's tag for that very frame (an augmented /
        re-cropped `pixel_values` tensor is a new object without the tag and is what gets encoded)."""
        eng = self._need_engine()
        if frames_u8 is not None and (pixel_values is None or getattr(pixel_values, "_emmax_frames_tag", None) is getattr(frames_u8, "_emmax_frames_tag", 0)):
            return eng.vision_encode(frames_u8.to(self.device).contiguous())
        if isinstance(pixel_values, dict):   # native layout {"dino": [B,3,H,W], "siglip": [B,3,H,W]}
            pixel_values = torch.cat([pixel_values["dino"], pixel_values["siglip"]], dim=1)
        return eng.vision_encode_pixels(pixel_values)

    def _prefill(self, rows: List[List[int]], pixel_values=None, frames_u8=None, max_new: int = 0, sampling=None, processing=None,
                 scores=None, logits=None, beams: Optional[BeamParams] = None, num_samples: int = 1, top=None, constraint=None,
                 constraint_start=None, taps=None) -> torch.Tensor:
        eng = self._need_engine()
        B = len(rows)
        src = pixel_values if pixel_values is not None else frames_u8
        nimg = src["dino"].shape[0] if isinstance(src, dict) else src.shape[0]
        if nimg != B:
            raise ValueError("Non-homogenous batch of (text, image) input -- forward() does not support mixed batches!")
        P = max(len(r) for r in rows)
        if P > self.config.llm.max_position:
            rows = [r[: self.config.llm.max_position] for r in rows]   # tokenizer truncation at llm_max_length
            P = self.config.llm.max_position
        N = int(num_samples)
        K = beams.num_beams if beams is not None else N
        if B * K > eng.max_decode_batch():
            what = f"{N} samples" if N > 1 else f"{K} beams"
            raise ValueError(f"{B} prompts x {what} exceed the {eng.max_decode_batch()} rows of a decode batch")
        eng.ensure_capacity(B * K, P, max(max_new, 1))
        patches = self._encode_images(pixel_values, frames_u8)
        if beams is None and getattr(eng, "beams", 0):
            eng.clear_beams()   # (first: sampling / processing cannot be set while beams are on)
        if N == 1 and getattr(eng, "sample_groups", 0):
            eng.clear_sample_groups()   # (and beams cannot be set while groups are on)
        # the call's automaton is the one the session holds: processing, which that automaton may have turned on with neutral values, is set
        # to neutral values instead of cleared (clearing it turns the automaton off, and the tables would be uploaded again for every call)
        keep = constraint is not None and processing is None and getattr(eng, "_automaton_set", None) is constraint and getattr(eng, "automaton", False)
        self._set_processing(eng, B * K, LogitsProcessing() if keep else processing, scores, logits, max_new)
        self._set_sampling(eng, B * K, sampling)
        if top is not None:   # (n_top, watch ids): bound behind sampling -- the launch reads the logit rows a sampled step writes
            eng.set_top_logprobs(top[0], top[1], max(max_new, 1))
        elif getattr(eng, "top_logprobs_bound", False):
            eng.clear_top_logprobs()
        if constraint is not None:   # behind processing: clearing that clears the automaton, and setting one turns neutral processing on
            eng.set_automaton(constraint)
            eng.set_automaton_starts(constraint.starts(constraint_start, B * K))
        elif getattr(eng, "automaton", False):
            eng.clear_automaton()
        if beams is not None:   # B groups prefill once each and decode as B x K rows on shared KV pages
            eng.set_beams(beams)
        if N > 1:   # B prompts prefill once each and fork into B x N sampled rows on the prompt's KV pages
            eng.set_sample_groups(N)
        if taps is not None:   # (taps.TapSpec) the pass fills them over its packed rows: self._pass_taps, with the rows' lengths
            S = [self.config.n_patches + len(r) for r in rows]
            self._pass_taps = eng.bind_pass_taps(taps, sum(S), max(S)) + (S, S)
        eng.prefill(rows, patches)
        return patches

    def _check_handle(self, handle, n_rows: int, who: str) -> None:
        eng = self._need_engine()
        if not isinstance(handle, KVHandle) or handle.engine is not eng:
            raise ValueError(f"{who}: past_key_values / continue_from must be the KVHandle an earlier call of this model returned")
        if handle.session != getattr(eng, "session_epoch", 0):
            raise ValueError(f"{who}: the handle's session was re-created since (a later call needed more rows, a longer prompt or more context than "
                             "the session had: create the model with max_batch / max_prompt / max_ctx, or raise cache_reserve, for the whole dialogue)")
        if n_rows != len(handle.lengths) or n_rows != getattr(eng, "_last_B", -1):
            raise ValueError(f"{who}: {n_rows} rows continue a cache of {len(handle.lengths)} rows: a continuation keeps the batch")

    def _continue(self, handle, rows: List[List[int]], max_new: int = 0, sampling=None, processing=None, scores=None, logits=None, top=None,
                  constraint=None, constraint_start=None, taps=None) -> None:
        """_prefill for rows that continue a cached context: no vision, no prefill -- the new ids are appended to what the handle's rows hold
        (engine.extend).  The session is never re-created here."""
        eng = self._need_engine()
        B = len(rows)
        self._check_handle(handle, B, "continue_from")
        if any(len(r) < 1 for r in rows):
            raise ValueError("every continued row needs at least one new id (the row's last emitted token, if nothing else)")
        if getattr(eng, "beams", 0) or getattr(eng, "sample_groups", 0):
            raise NotImplementedError("a cache left by beam search or sample groups is not continued (outside the hot path)")
        if processing is not None:
            ps = processing if isinstance(processing, (list, tuple)) else [processing]
            if any(p.repetition_penalty != 1.0 or p.no_repeat_ngram_size > 0 or p.min_new_tokens > 0 for p in ps):
                raise NotImplementedError("repetition_penalty / no_repeat_ngram_size / min_new_tokens with a continuation are outside the hot path: the "
                                          "processors' id history holds the prompt only, not the cached context it would have to read")
        if scores is not None or logits is not None:
            self._check_score_buffers(scores, logits, max_new, B, eng.cfg.llm.vocab_size)
        if getattr(eng, "automaton", False):
            eng.clear_automaton()    # (a constraint of this call enters at its start states: the extension restarts only rows outside an automaton)
        rules = processing is not None and any(p.rule_enable for p in (processing if isinstance(processing, (list, tuple)) else [processing]))
        if getattr(eng, "processing", False):
            eng.clear_processing()   # (history-reading processors are not continued; token rules / the automaton turn their neutral form on again)
        if rules:
            eng.set_token_rules(processing, n=B)
        elif getattr(eng, "token_rules", False):
            eng.clear_token_rules()
        if scores is not None or logits is not None:
            eng.set_scores(scores, logits, max_new, rows=B)
        elif getattr(eng, "scores_bound", False):
            eng.set_scores(None, None)
        self._set_sampling(eng, B, sampling)
        if top is not None:
            eng.set_top_logprobs(top[0], top[1], max(max_new, 1))
        elif getattr(eng, "top_logprobs_bound", False):
            eng.clear_top_logprobs()
        if constraint is not None:
            eng.set_automaton(constraint)
            eng.set_automaton_starts(constraint.starts(constraint_start, B))
        if taps is not None:   # the new rows alone; row i of sequence b sees the handle's cached keys and the rows up to itself
            n_new, keys = [len(r) for r in rows], [n + len(r) for n, r in zip(handle.lengths, rows)]
            self._pass_taps = eng.bind_pass_taps(taps, sum(n_new), max(keys)) + (n_new, keys)
        eng.extend(rows, max_new_tokens=max(max_new, 1))

    @staticmethod
    def _beam_args(num_beams=None, num_return_sequences=None, length_penalty=None, early_stopping=None, do_sample: bool = False,
                   processing=None, output_scores: bool = False) -> Optional[BeamParams]:
        """HF generate's beam arguments -> BeamParams (None: num_beams 1, today's greedy / sampled path).  Beam sampling, processors on
        beam log-probabilities and `scores` with beams are not built: they raise before the engine is touched."""
        k = 1 if num_beams is None else num_beams
        nrs = 1 if num_return_sequences is None else num_return_sequences
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
            raise ValueError(f"num_beams must be an integer >= 1, got {num_beams}")
        if int(k) == 1:
            if not do_sample and nrs != 1:
                raise ValueError(f"Greedy methods without beam search do not support `num_return_sequences` different than 1 (got {nrs}).")
            return None
        if do_sample:
            raise NotImplementedError("beam sampling (num_beams > 1 with do_sample=True) is outside the hot path")
        if processing is not None:
            raise NotImplementedError("logits processors on beam log-probabilities (repetition_penalty / no_repeat_ngram_size / min_new_tokens "
                                      "with num_beams > 1) are outside the hot path")
        if output_scores:
            raise NotImplementedError("output_scores with num_beams > 1 is outside the hot path (output_logits is served)")
        return BeamParams(int(k), 1.0 if length_penalty is None else length_penalty, False if early_stopping is None else early_stopping,
                          int(nrs) if isinstance(nrs, (int, np.integer)) and not isinstance(nrs, bool) else nrs)

    @staticmethod
    def _beam_kw(beams) -> Dict[str, Any]:
        """generate_ids' `beams` argument, passed only when there are beams (a greedy call is spelled exactly as before)."""
        return {} if beams is None else {"beams": beams}

    @staticmethod
    def _sample_group_args(do_sample: bool, num_beams=None, num_return_sequences=None) -> int:
        """HF generate's (do_sample=True, num_return_sequences=N) -> N sampled rows per prompt; 1 for every other call (greedy and beam calls
        keep their own checks in _beam_args).  N must be an integer >= 1: checked before the engine is touched."""
        if not do_sample or (num_beams is not None and num_beams != 1) or num_return_sequences is None:
            return 1
        return EmmaXForActionPrediction._check_num_samples(num_return_sequences, "num_return_sequences")

    @staticmethod
    def _check_num_samples(n, name: str = "num_samples") -> int:
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
            raise ValueError(f"{name} must be an integer >= 1, got {n!r}")
        return int(n)

    @staticmethod
    def _sample_kw(n: int) -> Dict[str, Any]:
        """generate_ids' `num_samples` argument, passed only when N > 1 (a plain call is spelled exactly as before)."""
        return {} if n == 1 else {"num_samples": n}

    def _kw_beams(self, kwargs, processing=None) -> Optional[BeamParams]:
        """The beam arguments of a **kwargs that the reference forwards to HF generate."""
        return self._beam_args(kwargs.get("num_beams"), kwargs.get("num_return_sequences"), kwargs.get("length_penalty"),
                               kwargs.get("early_stopping"), bool(kwargs.get("do_sample", False)), processing, bool(kwargs.get("output_scores", False)))

    @staticmethod
    def _set_processing(eng, B: int, processing, scores=None, logits=None, max_new: int = 0) -> None:
        """Before a prefill: processing = one LogitsProcessing for every row or one per row, None = off; scores / logits = the buffers
        the step fills (engine.set_scores), None = unbound.  What the call does not ask for is cleared from the session."""
        if scores is not None or logits is not None:
            EmmaXForActionPrediction._check_score_buffers(scores, logits, max_new, B, eng.cfg.llm.vocab_size)
        if processing is not None:
            eng.set_processing(processing, n=B)
        elif getattr(eng, "processing", False):
            eng.clear_processing()
        ps = processing if isinstance(processing, (list, tuple)) else [processing]
        if processing is not None and any(p.rule_enable for p in ps):   # the session's rule table and the rows' enable words
            eng.set_token_rules(processing, n=B)
        elif getattr(eng, "token_rules", False):
            eng.clear_token_rules()
        if scores is not None or logits is not None:
            eng.set_scores(scores, logits, max_new, rows=B)
        elif getattr(eng, "scores_bound", False):
            eng.set_scores(None, None)

    @staticmethod
    def _check_score_buffers(scores, logits, max_new: int, B: int, V: int) -> None:
        """scores / logits must be fp32 [max_new, B, V] tensors: the step stores row b's entry t at [t, b], so any other batch dimension
        would be written past its end or scrambled."""
        for name, t in (("scores", scores), ("logits", logits)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (int(max_new), B, V):
                got = f"{tuple(t.shape)} {t.dtype}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{name} must be a contiguous fp32 [max_new_tokens={max_new}, B={B}, vocab={V}] tensor, got {got}")

    @staticmethod
    def _processing_args(rows, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, min_length=None, sequence_bias=None,
                         bad_words_ids=None, suppress_tokens=None, begin_suppress_tokens=None, eos_token_id=None) -> Optional[LogitsProcessing]:
        """HF generate's processor arguments -> the LogitsProcessing every row gets (None: HF would add no processor).  min_length L (a
        total, prompt included) becomes min_new_tokens max(min_new_tokens, L - P_max), P_max the longest prompt, as HF counts it on a
        padded batch.  sequence_bias / bad_words_ids / suppress_tokens / begin_suppress_tokens are checked as HF's processors check them
        (a bad word that is the lone EOS id is dropped, as HF drops it)."""
        proc = LogitsProcessing(repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty,
                                no_repeat_ngram_size=0 if no_repeat_ngram_size is None else no_repeat_ngram_size,
                                min_new_tokens=0 if min_new_tokens is None else min_new_tokens, sequence_bias=sequence_bias,
                                bad_words_ids=fold_bad_words(bad_words_ids, eos_token_id), suppress_tokens=suppress_tokens,
                                begin_suppress_tokens=begin_suppress_tokens)   # (validates)
        if min_length is not None:
            if isinstance(min_length, bool) or not isinstance(min_length, (int, np.integer)) or min_length < 0:
                raise ValueError(f"min_length must be an integer >= 0, got {min_length}")
            m = max(int(proc.min_new_tokens), int(min_length) - max(len(r) for r in rows))
            proc = dataclasses.replace(proc, min_new_tokens=m)
        return None if proc.neutral else proc

    @staticmethod
    def _set_sampling(eng, B: int, sampling) -> None:
        """Before a prefill: sampling = one SamplingParams for every row or one per row (row b draws with subseq b; a params without a seed
        gets one from draw_seed), None = greedy -- which also clears what an earlier sampled call left in the session."""
        if sampling is not None:
            eng.set_sampling(sampling, n=B)
        elif getattr(eng, "sampling", False):
            eng.clear_sampling()
        ps = sampling if isinstance(sampling, (list, tuple)) else [sampling]
        if sampling is not None and any(p.has_warpers for p in ps):   # min_p / typical_p / epsilon_cutoff / eta_cutoff of the rows
            eng.set_warpers(sampling, n=B)
        elif getattr(eng, "warpers", False):
            eng.clear_warpers()

    @staticmethod
    def _sampling_args(do_sample: bool, temperature=None, top_k=None, top_p=None, seed=None, generator=None, min_p=None, typical_p=None,
                       epsilon_cutoff=None, eta_cutoff=None) -> Optional[SamplingParams]:
        """HF generate's sampling arguments -> the SamplingParams every row draws with (None: greedy).  Unset values take the HF defaults
        (temperature 1.0, top_k 50, top_p 1.0; top_k 0 = off; min_p / typical_p / epsilon_cutoff / eta_cutoff off); seed None =
        draw_seed(generator), so torch.manual_seed fixes a call.  Greedy calls consume no torch RNG and ignore the warpers, as HF does."""
        if not do_sample:
            return None
        t = 1.0 if temperature is None else float(temperature)
        if not t > 0.0:
            raise ValueError(f"`temperature` (={temperature}) has to be a strictly positive float when do_sample=True")
        p = SamplingParams(temperature=t, top_k=50 if top_k is None else top_k, top_p=1.0 if top_p is None else top_p, seed=seed,
                           min_p=0.0 if min_p is None else min_p, typical_p=1.0 if typical_p is None else typical_p,
                           epsilon_cutoff=0.0 if epsilon_cutoff is None else epsilon_cutoff,
                           eta_cutoff=0.0 if eta_cutoff is None else eta_cutoff)   # (validates)
        return p if seed is not None else dataclasses.replace(p, seed=draw_seed(generator))

    def _tap_args(self, output_hidden_states, output_attentions, tap_layers, num_beams=None, num_samples: int = 1) -> Optional["_taps.TapSpec"]:
        """output_hidden_states / output_attentions / tap_layers of a call -> taps.TapSpec (None: neither asked for), and what they are not
        served with, each with its own message, before the engine is touched."""
        spec = _taps.tap_spec(self.config.llm.num_layers, output_hidden_states, output_attentions, tap_layers)
        if spec is None:
            return None
        if self.engine is not None and getattr(self.engine, "exact", 0):
            raise NotImplementedError("output_hidden_states / output_attentions are not served by exact-numerics models (their fp32 cache has no "
                                      "probability kernel): load the model without exact=True for them")
        if num_beams is not None and num_beams != 1:
            raise NotImplementedError("output_hidden_states / output_attentions with num_beams > 1 are outside the hot path (the rows of a beam group "
                                      "reorder every step)")
        if num_samples != 1:
            raise NotImplementedError("output_hidden_states / output_attentions with num_return_sequences > 1 are outside the hot path (a sample "
                                      "group forks its rows behind the prompt pass)")
        return spec

    def forward(self, input_ids=None, attention_mask=None, pixel_values=None, labels=None, inputs_embeds=None,
                past_key_values=None, use_cache=None, output_attentions=None, output_hidden_states=None,
                output_projector_features=None, return_dict=None, frames_u8=None, tap_layers=None):
        """Multimodal forward -> logits for every position ([B,S,V] when rows have equal length, else a list), or one
        cached decode step when `input_ids.shape[1] == 1` and `past_key_values` is the handle of a previous call.
        output_hidden_states / output_attentions (every branch): `hidden_states` = a tuple of n_layers + 1 fp32 [B, S, H] tensors (entry 0 the
        embeddings with the patch rows spliced in -- they count in S, as in the reference -- entry i the residual stream behind layer i, the
        last one normed, as HF returns it), `attentions` = a tuple of n_layers fp32 [B, Hq, n, L] tensors (n new rows over L keys, zeros above
        the diagonal, HF's eager maps).  Rows of different lengths: each entry is a list with one tensor per row, the rule `logits` follows.
        They are written by the session's own pass through taps (include/emmax.h), not recomputed.  tap_layers=[...] (HF indices into those
        tuples, negative allowed; None = all, HF's meaning) keeps the selected entries only, in ascending order: the maps of all 32 layers of
        a 7B prompt of 768 rows are 32 x 768 x 32 x 768 x 4 bytes = 2.4 GB.  Not in exact numerics.
        labels (the three many-row branches; aligned with input_ids, -100 = ignored; on a cached context they cover the new ids): `loss` = HF's
        shifted mean cross-entropy as an fp32 0-dim device tensor, NaN when nothing is scored, from a fused lm-head pass that reads no logits
        (`score` is the same without `logits`).  The one-token cached branch asserts them away, as the reference does."""
        targets = None
        if labels is not None and input_ids is not None:   # checked before the engine is touched
            one_token = isinstance(input_ids, torch.Tensor) and input_ids.shape[-1] == 1 and past_key_values is not None
            assert not one_token, "Unexpected key `labels` provided during cached generation!"   # (modeling_prismatic.py:328)
            targets = self._targets_of(labels, self._rows(input_ids, attention_mask), attention_mask, pixel_values, frames_u8, past_key_values)
        eng = self._need_engine()
        spec = self._tap_args(output_hidden_states, output_attentions, tap_layers)
        # `inputs_embeds` is never consumed as data by the reference either: the cached branch hands the language model
        # inputs_embeds=None (modeling_prismatic.py:330-341), the multimodal branch embeds `input_ids` whatever else was passed
        # (:381), and the language-only branch asserts it away (:345).  Same behaviour here.
        if input_ids is None:
            raise ValueError("forward() needs `input_ids`: every branch of the reference embeds them (`inputs_embeds` is not read)")
        rows = self._rows(input_ids, attention_mask)
        if isinstance(input_ids, torch.Tensor) and input_ids.shape[-1] == 1 and past_key_values is not None:
            assert len(rows) == len(past_key_values.lengths), "cached step must keep the batch of the prefill"
            eng.set_current_tokens([r[0] for r in rows])
            hs = at = None
            if spec is not None:   # the single-step form of the step taps: every row lands in slot 0
                keys = [n + 1 for n in past_key_values.lengths]
                bufs = eng.bind_step_taps(spec, 1, max(keys))
            eng.decode_step()
            if spec is not None:
                eng.clear_taps()
                hs, at = _taps.cut_step(bufs[0], bufs[1], 0, keys)
            logits = eng.last_logits()[:, None, :]
            past_key_values.lengths = [n + 1 for n in past_key_values.lengths]
            return EmmaXCausalLMOutputWithPast(logits=logits, past_key_values=past_key_values, hidden_states=hs, attentions=at)
        if input_ids is not None and isinstance(input_ids, torch.Tensor) and input_ids.shape[-1] == 1:
            assert past_key_values is not None, "You must provide `past_key_values` during cached generation!"
        handle, hs, at, patches = self._many_row_pass(rows, pixel_values, frames_u8, past_key_values, use_cache, spec, inputs_embeds, "forward")
        loss = None if targets is None else self._score_rows(eng, targets)[0]   # the fused pass: lse / target logit / argmax per row, no logits read
        per_row = eng.prefill_logits()
        same = len({t.shape[0] for t in per_row}) == 1
        return EmmaXCausalLMOutputWithPast(loss=loss, logits=torch.stack(per_row) if same else per_row, past_key_values=handle, hidden_states=hs,
                                           attentions=at, projector_features=patches if output_projector_features else None)

    def _many_row_pass(self, rows, pixel_values, frames_u8, past_key_values, use_cache, spec, inputs_embeds, who: str):
        """The three many-row branches of forward -- n > 1 new ids on a cached context, language-only, multimodal -- up to and excluding what reads
        the rows' logits.  -> (the handle the call returns, hidden_states, attentions, the patch embeddings of a multimodal pass)"""
        eng = self._need_engine()
        if past_key_values is not None and pixel_values is None and frames_u8 is None:
            # n > 1 new ids per row on top of the handle's cache (ragged rows: lists, or a right-padding mask): one pass over the new rows alone
            self._check_handle(past_key_values, len(rows), who)
            self._set_processing(eng, len(rows), None)   # (as the language-only branch: what an earlier generate left in the session is cleared)
            hs = at = None
            if spec is not None:
                n_new, keys = [len(r) for r in rows], [n + len(r) for n, r in zip(past_key_values.lengths, rows)]
                bufs = eng.bind_pass_taps(spec, sum(n_new), max(keys))
            eng.extend(rows, max_new_tokens=0)
            if spec is not None:
                hs, at = _taps.cut_pass(bufs[0], bufs[1], n_new, keys)
            past_key_values.lengths = [n + len(r) for n, r in zip(past_key_values.lengths, rows)]
            return past_key_values, hs, at, None
        if pixel_values is None and frames_u8 is None:
            # unimodal forward (modeling_prismatic.py:343-359): text only, no patch rows
            assert inputs_embeds is None, "Missing `input_ids` in language-only forward!"
            assert past_key_values is None, "Unexpected key `past_key_values` provided during language-only forward!"
            eng.ensure_capacity(len(rows), max(len(r) for r in rows), self.cache_reserve if use_cache else 1)
            self._set_processing(eng, len(rows), None)   # (as _prefill: what an earlier generate left in the session is cleared)
            hs = at = None
            if spec is not None:
                if getattr(eng, "beams", 0):
                    eng.clear_beams()
                if getattr(eng, "sample_groups", 0):
                    eng.clear_sample_groups()
                S = [len(r) for r in rows]
                bufs = eng.bind_pass_taps(spec, sum(S), max(S))
            eng.prefill(rows, None)
            if spec is not None:
                hs, at = _taps.cut_pass(bufs[0], bufs[1], S, S)
            return (KVHandle(eng, eng._last_S) if use_cache else None), hs, at, None
        if past_key_values is not None:
            raise ValueError(f"{who}(past_key_values=...) extends the cached rows with text ids: pass no pixel_values / frames_u8 with it")
        patches = self._prefill(rows, pixel_values, frames_u8, max_new=self.cache_reserve if use_cache else 0, taps=spec)
        hs, at = _taps.cut_pass(*self._pass_taps) if spec is not None else (None, None)
        self._pass_taps = None
        return (KVHandle(eng, eng._last_S, self.config.n_patches) if use_cache else None), hs, at, patches

    def _targets_of(self, labels, rows, attention_mask, pixel_values, frames_u8, past_key_values) -> List[List[int]]:
        """labels -> the target id of every logit row of the pass these arguments select (scoring.targets_for), checked before the engine is touched"""
        multimodal = pixel_values is not None or frames_u8 is not None
        return targets_for(labels, rows, attention_mask, n_patches=self.config.n_patches if multimodal else 0,
                           new_rows_only=past_key_values is not None and not multimodal, vocab=self.config.llm.vocab_size)

    @staticmethod
    def _score_rows(eng, targets):
        """engine.score on the rows of the last pass -> (loss, token_logprobs, predicted_ids, lse, n_scored); loss = -sum(target_logit - lse) /
        n_scored as an fp32 0-dim device tensor, NaN when nothing is scored (HF's mean over nothing); per-row lists otherwise, NaN log-probabilities
        where nothing was scored"""
        lse, tl, am = eng.score(targets)
        scored = [torch.tensor([t != IGNORE_INDEX for t in row], dtype=torch.bool).to(lse[0].device) for row in targets]
        n = sum(int(t != IGNORE_INDEX) for row in targets for t in row)
        lp = [torch.where(m, a - b, torch.full_like(a, float("nan"))) for m, a, b in zip(scored, tl, lse)]
        total = torch.stack([torch.where(m, x, torch.zeros_like(x)).sum() for m, x in zip(scored, lp)]).sum()
        return -total / float(n) if n else torch.full((), float("nan"), device=total.device), lp, am, lse, n

    @torch.inference_mode()
    def score(self, input_ids, attention_mask=None, pixel_values=None, frames_u8=None, labels=None, past_key_values=None, use_cache=False):
        """Teacher-forced scoring without logits: the pass `forward` would run -- multimodal, language-only, or n > 1 new ids on the handle of an
        earlier call -- followed by the fused lm-head pass that keeps three numbers per row.  labels as forward takes them (aligned with input_ids,
        -100 = ignored; on a cached context they cover the new ids, whose first is not scored); None scores the input itself (perplexity).
        -> EmmaXScoreOutput.  The action metrics of the reference's evaluation follow from it: actions.action_token_metrics(predicted_ids, targets,
        config) with targets = scoring.targets_for(...)."""
        if input_ids is None:
            raise ValueError("score() needs `input_ids`")
        rows = self._rows(input_ids, attention_mask)
        if past_key_values is not None and all(len(r) == 1 for r in rows):
            raise ValueError("score(past_key_values=...) scores n > 1 new ids per row: the row that predicts a single new id belongs to the earlier pass")
        targets = self._targets_of(labels, rows, attention_mask, pixel_values, frames_u8, past_key_values)   # (checked before the engine is touched)
        eng = self._need_engine()
        if getattr(eng, "exact", 0):
            raise NotImplementedError("score: exact-numerics models are not scored (the scoring kernel has no two-term form)")
        handle, _, _, _ = self._many_row_pass(rows, pixel_values, frames_u8, past_key_values, use_cache, None, None, "score")
        loss, lp, am, lse, n = self._score_rows(eng, targets)
        same = len({t.shape[0] for t in lp}) == 1
        st = (lambda xs: torch.stack(xs)) if same else (lambda xs: xs)
        return EmmaXScoreOutput(loss=loss, token_logprobs=st(lp), predicted_ids=st(am), lse=st(lse), n_scored=n, past_key_values=handle)

    __call__ = forward

    @torch.inference_mode()
    def generate_ids(self, rows: List[List[int]], pixel_values=None, frames_u8=None, max_new_tokens: int = 512,
                     stop_on_eos: bool = True, sampling=None, return_logprobs: bool = False, processing=None, scores=None, logits=None,
                     beams: Optional[BeamParams] = None, num_samples: int = 1, top_logprobs: int = 0, watch_ids: Optional[Sequence[int]] = None,
                     constraint=None, constraint_start=None, continue_from=None, return_handle: bool = False, hidden: Optional[Sequence[int]] = None,
                     attentions: Optional[Sequence[int]] = None, draft=None, draft_params=None, return_draft_stats: bool = False):
        """Decode every row: greedy, or sampled in the step with `sampling` (one SamplingParams for all rows or one per row; row b draws
        with subseq b).  `processing` (one LogitsProcessing for all rows or one per row) applies HF's repetition penalty / n-gram ban /
        min-new-tokens in the step first.  `scores` / `logits`: fp32 [max_new, B, vocab] device buffers the step fills with HF's scores /
        raw logits at each emitted token's index (others are not written); any other shape is refused before the engine is touched, and
        the buffers are unbound again when the call returns.  Returns device tensors (new_ids int32 [B,max_new] pad-filled,
        lens int32 [B]), and with return_logprobs (sampling only) the fp32 [B,max_new] log-probabilities of the emitted tokens.
        `beams` (BeamParams; no sampling, processing or scores with it): beam search in the step.  The B rows are groups, the result has
        B x num_beams rows -- row g K + k = the k-th best hypothesis of group g -- and `logits` is [max_new, B x num_beams, vocab];
        engine.beam_result() / beam_trace() hold the scores, beam_indices and the per-step trace.
        `num_samples` = N > 1 (needs `sampling`; no beams): every row is a prompt that is prefilled once and forked into N sampled rows on its
        KV pages.  The result has B x N rows -- row b N + j = sample j of prompt b, drawing with subseq b N + j by default -- `sampling` /
        `processing` lists have one entry per result row (or one entry for all), and `scores` / `logits` are [max_new, B x N, vocab].
        `top_logprobs` = n (1..20) and / or `watch_ids` (up to 256 ids): the return gains one trailing TopLogprobsOutput -- per emitted token the
        n most likely ids with their log-probabilities and the log-probabilities of the watched ids, over the RAW logits, and the emitted
        tokens' own.  A greedy call samples at temperature 0 underneath (the greedy ids) and is greedy again afterwards.  Works with
        num_samples (B x N rows); not with beams.
        `constraint` (constraints.TokenAutomaton): constrained decoding in the step -- a row in automaton state s can only emit the ids that
        state allows (HF's prefix_allowed_tokens_fn, compiled).  `constraint_start`: None = every row enters at the automaton's entry "start"
        (state 0 without one), a name / state = every row there, a list = one per result row (None in it: that row is unconstrained).  Works
        greedy, sampled and with num_samples; not with beams.  Scores are -inf at the ids the automaton forbids; log-probabilities stay raw.
        `continue_from` (the KVHandle of an earlier call on the same rows): `rows` are the NEW ids per row, appended to what the handle's rows
        hold -- no vision, no prefill, one pass over the new rows (engine.extend).  A row's last emitted token is not cached: pass it first.
        Greedy, sampling, warpers, token rules, top_logprobs / watch_ids, scores and constraint work as after a prefill; beams, num_samples > 1
        and repetition_penalty / no_repeat_ngram_size / min_new_tokens raise NotImplementedError.
        `return_handle`: the return gains one trailing KVHandle of what the call leaves cached (lengths read back from the session).
        `hidden` / `attentions` (lists of entries of HF's hidden_states / attentions tuples, ascending; None = off): the return gains one trailing
        TapsOutput, the LAST element -- per generated token the selected hidden states and attention maps, written by the prompt pass and by
        every decode step through the session's taps (include/emmax.h).  Greedy, sampled, with processors, warpers, a constraint,
        top_logprobs and continue_from; not with beams or num_samples > 1, not in exact numerics.  The ids are those of the same call without.
        `draft` (one list of ids or None per row; None = off, today's path): draft-verified greedy decoding (drafting.py) -- each row's draft,
        typically the ids the previous call on almost the same scene generated, is checked window by window in verify passes and the longest
        prefix the model's own argmax agrees with is kept: the ids and lens are exactly those of the call without, in fewer weight passes.
        `draft_params`: drafting.DraftParams.  `return_draft_stats` (with a draft only): the return gains a trailing drafting.DraftStats (behind the handle).
        `stop_on_eos` has nothing to do with a draft: the loop ends when every row is done on the device (EOS, budget, stop rule), the ids are the same.
        Greedy only: sampling, processors / warpers / token rules, a constraint, beams, num_samples > 1, scores / logits, top_logprobs /
        watch_ids, hidden / attentions, fp8 decode weights and exact numerics raise NotImplementedError before the engine is touched."""
        if draft is not None:
            self._check_draft(draft, len(rows), sampling=sampling, processing=processing, scores=scores, logits=logits, beams=beams,
                              num_samples=num_samples, top=bool(top_logprobs) or bool(watch_ids), constraint=constraint,
                              taps=hidden is not None or attentions is not None, return_logprobs=return_logprobs)
        spec = None
        if hidden is not None or attentions is not None:
            spec = _taps.TapSpec(sorted(set(int(i) for i in hidden or [])), sorted(set(int(i) for i in attentions or [])))
            nl = self.config.llm.num_layers
            if not spec.any or any(not 0 <= i <= nl for i in spec.hidden) or any(not 0 <= i < nl for i in spec.attn):
                raise ValueError(f"hidden takes entries 0..{nl}, attentions layers 0..{nl - 1}, at least one of them (got {hidden!r}, {attentions!r})")
            if beams is not None:
                raise NotImplementedError("hidden states / attention maps with num_beams > 1 are outside the hot path (the rows of a beam group reorder every step)")
            if self._check_num_samples(num_samples) > 1:
                raise NotImplementedError("hidden states / attention maps with num_return_sequences > 1 are outside the hot path (a sample group forks its "
                                          "rows behind the prompt pass)")
            if self.engine is not None and getattr(self.engine, "exact", 0):
                raise NotImplementedError("hidden states / attention maps are not served by exact-numerics models")
        if continue_from is not None:
            if beams is not None:
                raise NotImplementedError("num_beams > 1 with a continuation is outside the hot path (beams fork their rows from a fresh prefill)")
            if self._check_num_samples(num_samples) > 1:
                raise NotImplementedError("num_return_sequences > 1 with a continuation is outside the hot path (sample groups fork from a fresh prefill)")
            if pixel_values is not None or frames_u8 is not None:
                raise ValueError("a continuation appends text ids to the cached rows: pass no pixel_values / frames_u8 with continue_from")
        cst = self._check_constraint(constraint, constraint_start, beams.num_beams if beams is not None else 1,
                                     len(rows) * self._check_num_samples(num_samples))
        n_top, watch = check_top_logprobs(top_logprobs, watch_ids, self.config.llm.vocab_size, "generate_ids")
        want_top = n_top > 0 or len(watch) > 0
        if want_top and beams is not None:
            raise NotImplementedError("top_logprobs / watch_ids with num_beams > 1 are outside the hot path (output_logits is served)")
        N = self._check_num_samples(num_samples)
        if N > 1:
            if beams is not None:
                raise ValueError("num_samples > 1 runs without beams (beam sampling is not built)")
            if sampling is None:
                raise ValueError(f"num_samples={N} needs sampling: {N} greedy rows of one prompt would be identical")
            if len(rows) * N > MAX_DECODE_BATCH:
                raise ValueError(f"{len(rows)} prompts x {N} samples exceed the {MAX_DECODE_BATCH} rows of a decode batch")
        eng = self._need_engine()
        if beams is not None:
            if not isinstance(beams, BeamParams):
                raise ValueError("beams must be BeamParams")
            if sampling is not None or processing is not None or scores is not None:
                raise ValueError("beams run without sampling, logits processing and scores")
        if return_logprobs and sampling is None and not want_top:
            raise ValueError("return_logprobs needs sampling (log-probabilities are kept by the sampled step only)")
        if processing is not None:
            ps = processing if isinstance(processing, (list, tuple)) else [processing]
            if not all(isinstance(p, LogitsProcessing) for p in ps):
                raise ValueError("processing must be LogitsProcessing (one, or one per row)")
        self._check_score_buffers(scores, logits, max_new_tokens, len(rows) * (beams.num_beams if beams is not None else N),
                                  self.config.llm.vocab_size)
        def start(**kw):   # the rows' context: a prefill, or the new ids on top of what continue_from holds
            if spec is not None:
                kw["taps"] = spec
            if continue_from is not None:
                self._continue(continue_from, rows, **kw)
            else:
                self._prefill(rows, pixel_values, frames_u8, beams=beams, **self._sample_kw(N), **kw)
            if spec is not None and max_new_tokens > 1:   # the steps' taps, bound behind the pass: the step emitting token t sees keys[b] + t keys
                self._step_taps = eng.bind_step_taps(spec, max_new_tokens, max(self._pass_taps[3]) + max_new_tokens - 1)

        def taps_out(lens):   # HF's layout over the generated tokens: element 0 the prompt pass, element t the step that emitted token t
            if spec is None:
                return ()
            ph, pa, n_new, keys = self._pass_taps
            sh, sa = self._step_taps if max_new_tokens > 1 else (None, None)
            if max_new_tokens > 1:
                eng.clear_taps()
            self._pass_taps = self._step_taps = None
            steps = [_taps.cut_pass(ph, pa, n_new, keys)] + [_taps.cut_step(sh, sa, t, [k + t for k in keys]) for t in range(1, max(int(lens.max()), 1))]
            return (TapsOutput(hidden_states=tuple(s[0] for s in steps) if spec.hidden else None,
                               attentions=tuple(s[1] for s in steps) if spec.attn else None),)

        def handle():      # what the call leaves cached (the rows of the result: beams / sample groups have B x K of them)
            if not return_handle:
                return ()
            n_pat = continue_from.n_patches if continue_from is not None else self.config.n_patches
            return (KVHandle(eng, eng.context_lengths(0, eng._last_B * (beams.num_beams if beams is not None else 1)), n_pat),)

        if not want_top:
            start(max_new=max_new_tokens, sampling=sampling, processing=processing, scores=scores, logits=logits, **cst)
            if draft is not None:
                out, dstats = self._drafted_generate(eng, draft, max_new_tokens, draft_params)
                return tuple(out) + handle() + ((dstats,) if return_draft_stats else ())
            out = eng.generate(max_new_tokens, stop_on_eos, return_logprobs=return_logprobs)
            if scores is not None or logits is not None:
                eng.set_scores(None, None)   # the buffers are the caller's now: no later step or prefill writes into them
            return tuple(out) + handle() + taps_out(out[1]) if return_handle or spec is not None else out
        # a greedy caller: temperature-0 sampling underneath (the argmax of the same fp32 rows), so that the logit rows are written
        start(max_new=max_new_tokens, sampling=sampling if sampling is not None else SamplingParams(0.0, 0, 1.0, seed=0),
              processing=processing, scores=scores, logits=logits, top=(n_top, watch), **cst)
        ids, lens, lp = eng.generate(max_new_tokens, stop_on_eos, return_logprobs=True)
        B = ids.shape[0]
        ti, tl, wl = (t[:B] for t in eng._top_bufs)
        eng.clear_top_logprobs()   # the state of before: the buffers are the caller's, and a greedy session is greedy again
        if scores is not None or logits is not None:
            eng.set_scores(None, None)
        if sampling is None:
            eng.clear_sampling()
        top = TopLogprobsOutput(top_ids=ti, top_logprobs=tl, watch_logprobs=wl, logprobs=lp)
        return ((ids, lens, lp, top) if return_logprobs else (ids, lens, top)) + handle() + taps_out(lens)

    def _check_draft(self, draft, n_rows: int, sampling=None, processing=None, scores=None, logits=None, beams=None, num_samples: int = 1,
                     top: bool = False, constraint=None, taps: bool = False, return_logprobs: bool = False) -> None:
        """What a draft is not served with (include/emmax.h: emmax_verify refuses the same), checked before the engine is touched."""
        def no(what):
            raise NotImplementedError(f"draft-verified decoding is greedy on raw logits: {what} with a draft is outside the hot path")
        if sampling is not None or return_logprobs:
            no("do_sample / sampling")
        if processing is not None:
            no("logits processors / warpers / token rules")
        if constraint is not None:
            no("a constraint (constrain_to_bins included)")
        if beams is not None:
            no("num_beams > 1")
        if self._check_num_samples(num_samples) > 1:
            no("num_return_sequences > 1")
        if scores is not None or logits is not None or top:
            no("output_scores / output_logits / top_logprobs / watch_ids")
        if taps:
            no("output_hidden_states / output_attentions")
        if self.config.decode_weight_dtype == "fp8":
            no("fp8 decode weights (their prefill multiplies by the unquantised matrices: the pass would verify another model)")
        if self.engine is not None and getattr(self.engine, "exact", 0):
            no("an exact-numerics model")
        if draft is not None and (not isinstance(draft, (list, tuple)) or len(draft) != n_rows):
            raise ValueError(f"draft takes one list of ids or None per row ({n_rows} rows)")

    @staticmethod
    def _draft_kw(draft_ids, n_rows: int, draft_params=None) -> Dict[str, Any]:
        """generate_ids' draft arguments from a caller's draft_ids (None: none -- the call is spelled exactly as before): one list of ids or
        None per row, a [B, n] tensor, or for one row the flat list of its ids."""
        if draft_ids is None:
            return {}
        if isinstance(draft_ids, torch.Tensor):
            draft_ids = draft_ids.tolist()
        draft_ids = list(draft_ids)
        if n_rows == 1 and draft_ids and not isinstance(draft_ids[0], (list, tuple, type(None))):
            draft_ids = [draft_ids]
        draft = [None if d is None else [int(t) for t in d] for d in draft_ids]
        return {"draft": draft, **({} if draft_params is None else {"draft_params": draft_params})}

    def _drafted_generate(self, eng, draft, max_new_tokens: int, draft_params=None):
        """drafting.drafted_generate over the rows the call's prefill / extension left, as eng.generate returns them: (ids int32 [B, max_new]
        pad-filled, lens int32 [B]) on the device, and the DraftStats."""
        from . import drafting

        params = draft_params or drafting.DraftParams()
        room = (self.config.n_patches + eng.max_prompt) * eng.max_batch // max(len(draft), 1)   # the packed rows of one pass: the prefill's scratch
        if params.window > room:
            params = drafting.DraftParams(max(room, 2), params.ngram, params.burst, params.give_up)
        ids, lens, stats = drafting.drafted_generate(eng, [None if d is None else [int(t) for t in d] for d in draft], int(max_new_tokens), params)
        out = torch.full((len(ids), int(max_new_tokens)), int(self.config.pad_token_id), dtype=torch.int32)
        for b, r in enumerate(ids):
            out[b, :len(r)] = torch.as_tensor(r, dtype=torch.int32)
        self.last_draft_stats = stats
        return (out.to(eng.device), torch.as_tensor(lens, dtype=torch.int32).to(eng.device)), stats

    def _check_constraint(self, constraint, constraint_start, num_beams: int, n_rows: int) -> Dict[str, Any]:
        """`constraint` / `constraint_start` of a call, checked before the engine is touched -> _prefill's keywords ({}: no constraint)."""
        from .constraints import TokenAutomaton

        if constraint is None:
            if constraint_start is not None:
                raise ValueError("constraint_start needs constraint= (a constraints.TokenAutomaton)")
            return {}
        if not isinstance(constraint, TokenAutomaton):
            raise ValueError("constraint must be a constraints.TokenAutomaton (constraints.build / action_bins / policy_line make one)")
        if num_beams > 1:
            raise NotImplementedError("constraint= with num_beams > 1 is outside the hot path (the automaton runs in the greedy and sampled finish)")
        if constraint.vocab != self.config.llm.vocab_size:
            raise ValueError(f"the constraint is over {constraint.vocab} ids, the model's vocabulary has {self.config.llm.vocab_size}")
        constraint.starts(constraint_start, n_rows)   # (validates)
        return {"constraint": constraint, "constraint_start": constraint_start}

    def _bin_automaton(self, dim: int):
        """constraints.action_bins for `dim` action tokens of this model, built once per (vocabulary, bins, dim, tokenizer vocabulary): the
        same object every call, so the session keeps its tables."""
        from .constraints import action_bins

        key = (self.config.llm.vocab_size, self.config.n_action_bins, int(dim), self.vocab_size)
        cache = self.__dict__.setdefault("_bin_automata", {})
        if key not in cache:
            cache[key] = action_bins(key[0], key[1], key[2], token_vocab=key[3])
        return cache[key]

    def _kw_constraint(self, kwargs) -> Dict[str, Any]:
        """The constraint arguments of a **kwargs, passed on only when given; prefix_allowed_tokens_fn (a Python callback per row per step cannot
        run inside the step) points at them."""
        if kwargs.get("prefix_allowed_tokens_fn") is not None:
            raise NotImplementedError("prefix_allowed_tokens_fn is a Python callback per row and step and cannot run in the decode step: compile the "
                                      "constraint into a constraints.TokenAutomaton and pass constraint= (and constraint_start=)")
        if kwargs.get("constraint") is None and kwargs.get("constraint_start") is None:
            return {}
        nb = kwargs.get("num_beams")
        if kwargs.get("constraint") is not None and nb is not None and nb != 1:
            raise NotImplementedError("constraint= with num_beams > 1 is outside the hot path (the automaton runs in the greedy and sampled finish)")
        return {"constraint": kwargs.get("constraint"), "constraint_start": kwargs.get("constraint_start")}

    def _max_new(self, rows, max_new_tokens, max_length, min_length, had_max_new: bool = True) -> int:
        """HF length semantics: `max_length` counts the PROMPT too (as HF counts it: the text ids, not the patch rows) and only
        applies when `max_new_tokens` is not given; `min_length` (total length, HF default 0) above the prompt length would
        suppress EOS -- outside the greedy hot path, so it raises instead of being ignored."""
        plen = max(len(r) for r in rows)
        if min_length is not None and int(min_length) > plen + 1:
            raise NotImplementedError(f"min_length={min_length} beyond the prompt ({plen} ids) needs EOS suppression, outside the hot path")
        if max_new_tokens is None:
            if max_length is None:
                max_new_tokens = 20       # HF GenerationConfig default max_length=20 is a total; keep the historical default here
            else:
                max_new_tokens = max(int(max_length) - plen, 1)
        return int(max_new_tokens)

    @torch.inference_mode()
    def generate(self, input_ids=None, pixel_values=None, attention_mask=None, max_new_tokens: Optional[int] = None, do_sample: bool = False,
                 min_length: int = 1, temperature: Optional[float] = None, frames_u8=None, top_k: Optional[int] = None,
                 top_p: Optional[float] = None, seed: Optional[int] = None, generator: Optional[torch.Generator] = None,
                 repetition_penalty: Optional[float] = None, no_repeat_ngram_size: Optional[int] = None, min_new_tokens: Optional[int] = None,
                 output_scores: bool = False, output_logits: bool = False, return_dict_in_generate: bool = False, top_logprobs: int = 0,
                 watch_ids: Optional[Sequence[int]] = None, past_key_values=None, output_hidden_states: bool = False, output_attentions: bool = False,
                 tap_layers: Optional[Sequence[int]] = None, draft_ids=None, prompt_lookup_num_tokens: Optional[int] = None, draft_params=None,
                 **kwargs):
        """HF-style: returns LongTensor [B, P + T] = prompt ++ generated (right-padded with pad_token_id).  do_sample=True draws every token
        in the decode step (include/emmax.h: emmax_session_set_sampling) with temperature / top_k / top_p (HF defaults 1.0 / 50 / 1.0 when
        unset); row b draws with (seed, subseq b), seed None = draw_seed(generator).  With num_return_sequences=N the prompt is prefilled once
        and decoded as N sampled rows on its KV pages: [B N, P + T], row b N + j = sample j of prompt b (scores / logits: [B N, vocab] each).
        repetition_penalty / no_repeat_ngram_size /
        min_new_tokens / min_length are applied in the step as HF's processors (emmax_session_set_processing).  return_dict_in_generate=True
        returns an EmmaXGenerateOutput: `sequences` (the tensor), and with output_scores / output_logits a tuple of T = max(lens) fp32
        [B, vocab] device tensors each (NaN past a row's length).  constraint= (a constraints.TokenAutomaton) and constraint_start= constrain the
        rows in the step as generate_ids describes (sample groups are served; num_beams > 1 and prefix_allowed_tokens_fn= raise).  top_logprobs=N / watch_ids=[...] (with return_dict_in_generate; not with
        num_beams > 1): `top_token_ids` / `top_logprobs` [B, T, N] and `watch_logprobs` [B, T, W] of the output, over the RAW logits.
        past_key_values= (the KVHandle in `past_key_values` of an earlier return_dict_in_generate=True call, or of forward(use_cache=True)):
        HF-style multi-turn -- input_ids is the FULL text sequence, the part behind the handle's cached length is appended to the cache (no
        vision, no prefill; at least one id per row, usually the last token of the previous answer); num_beams > 1, num_return_sequences > 1
        and repetition_penalty / no_repeat_ngram_size raise NotImplementedError with it.  The output's `past_key_values` is the handle of what
        this call leaves cached.
        output_hidden_states / output_attentions (with return_dict_in_generate): HF's `hidden_states` / `attentions` of the output -- a tuple over
        the generated tokens, element 0 the prompt pass (a tuple over layers of [B, S, H] / [B, Hq, S, S], the patch rows counting in S), element
        t >= 1 the step that emitted token t ([B, 1, H] / [B, Hq, 1, S + t]); a list per row where rows differ in length; zeros for tokens a
        finished row did not emit.  Served greedy and sampled, with processors, warpers, a constraint and log-probabilities alongside; the ids and
        logits are those of the same call without.  tap_layers=[...] keeps the selected entries only (forward() describes it: all maps of a 7B
        prompt of 768 rows are 2.4 GB, and every step adds 32 x 32 x its context).  num_beams > 1, num_return_sequences > 1 and exact-numerics
        models raise NotImplementedError with them.
        draft_ids= (one list of ids or None per row: typically the ids the previous call generated) runs draft-verified greedy decoding
        (generate_ids describes it): the same sequences in fewer weight passes; `last_draft_stats` holds the call's drafting.DraftStats.
        prompt_lookup_num_tokens=n (HF's keyword) makes each row's own prompt ids its draft, with a window of n + 1.  Greedy only: everything
        generate_ids refuses with a draft raises NotImplementedError before the engine is touched."""
        drafted = draft_ids is not None or prompt_lookup_num_tokens is not None
        if drafted:
            if draft_ids is not None and prompt_lookup_num_tokens is not None:
                raise ValueError("pass one of draft_ids= and prompt_lookup_num_tokens=")
            # what the arguments alone say; sampling, processors / warpers / token rules and the constraint are refused below, from the very objects
            # the call builds for them (whatever keyword made them)
            for k in ("logits_processor", "stopping_criteria", "prefix_allowed_tokens_fn"):
                if kwargs.get(k) is not None:
                    raise NotImplementedError(f"draft-verified decoding is greedy on raw logits: {k}= with a draft is outside the hot path")
            self._check_draft(None, 0, sampling=do_sample or None, beams=((kwargs.get("num_beams") or 1) != 1) or None,
                              num_samples=kwargs.get("num_return_sequences") or 1, scores=(output_scores or output_logits) or None,
                              top=bool(top_logprobs) or bool(watch_ids), taps=bool(output_hidden_states or output_attentions))
        spec = self._tap_args(output_hidden_states and return_dict_in_generate, output_attentions and return_dict_in_generate, tap_layers,
                              kwargs.get("num_beams"), kwargs.get("num_return_sequences") or 1)
        tap_kw = {} if spec is None else {"hidden": spec.hidden or None, "attentions": spec.attn or None}
        n_top, watch = check_top_logprobs(top_logprobs, watch_ids, self.config.llm.vocab_size, "generate")
        want_top = n_top > 0 or len(watch) > 0
        if want_top and not return_dict_in_generate:
            raise ValueError("top_logprobs / watch_ids are returned in the generate output: pass return_dict_in_generate=True")
        cst = self._kw_constraint(kwargs)   # (before the engine is touched: num_beams > 1 and prefix_allowed_tokens_fn raise here)
        rows = self._rows(input_ids, attention_mask)
        cont = {}
        full_rows = rows
        if past_key_values is not None:   # the ids behind what the handle's rows have cached (patch rows are not text)
            self._check_handle(past_key_values, len(rows), "generate")
            if (kwargs.get("num_beams") or 1) != 1:
                raise NotImplementedError("num_beams > 1 with past_key_values is outside the hot path (beams fork their rows from a fresh prefill)")
            if (kwargs.get("num_return_sequences") or 1) != 1:
                raise NotImplementedError("num_return_sequences > 1 with past_key_values is outside the hot path (sample groups fork from a fresh prefill)")
            if (repetition_penalty or 1.0) != 1.0 or (no_repeat_ngram_size or 0) > 0:
                raise NotImplementedError("repetition_penalty / no_repeat_ngram_size with past_key_values are outside the hot path: the processors' id "
                                          "history holds the prompt only, not the cached context")
            if pixel_values is not None or frames_u8 is not None:
                raise ValueError("generate(past_key_values=...) appends text ids to the cached rows: pass no pixel_values / frames_u8 with it")
            cached = [n - past_key_values.n_patches for n in past_key_values.lengths]
            if any(c < 0 or c >= len(r) for c, r in zip(cached, rows)):
                raise ValueError(f"input_ids must be the full text sequence, longer than what the handle has cached ({cached} text ids per row)")
            rows = [r[c:] for c, r in zip(cached, rows)]
            cont = {"continue_from": past_key_values}
        processing = self._processing_args(full_rows, repetition_penalty, no_repeat_ngram_size, min_new_tokens, min_length, **self._kw_rules(kwargs))
        beams = self._beam_args(kwargs.get("num_beams"), kwargs.get("num_return_sequences"), kwargs.get("length_penalty"),
                                kwargs.get("early_stopping"), do_sample, processing, bool(return_dict_in_generate and output_scores))
        if want_top and beams is not None:
            raise NotImplementedError("top_logprobs / watch_ids with num_beams > 1 are outside the hot path (output_logits is served)")
        N = self._sample_group_args(do_sample, kwargs.get("num_beams"), kwargs.get("num_return_sequences"))
        if len(rows) * N > MAX_DECODE_BATCH:
            raise ValueError(f"{len(rows)} prompts x {N} samples exceed the {MAX_DECODE_BATCH} rows of a decode batch")
        sampling = self._sampling_args(do_sample, temperature, top_k, top_p, seed, generator, **self._kw_warpers(kwargs))
        if drafted:   # (before the engine is touched)
            self._check_draft(None, 0, sampling=sampling, processing=processing, constraint=cst.get("constraint"), beams=beams, num_samples=N)
        max_new_tokens = self._max_new(full_rows, max_new_tokens, kwargs.get("max_length"), None)   # (min_length is in `processing`)
        want_sc, want_lg = bool(return_dict_in_generate and output_scores), bool(return_dict_in_generate and output_logits)
        sc = lg = None
        K = beams.num_beams if beams is not None else N
        if want_sc or want_lg:
            eng = self._need_engine()
            shape = (max_new_tokens, len(rows) * K, self.config.llm.vocab_size)
            sc = torch.full(shape, float("nan"), dtype=torch.float32, device=eng.device) if want_sc else None
            lg = torch.full(shape, float("nan"), dtype=torch.float32, device=eng.device) if want_lg else None
        draft_kw = {}
        if drafted:   # (the prompt's own ids as the draft: HF's prompt lookup, with its window)
            from .drafting import DraftParams

            if prompt_lookup_num_tokens is not None:
                if int(prompt_lookup_num_tokens) < 1:
                    raise ValueError(f"prompt_lookup_num_tokens={prompt_lookup_num_tokens} must be at least 1")
                draft_ids, draft_params = [list(r) for r in full_rows], DraftParams(window=int(prompt_lookup_num_tokens) + 1)
            draft_kw = self._draft_kw(draft_ids, len(rows), draft_params)
        res = self.generate_ids(rows, pixel_values, frames_u8, max_new_tokens, sampling=sampling, processing=processing, scores=sc,
                                logits=lg, **self._beam_kw(beams), **self._sample_kw(N), **self._top_kw(n_top, watch), **cst, **cont, **tap_kw, **draft_kw)
        new_ids, lens = res[0], res[1]
        tapped = res[-1] if spec is not None else TapsOutput()
        kvh = None
        if return_dict_in_generate and self.engine is not None:   # what the call left cached: the lengths are read back from the session
            n_pat = past_key_values.n_patches if past_key_values is not None else self.config.n_patches
            kvh = KVHandle(self.engine, self.engine.context_lengths(0, len(rows) * K), n_pat)
        rows = full_rows
        if beams is not None:   # HF's layout: [B * num_return_sequences, P + T], best first per prompt
            R = beams.num_return_sequences
            keep = [g * K + k for g in range(len(rows)) for k in range(R)]
            new_ids, lens = new_ids.cpu()[keep], lens.cpu()[keep].tolist()
            T = max(max(lens), 1)
            P = max(len(r) for r in rows)
            out = torch.full((len(keep), P + T), self.config.pad_token_id, dtype=torch.long)
            for i, r in enumerate(keep):
                seq = rows[r // K] + new_ids[i, : lens[i]].tolist()
                out[i, : len(seq)] = torch.tensor(seq, dtype=torch.long)
            if not return_dict_in_generate:
                return out
            _, _, scores_d, bidx_d = self._need_engine().beam_result()
            Tl = int(torch.isfinite(lg).any(dim=2).any(dim=1).sum()) if want_lg else 0
            return EmmaXGenerateOutput(sequences=out, logits=tuple(lg[t] for t in range(Tl)) if want_lg else None,
                                       sequences_scores=scores_d[:, :R].reshape(-1), beam_indices=bidx_d[:, :R, :T].reshape(len(keep), T),
                                       past_key_values=kvh)
        new_ids, lens = new_ids.cpu(), lens.cpu().tolist()
        T = max(lens)
        P = max(len(r) for r in rows)
        out = torch.full((len(rows) * N, P + T), self.config.pad_token_id, dtype=torch.long)
        for b in range(len(rows) * N):   # (num_return_sequences = N: row b N + j is sample j of prompt b, HF's expand_inputs_for_generation order)
            seq = rows[b // N] + new_ids[b, : lens[b]].tolist()
            out[b, : len(seq)] = torch.tensor(seq, dtype=torch.long)
        if not return_dict_in_generate:
            return out
        top = res[2] if want_top else None
        return EmmaXGenerateOutput(sequences=out, scores=tuple(sc[t] for t in range(T)) if want_sc else None,
                                   logits=tuple(lg[t] for t in range(T)) if want_lg else None,
                                   top_token_ids=top.top_ids[:, :T] if n_top else None, top_logprobs=top.top_logprobs[:, :T] if n_top else None,
                                   watch_logprobs=top.watch_logprobs[:, :T] if watch else None, past_key_values=kvh,
                                   hidden_states=tapped.hidden_states, attentions=tapped.attentions)

    @staticmethod
    def _top_kw(n_top: int, watch) -> Dict[str, Any]:
        """generate_ids' `top_logprobs` / `watch_ids` arguments, passed only when asked for (a plain call is spelled exactly as before)."""
        return {} if not n_top and not watch else {"top_logprobs": n_top, "watch_ids": list(watch) if watch else None}

    def _kw_processing(self, rows, kwargs) -> Optional[LogitsProcessing]:
        """The processor arguments of a **kwargs that the reference forwards to HF generate."""
        return self._processing_args(rows, kwargs.get("repetition_penalty"), kwargs.get("no_repeat_ngram_size"), kwargs.get("min_new_tokens"),
                                     kwargs.get("min_length"), **self._kw_rules(kwargs))

    def _kw_rules(self, kwargs) -> Dict[str, Any]:
        """The token-rule arguments of a **kwargs (HF generate's names), with the EOS id HF filters bad words by."""
        return {"sequence_bias": kwargs.get("sequence_bias"), "bad_words_ids": kwargs.get("bad_words_ids"),
                "suppress_tokens": kwargs.get("suppress_tokens"), "begin_suppress_tokens": kwargs.get("begin_suppress_tokens"),
                "eos_token_id": self.config.eos_token_id}

    @staticmethod
    def _kw_warpers(kwargs) -> Dict[str, Any]:
        """The warper arguments of a **kwargs (HF generate's names)."""
        return {k: kwargs.get(k) for k in ("min_p", "typical_p", "epsilon_cutoff", "eta_cutoff")}

    # ------------------------------------------------------------------------------------------------------------------
    # action APIs
    # ------------------------------------------------------------------------------------------------------------------
    @torch.inference_mode()
    def predict_action(self, input_ids=None, unnorm_key: Optional[str] = None, return_bin_logprobs: bool = False, constrain_to_bins: bool = False,
                       return_hidden_states: bool = False, **kwargs) -> np.ndarray:
        """modeling_prismatic.py:506-537: append 29871 if missing, generate `action_dim` tokens, de-tokenise, un-normalise.
        return_bin_logprobs=True returns (action, fp32 [action_dim, n_action_bins]): at each action token the log-probabilities of the action-bin
        ids, renormalised over the bins, column k = bin k (actions.py: id vocab_size - 1 - k); [N, action_dim, n_action_bins] for a sample
        group.  Not with num_beams > 1.
        constrain_to_bins=True: every one of the `action_dim` tokens is an action-bin id (constraints.action_bins in the decode step; a token
        outside the bins would be mapped to a wrong bin unnoticed).  Also with return_bin_logprobs and num_return_sequences=N; not with
        num_beams > 1.
        return_hidden_states=True: the return gains, as its last element, fp32 [action_dim, H] on the device -- the NORMED last-layer state that
        produced each action token (HF's hidden_states[-1] at the emitting position: what a continuous-action head consumes), written by the
        prompt pass and the decode steps through the session's taps.  Not with num_beams > 1 or num_return_sequences > 1.
        draft_ids= (the ids an earlier call generated for almost the same observation): draft-verified greedy decoding, the same action in
        fewer weight passes (generate_ids: draft); greedy only -- not with sampling, processors, constrain_to_bins, beams or the extras above."""
        draft_kw = self._draft_kw(kwargs.pop("draft_ids", None), 1, kwargs.pop("draft_params", None))
        rows = self._rows(input_ids, kwargs.pop("attention_mask", None))
        if len(rows) != 1:
            raise ValueError("Generation with batch size > 1 is not currently supported!")   # reference contract
        if rows[0][-1] != PREFIX_TOKEN_ID:
            rows[0] = rows[0] + [PREFIX_TOKEN_ID]
        dim = self.get_action_dim(unnorm_key)
        # the reference forwards **kwargs to HF generate (modeling_prismatic.py:519): do_sample / temperature / top_k / top_p are honoured, and
        # num_beams / length_penalty / early_stopping decode the best of the beams (row 0 of the group)
        processing = self._kw_processing(rows, kwargs)
        beams = self._kw_beams(kwargs, processing)
        sampling = self._sampling_args(bool(kwargs.get("do_sample", False)), kwargs.get("temperature"), kwargs.get("top_k"), kwargs.get("top_p"),
                                       kwargs.get("seed"), kwargs.get("generator"), **self._kw_warpers(kwargs))
        N = self._sample_group_args(sampling is not None, kwargs.get("num_beams"), kwargs.get("num_return_sequences"))
        bin_ids = action_bin_token_ids(self.vocab_size, self.config.n_action_bins) if return_bin_logprobs else []
        if return_bin_logprobs and beams is not None:
            raise NotImplementedError("return_bin_logprobs with num_beams > 1 is outside the hot path")
        tap_kw = {}
        if return_hidden_states:
            self._tap_args(True, False, [-1], kwargs.get("num_beams"), N)
            tap_kw = {"hidden": [self.config.llm.num_layers]}
        cst = self._kw_constraint(kwargs)
        if constrain_to_bins:
            if beams is not None:
                raise NotImplementedError("constrain_to_bins with num_beams > 1 is outside the hot path")
            if cst:
                raise ValueError("constrain_to_bins builds its own constraint: pass one of constrain_to_bins= and constraint=")
            cst = {"constraint": self._bin_automaton(dim)}
        res = self.generate_ids(rows, kwargs.get("pixel_values"), kwargs.get("frames_u8"), max_new_tokens=dim, sampling=sampling,
                                processing=processing, **self._beam_kw(beams), **self._sample_kw(N), **self._top_kw(0, bin_ids), **cst, **tap_kw, **draft_kw)
        new_ids, lens = res[0], res[1]
        states = None
        if return_hidden_states:   # element t, its one entry, row 0, the emitting (last) position
            hs = res[-1].hidden_states
            states = torch.stack([hs[t][0][0][-1] for t in range(len(hs))])
            if states.shape[0] < dim:   # (the row stopped early: zeros for what it did not emit)
                states = torch.cat([states, states.new_zeros(dim - states.shape[0], states.shape[1])])

        def action(j):
            got = new_ids[j, : int(lens[j])].cpu().tolist()
            if j == 0:
                self.last_generated_ids = got   # (a caller's next draft_ids: the copy this function makes anyway)
            full = rows[0] + got
            normalized = token_ids_to_actions(np.array(full[-dim:]), self.vocab_size, self.bin_centers)
            return unnormalize(normalized, self.get_action_stats(unnorm_key))

        # do_sample=True with num_return_sequences=N > 1: the N sampled actions of the one observation, [N, action_dim]
        acts = action(0) if N == 1 else np.stack([action(j) for j in range(N)])
        if not return_bin_logprobs:
            return (acts, states) if return_hidden_states else acts
        lp = self.renormalize_logprobs(res[2].watch_logprobs[:, :dim].cpu().numpy())   # [N, dim, n_action_bins]
        return (acts, (lp[0] if N == 1 else lp)) + ((states,) if return_hidden_states else ())

    @staticmethod
    def renormalize_logprobs(lp: np.ndarray) -> np.ndarray:
        """log-probabilities of a subset of the vocabulary -> fp32 log-probabilities over that subset alone (last axis; float64 inside)"""
        x = np.asarray(lp, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            m = np.max(x, axis=-1, keepdims=True)
            return (x - (m + np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True)))).astype(np.float32)

    # ------------------------------------------------------------------------------------------------------------------
    # generate_batch (prismatic/models/vlms/prismatic.py:524-595)
    # ------------------------------------------------------------------------------------------------------------------
    TRIGGER_STRINGS = ["True", "False", "Yes", "No"] + [chr(ord("A") + i) for i in range(26)]

    def string2idx(self, tokenizer=None) -> Dict[str, List[int]]:
        """The reference's trigger strings ("True", "False", "Yes", "No", "A" .. "Z") -> their token ids without special tokens
        (prismatic.py:83-87).  The reference asserts one token each when the model is built; here the rule is enforced on the strings a call
        asks for (generate_batch), since the offline stand-in tokenizer spells every string as several tokens."""
        tok = tokenizer if tokenizer is not None else self.tokenizer
        if tok is None:
            raise ValueError("no tokenizer attached: the checkpoint directory holds no tokenizer files; set model.tokenizer")
        return {s: [int(i) for i in tok.encode(s, add_special_tokens=False)] for s in self.TRIGGER_STRINGS}

    @staticmethod
    def string_probabilities(watch_logprobs_first: np.ndarray) -> List[float]:
        """softmax(first position)[ids] / their sum, from the watched log-probabilities of that position (the lse cancels)"""
        x = np.asarray(watch_logprobs_first, dtype=np.float64)
        p = np.exp(x - np.max(x))
        return (p / p.sum()).tolist()

    @torch.inference_mode()
    def generate_batch(self, pixel_values, texts: List[str], return_string_probabilities: Optional[List[str]] = None, **kwargs):
        """The reference's PrismaticVLM.generate_batch: `pixel_values` is one image ([C, H, W] tensor or {"dino", "siglip"} dict of them) shared by
        every text, or a batch with one image per text; **kwargs go to generate.  Returns the generated texts -- or, with
        return_string_probabilities=[...] (trigger strings of string2idx, one token each), per text the probabilities the FIRST generated
        position gives those strings' tokens, divided by their sum.  The texts run as one batch: each row equals its batch-1 result."""
        tok = kwargs.pop("tokenizer", None)
        tok = tok if tok is not None else self.tokenizer
        if tok is None:
            raise ValueError("no tokenizer attached: the checkpoint directory holds no tokenizer files; set model.tokenizer")
        if isinstance(texts, str) or len(texts) < 1:
            raise ValueError("generate_batch: `texts` is a non-empty list of strings")
        watch: List[int] = []
        if return_string_probabilities is not None:
            table = self.string2idx(tok)
            for st in return_string_probabilities:
                if st not in table:
                    raise ValueError(f'String "{st}" is not one of the trigger strings {self.TRIGGER_STRINGS}')
                if len(table[st]) != 1:
                    raise ValueError(f'String "{st}" is tokenized as more than one token!')
                watch.append(table[st][0])
            if not watch:
                raise ValueError("generate_batch: return_string_probabilities names no string")
        n = len(texts)

        def batch(t):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"Unsupported `pixel_values` type = {type(t)}")
            if t.ndim == 3:
                return t[None].expand(n, *t.shape)
            if t.ndim != 4 or t.shape[0] != n:
                raise ValueError(f"generate_batch: one image for all texts or one per text, got {tuple(t.shape)} for {n} texts")
            return t

        if isinstance(pixel_values, dict):
            pv = {k: batch(v) for k, v in pixel_values.items()}
        else:
            pv = batch(pixel_values)
        rows = [self._rows(tok(t, truncation=True, return_tensors="pt").input_ids)[0] for t in texts]
        if watch:
            out = self.generate(rows, pv, return_dict_in_generate=True, watch_ids=watch, **kwargs)
            first = out.watch_logprobs[:, 0].cpu().numpy()
            return [self.string_probabilities(first[b]) for b in range(n)]
        seqs = self.generate(rows, pv, **kwargs)
        return [tok.decode(seqs[b, len(rows[b]):].tolist(), skip_special_tokens=True).strip() for b in range(n)]

    def _solver(self, tokenizer) -> Solver:
        return Solver(ActionTokenizer(tokenizer, bins=self.config.n_action_bins), verbose=False)

    def _postprocess(self, generated_ids: List[int], tokenizer, type: str = "act"):
        """prismatic.py:666-696: decode -> Solver -> un-normalise."""
        text = tokenizer.decode(generated_ids, skip_special_tokens=True).strip()
        s = self._solver(tokenizer)
        if type == "act":
            actions, _ = s.extract_action_policies(text)
            stats = self.get_action_stats(None)
            return [unnormalize(np.array(a), stats) for a in actions], text
        if type == "pos":
            require_unorm, delta = s.extract_movement_plan(text)
            proprio = delta
            if require_unorm:
                proprio = unnormalize(np.array(delta), self.get_proprio_stats(), "Q1", "Q99")
            return proprio, text
        raise ValueError(f"Unsupported generate_actions type `{type}` (expected 'act' or 'pos')")

    @torch.inference_mode()
    def generate_actions(self, *args, **kwargs):
        """Two call forms, positional or by keyword:
          README   generate_actions(inputs, tokenizer, do_sample=False, max_new_tokens=512) -> (action[7], reasoning)
          native   generate_actions(image, prompt_text, type, **generate_kwargs) -> (list of action[7] | proprio, generated_text)
                   (prismatic/models/vlms/prismatic.py:628; called as `vla.generate_actions(image=image, prompt_text=prompt,
                   type=type, temperature=0.0, max_new_tokens=512, min_length=1, do_sample=False)` by
                   experiments/robot/openvla_utils.py:215-217).  The tokenizer is the model's own (`self.tokenizer`, attached by
                   from_pretrained like the reference's `llm_backbone.tokenizer`); `tokenizer=` overrides it.
        draft_ids= (either form; the ids of an earlier answer, e.g. `last_generated_ids` of the previous control step): draft-verified greedy
        decoding -- the same answer in fewer weight passes (generate_ids: draft).
        """
        args = list(args)
        draft_kw = self._draft_kw(kwargs.pop("draft_ids", None), 1, kwargs.pop("draft_params", None))   # (generate_ids: draft; `last_draft_stats`)
        inputs = kwargs.pop("inputs", None)
        if inputs is None and args and hasattr(args[0], "keys") and "input_ids" in args[0]:
            inputs = args.pop(0)   # dict, our BatchFeature, or transformers.BatchFeature (a UserDict: processing_prismatic.py:216)
        if kwargs.get("do_sample", False):
            raise NotImplementedError("only greedy decoding (do_sample=False) is on the hot path")
        if inputs is not None:   # README form
            tokenizer = args.pop(0) if args else kwargs.pop("tokenizer", None)
            tokenizer = tokenizer if tokenizer is not None else self.tokenizer
            if tokenizer is None:
                raise ValueError("generate_actions(inputs, tokenizer): no tokenizer given and none attached to the model")
            rows = self._rows(inputs["input_ids"], inputs.get("attention_mask"))
            if len(rows) != 1:
                raise ValueError("Generation with batch size > 1 is not currently supported!")
            processing = self._kw_processing(rows, kwargs)
            beams = self._kw_beams(kwargs, processing)   # num_beams > 1: the best hypothesis (row 0 of the group) is decoded
            max_new = self._max_new(rows, kwargs.get("max_new_tokens", None if "max_length" in kwargs else 512), kwargs.get("max_length"), None)
            new_ids, lens = self.generate_ids(rows, inputs.get("pixel_values"), inputs.get("frames_u8"), max_new_tokens=max_new,
                                              processing=processing, **self._beam_kw(beams), **self._kw_constraint(kwargs), **draft_kw)[:2]
            self.last_generated_ids = new_ids[0, : int(lens[0])].cpu().tolist()   # (a caller's next draft_ids)
            actions, text = self._postprocess(self.last_generated_ids, tokenizer, "act")
            return actions[0], text
        # native form
        names = ("image", "prompt_text", "type")
        vals = {}
        for n in names:
            if args:
                if n in kwargs:
                    raise TypeError(f"generate_actions() got multiple values for argument '{n}'")
                vals[n] = args.pop(0)
            elif n in kwargs:
                vals[n] = kwargs.pop(n)
            else:
                raise TypeError(f"generate_actions() missing required argument: '{n}'")
        if args:
            raise TypeError(f"generate_actions() takes 3 positional arguments but {3 + len(args)} were given")
        tokenizer = kwargs.pop("tokenizer", None)
        tokenizer = tokenizer if tokenizer is not None else self.tokenizer
        if tokenizer is None:
            raise ValueError("no tokenizer attached: the checkpoint directory holds no tokenizer files; set model.tokenizer")
        if vals["type"] not in ("act", "pos"):
            raise ValueError(f"Unsupported generate_actions type `{vals['type']}` (expected 'act' or 'pos')")
        enc = tokenizer(vals["prompt_text"], truncation=True, return_tensors="pt")
        rows = self._rows(enc.input_ids)
        processing = self._kw_processing(rows, kwargs)
        beams = self._kw_beams(kwargs, processing)
        max_new = self._max_new(rows, kwargs.get("max_new_tokens"), kwargs.get("max_length"), None)
        feat = self.image_transform(vals["image"])
        new_ids, lens = self.generate_ids(rows, feat["pixel_values"], feat.get("frames_u8"), max_new_tokens=max_new, processing=processing,
                                          **self._beam_kw(beams), **self._kw_constraint(kwargs), **draft_kw)[:2]
        self.last_generated_ids = new_ids[0, : int(lens[0])].cpu().tolist()   # (a caller's next draft_ids)
        return self._postprocess(self.last_generated_ids, tokenizer, vals["type"])

    @torch.inference_mode()
    def generate_actions_batch(self, frames_u8: torch.Tensor, prompt_rows: Sequence[Sequence[int]], max_new_tokens: int = 512,
                               stop_on_eos: bool = True, tokenizer=None, sampling=None, processing=None, beams: Optional[BeamParams] = None,
                               num_samples: int = 1):
        """Batched extension: returns (actions f32 [B,7], new_ids int32 [B,T], lens int32 [B]).

        With `tokenizer` each row goes ids -> text -> Solver exactly like the bs=1 path; without it the ids-level
        stand-in `actions_from_ids` is used (synthetic weights / throughput runs).  `sampling` / `processing`: as generate_ids (None = off).
        `num_samples` = N > 1 (with `sampling`): N sampled rows per frame, all three results with B x N rows (row b N + j = sample j of frame b)."""
        new_ids, lens = self.generate_ids([list(r) for r in prompt_rows], None, frames_u8, max_new_tokens, stop_on_eos, sampling=sampling,
                                          processing=processing, **self._beam_kw(beams), **self._sample_kw(self._check_num_samples(num_samples)))
        if beams is not None:   # the best hypothesis of every prompt
            new_ids, lens = new_ids[:: beams.num_beams].contiguous(), lens[:: beams.num_beams].contiguous()
        ids_h, lens_h = new_ids.cpu(), lens.cpu().tolist()
        acts = np.zeros((len(lens_h), 7), dtype=np.float32)
        stats = self.get_action_stats(None)
        for b, n in enumerate(lens_h):
            row = ids_h[b, :n].tolist()
            if tokenizer is not None:
                a, _ = self._postprocess(row, tokenizer, "act")
                acts[b] = a[0]
            else:
                acts[b] = self.actions_from_ids(row, stats)
        return acts, new_ids, lens

    def actions_from_ids(self, row: List[int], stats: Dict[str, Any]) -> np.ndarray:
        """ids-level stand-in for Solver.extract_action_policies when no tokenizer round trip is wanted (synthetic
        runs / throughput benches): the first 7 ids of the LAST run of >= 7 action-range ids (the policy group is the
        last thing the grammar emits: "...MOVEMENT:\n..\nPOLICIES:\n{tokens}\n"); zeros when there is none, like the
        reference's parse-failure contract.  With a real checkpoint use the tokenizer path (default)."""
        lo = self.vocab_size - self.config.n_action_bins
        runs: List[List[int]] = []
        cur: List[int] = []
        for t in row:
            if lo <= t < self.vocab_size:
                cur.append(t)
            else:
                if cur:
                    runs.append(cur)
                cur = []
        if cur:
            runs.append(cur)
        runs = [r for r in runs if len(r) >= 7]
        if not runs:
            return np.zeros(7, dtype=np.float32)
        seven = runs[-1][:7]
        return unnormalize(token_ids_to_actions(np.array(seven), self.vocab_size, self.bin_centers), stats).astype(np.float32)
