"""
engine.py -- thin Python owner of the libemmax_hip handles: device memory (torch tensors), weight binding, sessions.

PyTorch is used for plumbing only (device allocations, the current HIP stream); every FLOP on the hot path happens in
the hand-written gfx950 kernels behind the C ABI (include/emmax.h).
"""

from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from . import _lib
from .config import EmmaXConfig, check_decode_weight_dtype, decode_weight_code
from .weights import param_shapes, validate_state_dict


def _config_c(cfg: EmmaXConfig) -> _lib.ConfigC:
    c = _lib.ConfigC()
    for i, tw in enumerate(cfg.towers):
        t = c.tower[i]
        t.embed_dim, t.depth, t.num_heads, t.mlp_hidden = tw.embed_dim, tw.depth, tw.num_heads, tw.mlp_hidden
        t.has_cls, t.n_reg, t.layerscale = int(tw.has_cls), tw.n_reg, int(tw.layerscale)
        t.patch, t.image_size, t.take_index = tw.patch, tw.image_size, tw.take_index
        t.ln_eps = tw.ln_eps
        for j in range(3):
            t.mean[j] = tw.mean[j]
            t.std[j] = tw.std[j]
    L = cfg.llm
    c.hidden, c.inter, c.n_layers, c.n_heads, c.n_kv_heads, c.head_dim, c.vocab = (
        L.hidden_size, L.intermediate_size, L.num_layers, L.num_heads, L.num_kv_heads, L.head_dim, L.vocab_size)
    c.rms_eps, c.rope_theta = L.rms_eps, L.rope_theta
    c.bos_id, c.eos_id, c.pad_id = cfg.bos_token_id, cfg.eos_token_id, cfg.pad_token_id
    c.decode_fp8 = decode_weight_code(getattr(cfg, "decode_weight_dtype", "bf16"))
    return c


class _Staged:
    """A staged prefill in flight on the admission stream."""

    def __init__(self, n, event, keep):
        self.n, self.event, self.keep, self.committed = n, event, keep, 0

    def ready(self) -> bool:
        return self.event.query()

    def wait(self) -> None:
        self.event.synchronize()


def _device_bytes(nbytes: int, device, what: str):
    """The weight arenas ("ARENA", "AUX") and the paged KV region ("KV") come from torch's allocator (tools/malloc_flags_probe.py replaces
    this function to measure uncached / fine-grained device memory: no difference, profiles/r05_malloc_flags_ab.txt)."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class EmmaxEngine:
    """Model weights (re-laid-out into one device arena) + one session (workspace + paged KV cache)."""

    def __init__(self, cfg: EmmaXConfig, state_dict: Dict[str, torch.Tensor], device: str = "cuda:0",
                 max_batch: int = 1, max_prompt: int = 512, max_ctx: Optional[int] = None, free_state_dict: bool = False,
                 exact: Optional[bool] = None, mxfp4_wide: Optional[bool] = None):
        if mxfp4_wide and cfg.decode_weight_dtype != "mxfp4":   # (before anything touches the device)
            raise ValueError(f"mxfp4_wide serves MXFP4 decode weights at 17-64 rows: this config has decode_weight_dtype={cfg.decode_weight_dtype!r}")
        self.lib = _lib.load()
        # EXACT NUMERICS (include/emmax.h, tuning switch `exact`): the fp32 CPU arithmetic of the reference instead of bf16 operands.  Frozen into
        # the model at finalize (ViT LayerNorms unfolded) and into every session of this engine; None = what the library's switch says (EMMAX_EXACT)
        # (1 / True: 24-bit K / V cache, the default exact format; 2: fp32 cache, its A/B partner)
        self.exact = int(_lib.tuning_get("exact")) if exact is None else int(exact)
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.EmmaxError("EmmaxEngine needs a HIP device (cuda:N); the product path has no CPU fallback")
        validate_state_dict(state_dict, cfg)
        torch.cuda.set_device(self.device)
        self._model = C.c_void_p()
        self._session = C.c_void_p()
        cc = _config_c(cfg)
        # MXFP4 at 17-64 rows (include/emmax.h, tuning switch `mx4_wide`): read once, at emmax_model_create, and frozen into the model; None = what
        # the library's switch says (EMMAX_MX4_WIDE)
        with _lib.tuning(**({} if mxfp4_wide is None else {"mx4_wide": int(bool(mxfp4_wide))})):
            _lib.check(self.lib.emmax_model_create(C.byref(cc), C.byref(self._model)), "emmax_model_create")
        self.mxfp4_wide = bool(self.lib.emmax_model_mxfp4_wide(self._model) == 1)   # what the model froze
        # ---- bind (bf16, on device) and finalize into the arena ----
        keep: List[torch.Tensor] = []
        for key, shape, _ in param_shapes(cfg):
            t = state_dict[key]
            if t.device != self.device or t.dtype != torch.bfloat16 or not t.is_contiguous():
                t = t.to(device=self.device, dtype=torch.bfloat16).contiguous()
            keep.append(t)
            shp = (C.c_int64 * t.ndim)(*t.shape)
            _lib.check(self.lib.emmax_model_bind_weight(self._model, key.encode(), t.data_ptr(), 0, shp, t.ndim),
                       f"bind {key}")
            if free_state_dict:
                state_dict[key] = None  # drop the caller's copy as soon as ours exists
        nbytes = self.lib.emmax_model_arena_bytes(self._model)
        self.arena = _device_bytes(nbytes, self.device, "ARENA")
        stream = _lib.current_stream()
        import time

        t0 = time.perf_counter()
        with _lib.tuning(exact=int(self.exact)):
            _lib.check(self.lib.emmax_model_finalize(self._model, self.arena.data_ptr(), nbytes, stream), "emmax_model_finalize")
        self.finalize_s = time.perf_counter() - t0     # re-layout of the bound tensors into the arena (synchronous)
        self.aux_build_s = 0.0
        del keep
        self.aux_arena: Optional[torch.Tensor] = None    # the batch >= 3 weight copies, built when a batch >= 3 first decodes
        self.max_batch = self.max_prompt = self.max_ctx = 0
        self._resize_tables: Dict[Tuple[int, int, int], tuple] = {}   # bicubic tables per (H, W, size): resize_frames
        self._adm_stream = None     # the admission stream and the last commit on the decode stream: admission
        self._commit_event = None
        self.new_session(max_batch, max_prompt, max_ctx)

    # ------------------------------------------------------------------------------------------------------------------
    def new_session(self, max_batch: int, max_prompt: int, max_ctx: Optional[int] = None, stage_rows: int = 0) -> None:
        """(Re)create the session.  `stage_rows` staging rows (overlapped slot admissions, include/emmax.h) cost per-row state and
        their share of the paged KV region: only slot serving asks for them (ensure_stage_rows)."""
        if self._session:
            self.lib.emmax_session_destroy(self._session)
            self._session = C.c_void_p()
        np_ = self.cfg.n_patches
        if max_ctx is None:
            max_ctx = np_ + max_prompt + 512 + 1
        ws, kv = C.c_int64(), C.c_int64()
        with _lib.tuning(exact=int(self.exact)):   # the session kind (and the KV format) is read when the session is sized and created
            _lib.check(self.lib.emmax_session_bytes_ex(self._model, max_batch, max_prompt, max_ctx, int(stage_rows), C.byref(ws), C.byref(kv)),
                       "emmax_session_bytes_ex")
            self.workspace = torch.empty(ws.value, dtype=torch.uint8, device=self.device)
            self.kv = _device_bytes(kv.value, self.device, "KV")
            _lib.check(self.lib.emmax_session_create_ex(self._model, max_batch, max_prompt, max_ctx, int(stage_rows), self.workspace.data_ptr(),
                                                        ws.value, self.kv.data_ptr(), kv.value, C.byref(self._session)),
                       "emmax_session_create_ex")
        assert bool(self.lib.emmax_session_exact(self._session)) == bool(self.exact)
        self._score_bufs = None   # a new session binds no scores
        self._top_bufs = None     # ... and no top / watched log-probability buffers
        self._tap_bufs = None     # ... and no taps
        self._beam_K = 0          # ... and has beams off
        self._group_N = 0         # ... and sample groups off
        self.session_epoch = getattr(self, "session_epoch", 0) + 1   # which session a KV handle names (modeling.KVHandle)
        self.max_batch, self.max_prompt, self.max_ctx, self.stage_rows = max_batch, max_prompt, max_ctx, int(stage_rows)

    def ensure_stage_rows(self, n: int) -> None:
        """Slot serving with overlapped admission stages up to `n` requests at a time: re-create the session with that many staging
        rows if it has fewer (drops any state of the current session -- call before slots_open)."""
        if n > self.stage_rows:
            # staging rows are bounded by the decode batch: grow that first, so that n_slots > max_batch surfaces as what it is
            self.new_session(max(self.max_batch, int(n)), self.max_prompt, self.max_ctx, stage_rows=int(n))

    def ensure_decode_batch(self, batch: int) -> None:
        """Decode batches >= 3 read MFMA-fragment-major weight copies that live in a second arena (include/emmax.h:
        emmax_model_build_aux); a model that only ever serves batches 1-2 never pays for them (13 GB at 7B)."""
        if batch < 3 or self.aux_arena is not None:
            return
        n = int(self.lib.emmax_model_aux_bytes(self._model))
        import time

        t0 = time.perf_counter()
        self.aux_arena = _device_bytes(max(n, 256), self.device, "AUX")
        _lib.check(self.lib.emmax_model_build_aux(self._model, self.aux_arena.data_ptr(), n, _lib.current_stream()), "emmax_model_build_aux")
        self.aux_build_s = time.perf_counter() - t0

    @property
    def patch_dtype(self) -> torch.dtype:
        """Element type of the patch embeddings the session hands out and takes back: bf16, fp32 in exact numerics (include/emmax.h)."""
        return torch.float32 if self.exact else torch.bfloat16

    def max_decode_batch(self) -> int:
        """Rows of one decode batch this model can run (64 for LLaMA-2-7B shapes, 8 for shapes outside the K-split kernels; MXFP4 / MXFP6 weights: 16, or 8
        when nine rows would split the attention; MXFP4 created with mxfp4_wide: up to 64).  Exact numerics: the two-term kernels take 8 rows per launch and larger batches run in chunks
        of 8 -- 64 on the shapes those kernels take, 2 where only the batch 1-2 kernel does."""
        if self.exact:
            return int(self.lib.emmax_model_max_decode_batch_exact(self._model))
        return int(self.lib.emmax_model_max_decode_batch(self._model))

    def weight_bytes(self) -> int:
        return int(self.arena.numel()) + (int(self.aux_arena.numel()) if self.aux_arena is not None else 0)

    def ensure_capacity(self, batch: int, prompt: int, max_new: int) -> None:
        need_ctx = self.cfg.n_patches + prompt + max_new + 1
        if batch > self.max_batch or prompt > self.max_prompt or need_ctx > self.max_ctx:
            self.new_session(max(batch, self.max_batch), max(prompt, self.max_prompt), max(need_ctx, self.max_ctx),
                             stage_rows=self.stage_rows)

    def close(self) -> None:
        if getattr(self, "_session", None):
            self.lib.emmax_session_destroy(self._session)
            self._session = C.c_void_p()
        if getattr(self, "_model", None):
            self.lib.emmax_model_destroy(self._model)
            self._model = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------------
    def vision_encode(self, frames_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B,224,224,3] on device -> [B,256,hidden] projected patch embeddings (bf16; fp32 in an exact-numerics session: `patch_dtype`)."""
        assert frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.is_contiguous()
        frames_u8 = self.resize_frames(frames_u8)   # no-op at the native 224x224
        B = frames_u8.shape[0]
        out = torch.empty(B, self.cfg.n_patches, self.cfg.llm.hidden_size, dtype=self.patch_dtype, device=self.device)
        _lib.check(self.lib.emmax_vision_encode(self._session, frames_u8.data_ptr(), B, out.data_ptr(), _lib.current_stream()),
                   "emmax_vision_encode")
        return out

    def resize_frames(self, frames_u8: torch.Tensor, size: Optional[int] = None) -> torch.Tensor:
        """uint8 [B,H,W,3] on device -> uint8 [B,size,size,3], bit-exact with PIL.Image.resize(BICUBIC) (resize-naive)."""
        from .resize import bicubic_coeffs

        size = size or self.cfg.towers[0].image_size
        B, H, W, _ = frames_u8.shape
        if H == size and W == size:
            return frames_u8
        assert frames_u8.dtype == torch.uint8 and frames_u8.is_cuda and frames_u8.is_contiguous()
        key = (H, W, size)
        if key not in self._resize_tables:
            bh, kh, nh = bicubic_coeffs(W, size)
            bv, kv, nv = bicubic_coeffs(H, size)
            self._resize_tables[key] = tuple(torch.from_numpy(a.copy()).to(self.device) for a in (bh, kh, bv, kv)) + (nh, nv)
        bh, kh, bv, kv, nh, nv = self._resize_tables[key]
        out = torch.empty(B, size, size, 3, dtype=torch.uint8, device=self.device)
        tmp = torch.empty(B, H, size, 3, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.emmax_op_resize_bicubic_u8(frames_u8.data_ptr(), B, H, W, out.data_ptr(), size, size, tmp.data_ptr(),
                                                       bh.data_ptr(), kh.data_ptr(), nh, bv.data_ptr(), kv.data_ptr(), nv,
                                                       _lib.current_stream()), "emmax_op_resize_bicubic_u8")
        return out

    def vision_encode_pixels(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """bf16 [B,6,224,224] (PrismaticProcessor layout) -> bf16 [B,256,hidden]."""
        pv = pixel_values.to(device=self.device, dtype=torch.bfloat16).contiguous()
        B = pv.shape[0]
        out = torch.empty(B, self.cfg.n_patches, self.cfg.llm.hidden_size, dtype=self.patch_dtype, device=self.device)
        _lib.check(self.lib.emmax_vision_encode_pixels(self._session, pv.data_ptr(), B, out.data_ptr(), _lib.current_stream()),
                   "emmax_vision_encode_pixels")
        return out

    def vision_features(self, B: int) -> torch.Tensor:
        out = torch.empty(B, self.cfg.n_patches, self.cfg.vision_dim, dtype=torch.bfloat16, device=self.device)
        _lib.check(self.lib.emmax_vision_features(self._session, B, out.data_ptr(), _lib.current_stream()), "emmax_vision_features")
        return out

    def _pack_prompts(self, who: str, prompts: Sequence[Sequence[int]], pad: int, patch_embeds: Optional[Sequence[torch.Tensor]] = None):
        """Ragged prompts as one int32 [n, P_max] device tensor padded with `pad`, their lengths and P_max; `patch_embeds` (one tensor per
        prompt) stacked into one [n, n_patches, hidden] tensor, else None."""
        lens = [len(p) for p in prompts]
        P_max = max(lens)
        ids = torch.full((len(prompts), P_max), pad, dtype=torch.int32)
        for i, p in enumerate(prompts):
            ids[i, : lens[i]] = torch.as_tensor(list(p), dtype=torch.int32)
        pe = None
        if patch_embeds is not None:
            if len(patch_embeds) != len(prompts):
                raise ValueError(f"{who}: one patch-embedding tensor per prompt")
            pe = torch.stack([t.reshape(self.cfg.n_patches, self.cfg.llm.hidden_size) for t in patch_embeds]).contiguous()
            assert pe.dtype == self.patch_dtype
        return ids.to(self.device), lens, P_max, pe

    def prefill(self, input_ids: Sequence[Sequence[int]], patch_embeds: torch.Tensor) -> List[int]:
        """Ragged prompts (row b = list of ids starting with BOS). Returns per-row packed lengths S_b = 256 + P_b."""
        B = len(input_ids)
        K = self._beam_K
        N = self._group_N or 1
        self.ensure_decode_batch(B * (K or N))   # beams / sample groups on: B groups decode as B x K / B x N rows
        ids_d, lens, P_max, _ = self._pack_prompts("prefill", input_ids, self.cfg.pad_token_id)
        lens_c = (C.c_int32 * B)(*lens)
        if patch_embeds is None:   # language-only forward
            _lib.check(self.lib.emmax_prefill_text(self._session, ids_d.data_ptr(), lens_c, B, P_max, _lib.current_stream()),
                       "emmax_prefill_text")
            self._last_S = list(lens)
            self._last_B = B * N
            return self._last_S
        pe = patch_embeds.contiguous()
        assert pe.dtype == self.patch_dtype and pe.shape[0] == B
        _lib.check(self.lib.emmax_prefill(self._session, ids_d.data_ptr(), lens_c, B, P_max, pe.data_ptr(), _lib.current_stream()),
                   "emmax_prefill")
        self._last_S = [self.cfg.n_patches + n for n in lens]
        self._last_B = B * N   # (sample groups: the prefill forked the B prompts into B x N rows; everything after it sees that batch)
        return self._last_S

    def prefill_logits(self) -> List[torch.Tensor]:
        """f32 logits of every prefill position, one [S_b, vocab] tensor per row."""
        total = sum(self._last_S)
        out = torch.empty(total, self.cfg.llm.vocab_size, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.emmax_prefill_logits(self._session, out.data_ptr(), _lib.current_stream()), "emmax_prefill_logits")
        return list(torch.split(out, self._last_S, dim=0))

    def score(self, targets: Sequence[Sequence[int]]):
        """The rows prefill_logits would return, scored without their logits (include/emmax.h: emmax_prefill_score).  targets: per row of the
        last pass one id per position (-100 = not scored), aligned as the pass packed its rows.  -> (lse, target_logit, argmax): lists of
        per-row device tensors, fp32 / fp32 / int32 [S_b]; target_logit is 0 where the target is -100."""
        if self.exact:
            raise NotImplementedError("score: exact-numerics models are not scored (the scoring kernel has no two-term form)")
        if [len(t) for t in targets] != list(self._last_S):
            raise ValueError(f"score: targets of lengths {[len(t) for t in targets]} for rows of lengths {list(self._last_S)}")
        total = sum(self._last_S)
        tg = torch.tensor([int(x) for t in targets for x in t], dtype=torch.int32).to(self.device)
        out = torch.empty(3, total, dtype=torch.float32, device=self.device)   # lse | target logit | argmax (int32 bits)
        _lib.check(self.lib.emmax_prefill_score(self._session, tg.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _lib.current_stream()),
                   "emmax_prefill_score")
        return tuple(list(torch.split(x, self._last_S)) for x in (out[0], out[1], out[2].view(torch.int32)))

    def last_logits(self) -> torch.Tensor:
        out = torch.empty(self._last_B, self.cfg.llm.vocab_size, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.emmax_last_logits(self._session, out.data_ptr(), _lib.current_stream()), "emmax_last_logits")
        return out

    def decode_step(self) -> None:
        _lib.check(self.lib.emmax_decode_step(self._session, _lib.current_stream()), "emmax_decode_step")

    def set_current_tokens(self, toks: Sequence[int]) -> None:
        t = torch.as_tensor(list(toks), dtype=torch.int32).to(self.device)
        _lib.check(self.lib.emmax_set_current_tokens(self._session, t.data_ptr(), _lib.current_stream()), "emmax_set_current_tokens")
        torch.cuda.current_stream().synchronize()   # `t` must outlive the copy

    def generate(self, max_new_tokens: int, stop_on_eos: bool = True, return_logprobs: bool = False):
        """The decode loop after prefill: greedy, or sampled per row once set_sampling ran.  Returns (ids int32 [B,max_new] padded with pad_id,
        lens int32 [B]) on device; with return_logprobs (sampling on only) also the fp32 [B,max_new] log-probabilities of the emitted tokens.
        Beams on: B = groups x num_beams rows, row g K + k = the k-th best kept hypothesis of group g (beam_result has the scores)."""
        B = self._last_B * (self._beam_K or 1)
        self._beam_T = int(max_new_tokens)
        out = torch.empty(B, max_new_tokens, dtype=torch.int32, device=self.device)
        lens = torch.empty(B, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.emmax_generate(self._session, max_new_tokens, int(stop_on_eos), out.data_ptr(), lens.data_ptr(),
                                           _lib.current_stream()), "emmax_generate")
        if not return_logprobs:
            return out, lens
        lp = torch.empty(B, max_new_tokens, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.emmax_session_logprobs(self._session, max_new_tokens, lp.data_ptr(), _lib.current_stream()), "emmax_session_logprobs")
        return out, lens, lp

    # ---- extending a cached context (include/emmax.h: emmax_extend) ----------------------------------------------------------
    def _check_extension_fits(self, who: str, n_rows: int, longest: int) -> None:
        """A continuation must never re-create the session (that would drop the very cache it extends): what ensure_capacity would grow is an error."""
        if n_rows > self.max_batch or longest * n_rows > self.max_batch * (self.cfg.n_patches + self.max_prompt):
            raise _lib.EmmaxError(
                f"{who}: {n_rows} rows of up to {longest} new ids exceed the session's prefill capacity (max_batch {self.max_batch} x "
                f"(n_patches + max_prompt {self.max_prompt}) packed rows); a continuation cannot re-create the session -- create it larger "
                f"(max_prompt / cache_reserve / max_ctx) before the first prefill")

    def extend(self, rows: Sequence[Sequence[int]], row0: int = 0, max_new_tokens: int = 0) -> List[int]:
        """Append the ids rows[b] (>= 1 each) to the cached context of live rows row0 .. row0 + len(rows) - 1 -- after a prefill and any number of
        decode steps -- in one pass over the new rows alone.  A row's pending token (picked, not yet cached) is dropped: pass it as the first id
        to keep it.  Afterwards the rows are as a prefill leaves them (first token of the continuation picked; `generate` continues), and
        prefill_logits() returns the new rows' logits.  max_new_tokens: what will be generated next, for the capacity check (a context beyond
        max_ctx is refused: it is fixed when the session is created).  Returns the rows' new cached lengths."""
        rows = [list(r) for r in rows]
        B = len(rows)
        self._check_extension_fits("extend", B, max(len(r) for r in rows))
        ids_d, lens, P_max, _ = self._pack_prompts("extend", rows, self.cfg.pad_token_id)
        lens_c = (C.c_int32 * B)(*lens)
        _lib.check(self.lib.emmax_extend(self._session, int(row0), B, ids_d.data_ptr(), lens_c, P_max, int(max_new_tokens), _lib.current_stream()),
                   "emmax_extend")
        torch.cuda.current_stream().synchronize()   # `ids_d` must outlive the pass
        self._last_S = list(lens)   # what prefill_logits splits by: the new rows
        return self.context_lengths(int(row0), B)

    def slot_extend(self, slot: int, ids: Sequence[int], max_new_tokens: int) -> None:
        """A follow-up on the context a FINISHED request left in `slot` (done, not released): its ids are appended in one pass, the first token
        of the answer is in place afterwards and the slot decodes again with the new budget.  The other slots are untouched."""
        ids = list(ids)
        self._check_extension_fits("slot_extend", 1, len(ids))
        ids_d = torch.as_tensor(ids, dtype=torch.int32).to(self.device)
        _lib.check(self.lib.emmax_slot_extend(self._session, int(slot), ids_d.data_ptr(), len(ids), int(max_new_tokens), _lib.current_stream()),
                   "emmax_slot_extend")
        torch.cuda.current_stream().synchronize()   # `ids_d` must outlive the pass
        self._last_S = [len(ids)]   # what prefill_logits splits by: the slot's new rows

    def context_lengths(self, row0: int = 0, n: Optional[int] = None) -> List[int]:
        """The cached lengths of rows row0 .. row0 + n - 1 (default: the live batch), read back from the device."""
        n = self._last_B if n is None else int(n)
        out = (C.c_int32 * n)()
        _lib.check(self.lib.emmax_session_context(self._session, int(row0), n, out, _lib.current_stream()), "emmax_session_context")
        return list(out)

    # ---- draft-verified greedy decoding (include/emmax.h: emmax_verify; drafting.py holds the policy and the loop) ---------------
    def verify(self, windows: Sequence[Sequence[int]], row0: int = 0, max_new: Optional[int] = None):
        """One verify pass over live rows row0 .. in mid-generation: windows[b] = the row's pending token, then guessed ids.  Every row emits the
        model's own greedy tokens as far as the guess agrees with them (1 .. len(windows[b]) tokens; a done row none) and is then as that many
        decode steps would have left it.  max_new: the rows' token budget (default: the session's output row, max_ctx ids).
        -> (emitted, new_ids, done): per row the count, the emitted ids and the done flag.  drafting.VerifyRefused when the windows do not fit
        the rows' cache (nothing changed: fall back to decode_step); prefill_logits() returns the window rows' logits afterwards."""
        from .drafting import VerifyRefused

        windows = [list(w) for w in windows]
        B = len(windows)
        self._check_extension_fits("verify", B, max(len(w) for w in windows))
        ids_d, lens, P_max, _ = self._pack_prompts("verify", windows, self.cfg.pad_token_id)
        lens_c = (C.c_int32 * B)(*lens)
        emitted, done, new_ids = (C.c_int32 * B)(), (C.c_int32 * B)(), (C.c_int32 * (B * P_max))()
        rc = self.lib.emmax_verify(self._session, int(row0), B, ids_d.data_ptr(), lens_c, P_max, int(max_new if max_new is not None else self.max_ctx),
                                   emitted, new_ids, done, _lib.current_stream())
        if rc == -3:   # EMMAX_ERR_NOMEM
            raise VerifyRefused(self.lib.emmax_last_error().decode("utf-8", "replace"))
        _lib.check(rc, "emmax_verify")
        self._last_S = list(lens)   # what prefill_logits splits by: the window rows
        return list(emitted), [list(new_ids[b * P_max:b * P_max + emitted[b]]) for b in range(B)], list(done)

    def set_budget(self, max_new: int, row0: int = 0, n: Optional[int] = None) -> None:
        """The token budget of live rows row0 .. row0 + n - 1, as generate sets it before its loop: for a host loop of decode_step / verify."""
        n = self._last_B if n is None else int(n)
        _lib.check(self.lib.emmax_session_set_budget(self._session, int(row0), n, int(max_new), _lib.current_stream()), "emmax_session_set_budget")

    def output_tail(self, first: int, n: int, row0: int = 0, rows: Optional[int] = None):
        """Generated ids first .. first + n - 1 of live rows row0 .. (pad where a row has none), their counts and done flags, read back to the host."""
        B = self._last_B if rows is None else int(rows)
        ids, n_out, done = (C.c_int32 * (B * n))(), (C.c_int32 * B)(), (C.c_int32 * B)()
        _lib.check(self.lib.emmax_session_output(self._session, int(row0), B, int(first), int(n), ids, n_out, done, _lib.current_stream()), "emmax_session_output")
        return [list(ids[b * n:(b + 1) * n]) for b in range(B)], list(n_out), list(done)

    # ---- taps: hidden states and attention maps out of the passes (include/emmax.h: emmax_session_set_pass_taps) ---------------
    def _tap_refusals(self, who: str) -> None:
        if self.exact:
            raise NotImplementedError(f"{who}: exact-numerics models serve no hidden states / attention maps (their fp32 cache has no probability kernel)")

    def _tap_buffers(self, shapes, zero: bool):
        make = torch.zeros if zero else torch.empty
        return tuple(make(sh, dtype=torch.float32, device=self.device) if sh is not None else None for sh in shapes)

    def bind_pass_taps(self, spec, total_rows: int, max_keys: int):
        """Bind fp32 buffers that the NEXT prefill or extend fills over its `total_rows` packed rows (taps.TapSpec; taps.pass_shapes) and that are
        unbound behind it: (hidden [n_sel, total_rows, H] or None, attentions [n_sel, total_rows, Hq, ld_keys] or None).  max_keys: the keys
        the longest row of the pass sees.  The kernel writes every entry of every row: the buffers are not cleared."""
        from . import taps as T

        self._tap_refusals("bind_pass_taps")
        ld = T.round_keys(max_keys)
        hid, att = self._tap_buffers(T.pass_shapes(spec, int(total_rows), self.cfg.llm.hidden_size, self.cfg.llm.num_heads, ld), zero=False)
        _lib.check(self.lib.emmax_session_set_pass_taps(self._session, _lib.ptr(hid), T.layer_mask(spec.hidden), _lib.ptr(att), T.layer_mask(spec.attn), ld,
                                                        _lib.current_stream()), "emmax_session_set_pass_taps")
        self._tap_bufs = (hid, att)
        return hid, att

    def bind_step_taps(self, spec, max_new: int, max_keys: int):
        """Bind zeroed fp32 buffers that every decode step from now on fills at each row's generation index (after a prefill or extend; unbound
        by the next one or by clear_taps): (hidden [max_new, n_sel, B, H] or None, attentions [max_new, n_sel, B, Hq, ld_keys] or None), B
        the live batch.  Slot 0 is the prompt pass's and stays zero, as do the slots of tokens a finished row did not emit; max_new = 1 is the
        single-step form (every row lands in slot 0).  max_keys: the keys the longest row sees in its last step."""
        from . import taps as T

        self._tap_refusals("bind_step_taps")
        ld = T.round_keys(max_keys)
        hid, att = self._tap_buffers(T.step_shapes(spec, int(max_new), self._last_B, self.cfg.llm.hidden_size, self.cfg.llm.num_heads, ld), zero=True)
        _lib.check(self.lib.emmax_session_set_step_taps(self._session, _lib.ptr(hid), T.layer_mask(spec.hidden), _lib.ptr(att), T.layer_mask(spec.attn), ld,
                                                        int(max_new), _lib.current_stream()), "emmax_session_set_step_taps")
        self._tap_bufs = (hid, att)
        return hid, att

    def clear_taps(self) -> None:
        """Unbind: the session launches what it launched before, and the buffers are the caller's."""
        _lib.check(self.lib.emmax_session_clear_taps(self._session, _lib.current_stream()), "emmax_session_clear_taps")
        self._tap_bufs = None

    @property
    def taps_bound(self) -> int:
        """bit 0: pass taps, bit 1: step taps"""
        return max(int(self.lib.emmax_session_taps(self._session)), 0)

    # ---- sampling inside the decode step (include/emmax.h, ABI 7) -------------------------------------------------------
    @staticmethod
    def _sampling_arrays(params, seeds, subseqs, n: Optional[int] = None, generator=None):
        """Host arrays (temperature, top_k, top_p, seed, subseq) of len(params) rows: one SamplingParams for all rows needs `n`.  Seeds default
        to each SamplingParams.seed, else draw_seed(generator); subseqs default to the row index."""
        from .sampling import SamplingParams, _per_row, draw_seed

        ps = _per_row(params, n if n is not None else (len(params) if isinstance(params, (list, tuple)) else 1), "params")
        if not all(isinstance(p, SamplingParams) for p in ps):
            raise ValueError("set_sampling: params must be SamplingParams")
        k = len(ps)
        if seeds is None:
            seeds = [p.seed if p.seed is not None else draw_seed(generator) for p in ps]
        seeds = [int(x) & ((1 << 64) - 1) for x in _per_row(seeds, k, "seeds")]
        subseqs = list(range(k)) if subseqs is None else [int(x) & 0xFFFFFFFF for x in _per_row(subseqs, k, "subseqs")]
        return (k, (C.c_float * k)(*[float(p.temperature) for p in ps]), (C.c_int32 * k)(*[int(p.top_k) for p in ps]),
                (C.c_float * k)(*[float(p.top_p) for p in ps]), (C.c_uint64 * k)(*seeds), (C.c_uint32 * k)(*subseqs))

    def set_sampling(self, params, seeds=None, subseqs=None, row0: int = 0, n: Optional[int] = None, generator=None) -> None:
        """Sample rows row0.. in the decode step from now on (turns sampling on): one SamplingParams per row (or one for `n` rows), seeds
        (default: each params' seed, else drawn from `generator`), subseqs (default: 0, 1, ... in row order).  Precedes the prefill whose
        first token it governs."""
        k, T, tk, tp, sd, sb = self._sampling_arrays(params, seeds, subseqs, n, generator)
        _lib.check(self.lib.emmax_session_set_sampling(self._session, int(row0), k, T, tk, tp, sd, sb, _lib.current_stream()),
                   "emmax_session_set_sampling")

    def set_sampling_staged(self, params, seeds=None, subseqs=None, n: Optional[int] = None, generator=None) -> None:
        """set_sampling for the requests of the next slots_prefill_staged (call inside `with engine.admission():`, before it)."""
        k, T, tk, tp, sd, sb = self._sampling_arrays(params, seeds, subseqs, n, generator)
        _lib.check(self.lib.emmax_slots_set_sampling_staged(self._session, k, T, tk, tp, sd, sb, _lib.current_stream()),
                   "emmax_slots_set_sampling_staged")

    def clear_sampling(self) -> None:
        """Greedy again: the session launches exactly the kernels of one that never sampled."""
        _lib.check(self.lib.emmax_session_clear_sampling(self._session, _lib.current_stream()), "emmax_session_clear_sampling")
        self._drop_unbound_top()

    @property
    def sampling(self) -> bool:
        return self.lib.emmax_session_sampling(self._session) == 1

    # ---- logits processors and scores inside the decode step (include/emmax.h, ABI 8) --------------------------------------
    @staticmethod
    def _processing_arrays(params, n: Optional[int] = None):
        """Host arrays (penalty, ngram, min_new) of len(params) rows: one LogitsProcessing for all rows needs `n`."""
        from .sampling import LogitsProcessing, _per_row

        ps = _per_row(params, n if n is not None else (len(params) if isinstance(params, (list, tuple)) else 1), "processing")
        if not all(isinstance(p, LogitsProcessing) for p in ps):
            raise ValueError("set_processing: params must be LogitsProcessing")
        k = len(ps)
        return (k, (C.c_float * k)(*[float(p.repetition_penalty) for p in ps]), (C.c_int32 * k)(*[int(p.no_repeat_ngram_size) for p in ps]),
                (C.c_int32 * k)(*[int(p.min_new_tokens) for p in ps]))

    def set_processing(self, params, row0: int = 0, n: Optional[int] = None) -> None:
        """Apply the logits processors to rows row0.. in the decode step from now on (turns processing on): one LogitsProcessing per row
        (or one for `n` rows).  Precedes the prefill whose tokens it governs (the prefill keeps the rows' prompt ids)."""
        k, pen, ng, mn = self._processing_arrays(params, n)
        _lib.check(self.lib.emmax_session_set_processing(self._session, int(row0), k, pen, ng, mn, _lib.current_stream()),
                   "emmax_session_set_processing")

    def set_processing_staged(self, params, n: Optional[int] = None) -> None:
        """set_processing for the requests of the next slots_prefill_staged (call inside `with engine.admission():`, before it)."""
        k, pen, ng, mn = self._processing_arrays(params, n)
        _lib.check(self.lib.emmax_slots_set_processing_staged(self._session, k, pen, ng, mn, _lib.current_stream()),
                   "emmax_slots_set_processing_staged")

    def clear_processing(self) -> None:
        """Processing off: with scores unbound and sampling off the session launches exactly what a greedy session launches."""
        _lib.check(self.lib.emmax_session_clear_processing(self._session, _lib.current_stream()), "emmax_session_clear_processing")
        self._drop_unbound_top()

    @property
    def processing(self) -> bool:
        return self.lib.emmax_session_processing(self._session) == 1

    # ---- the further warpers and the token rules (include/emmax.h: emmax_session_set_warpers / emmax_session_set_token_rules) ----------
    @staticmethod
    def _warper_arrays(params, n: Optional[int] = None):
        """Host arrays (min_p, typical_p, epsilon_cutoff, eta_cutoff; 0 = off) of len(params) rows: one SamplingParams for all rows needs `n`."""
        from .sampling import SamplingParams, _per_row

        ps = _per_row(params, n if n is not None else (len(params) if isinstance(params, (list, tuple)) else 1), "params")
        if not all(isinstance(p, SamplingParams) for p in ps):
            raise ValueError("set_warpers: params must be SamplingParams")
        k = len(ps)
        return (k,) + tuple((C.c_float * k)(*[p.warpers[j] for p in ps]) for j in range(4))

    def set_warpers(self, params, row0: int = 0, n: Optional[int] = None) -> None:
        """min_p / typical_p / epsilon_cutoff / eta_cutoff of rows row0.. from their SamplingParams (turns the warpers on: the step ends in
        the EXT finish).  set_sampling leaves them alone; clear_sampling and clear_warpers turn them off."""
        k, mp, ty, ep, et = self._warper_arrays(params, n)
        _lib.check(self.lib.emmax_session_set_warpers(self._session, int(row0), k, mp, ty, ep, et, _lib.current_stream()), "emmax_session_set_warpers")

    def set_warpers_staged(self, params, n: Optional[int] = None) -> None:
        """set_warpers for the requests of the next slots_prefill_staged."""
        k, mp, ty, ep, et = self._warper_arrays(params, n)
        _lib.check(self.lib.emmax_slots_set_warpers_staged(self._session, k, mp, ty, ep, et, _lib.current_stream()), "emmax_slots_set_warpers_staged")

    def clear_warpers(self) -> None:
        _lib.check(self.lib.emmax_session_clear_warpers(self._session, _lib.current_stream()), "emmax_session_clear_warpers")

    @property
    def warpers(self) -> bool:
        return self.lib.emmax_session_warpers(self._session) == 1

    def set_token_rules(self, params, row0: int = 0, n: Optional[int] = None, enables: bool = True) -> None:
        """The session's rule table (sequence_bias / bad_words_ids / suppress_tokens / begin_suppress_tokens) from the LogitsProcessing of rows
        row0.. (one per row, or one for `n` rows), and those rows' enable words.  The rows that name a kind name the same rules.  Turns
        processing on with neutral values where it was off (the rules read the history); params without rules clear the table.
        enables=False: the table alone (a serve sets each request's word at its admission)."""
        from .sampling import _per_row, rule_table

        ps = _per_row(params, n if n is not None else (len(params) if isinstance(params, (list, tuple)) else 1), "processing")
        t = rule_table(ps)
        if t is None:
            return self.clear_token_rules()
        off, ids, flags, bias, en = t
        R = len(flags)
        _lib.check(self.lib.emmax_session_set_token_rules(self._session, R, (C.c_int32 * (R + 1))(*off), (C.c_int32 * len(ids))(*ids), (C.c_int32 * R)(*flags),
                                                          (C.c_float * R)(*bias), _lib.current_stream()), "emmax_session_set_token_rules")
        if enables:
            self.set_rule_enables(en, row0)

    def set_rule_enables(self, words, row0: int = 0) -> None:
        """Rows row0..: which kinds of the session's rules apply (bit 0 sequence_bias, 1 bad_words_ids, 2 suppress_tokens, 3 begin_suppress_tokens)."""
        k = len(words)
        _lib.check(self.lib.emmax_session_set_rule_enables(self._session, int(row0), k, (C.c_uint32 * k)(*[int(w) for w in words]), _lib.current_stream()),
                   "emmax_session_set_rule_enables")

    def set_rule_enables_staged(self, words) -> None:
        """set_rule_enables for the requests of the next slots_prefill_staged."""
        k = len(words)
        _lib.check(self.lib.emmax_slots_set_rule_enables_staged(self._session, k, (C.c_uint32 * k)(*[int(w) for w in words]), _lib.current_stream()),
                   "emmax_slots_set_rule_enables_staged")

    def clear_token_rules(self) -> None:
        _lib.check(self.lib.emmax_session_clear_token_rules(self._session, _lib.current_stream()), "emmax_session_clear_token_rules")
        self._drop_unbound_top()

    @property
    def token_rules(self) -> bool:
        return self.lib.emmax_session_token_rules(self._session) == 1

    # ---- constrained decoding: a token automaton in the decode step (include/emmax.h: emmax_session_set_automaton) ----------------
    def set_automaton(self, automaton) -> None:
        """The session's token automaton (constraints.TokenAutomaton; turns processing on with neutral values where it was off).  The first
        one leaves every row unconstrained: set_automaton_starts says which rows enter it, and where.  Another table re-captures nothing."""
        a = automaton
        if getattr(self, "_automaton_set", None) is a and self.automaton:   # this very object is on the device and still on: nothing to upload
            return                                                            # (a set automaton's tables are not to be changed in place)
        if a.vocab != self.cfg.llm.vocab_size:
            raise ValueError(f"set_automaton: the automaton is over {a.vocab} ids, the model's vocabulary has {self.cfg.llm.vocab_size}")
        cls, allow, nxt = a.tables()
        _lib.check(self.lib.emmax_session_set_automaton(self._session, a.n_states, a.n_classes, cls.ctypes.data, allow.ctypes.data, nxt.ctypes.data,
                                                        _lib.current_stream()), "emmax_session_set_automaton")
        self._automaton_set = a

    def set_automaton_starts(self, starts: Sequence[int], row0: int = 0) -> None:
        """Rows row0..: the state each enters the automaton at with its next prefill (-1: unconstrained)."""
        k = len(starts)
        _lib.check(self.lib.emmax_session_set_automaton_starts(self._session, int(row0), k, (C.c_int32 * k)(*[int(v) for v in starts]), _lib.current_stream()),
                   "emmax_session_set_automaton_starts")

    def set_automaton_starts_staged(self, starts: Sequence[int]) -> None:
        """set_automaton_starts for the requests of the next slots_prefill_staged."""
        k = len(starts)
        _lib.check(self.lib.emmax_slots_set_automaton_starts_staged(self._session, k, (C.c_int32 * k)(*[int(v) for v in starts]), _lib.current_stream()),
                   "emmax_slots_set_automaton_starts_staged")

    def clear_automaton(self) -> None:
        _lib.check(self.lib.emmax_session_clear_automaton(self._session, _lib.current_stream()), "emmax_session_clear_automaton")
        self._automaton_set = None
        self._drop_unbound_top()

    @property
    def automaton(self) -> bool:
        return self.lib.emmax_session_automaton(self._session) == 1

    def automaton_state(self, row0: int = 0, n: int = 1) -> List[int]:
        """The automaton states of rows row0 .. row0 + n - 1 (staging row k = max_batch + k); synchronises with the device."""
        out = torch.empty(int(n), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.emmax_session_automaton_state(self._session, int(row0), int(n), out.data_ptr(), _lib.current_stream()),
                   "emmax_session_automaton_state")
        return out.cpu().tolist()

    def set_scores(self, scores: Optional[torch.Tensor], logits: Optional[torch.Tensor], max_new: int = 0, rows: int = 0) -> None:
        """Bind fp32 [max_new, rows, vocab] device buffers that the decode step fills with HF's `scores` (processed rows) / `logits` (raw
        rows) at each emitted token's index; `rows` must be the batch of the next prefill (the step stores row b of that batch at [t, b]).
        Either buffer may be None, both None unbinds.  The engine keeps the tensors alive while they are bound."""
        if scores is None and logits is None:
            _lib.check(self.lib.emmax_session_set_scores(self._session, None, None, 0, _lib.current_stream()), "emmax_session_set_scores")
            self._score_bufs = None
            return
        V = self.cfg.llm.vocab_size
        if int(rows) < 1 or int(max_new) < 1:
            raise ValueError(f"set_scores: max_new ({max_new}) and rows ({rows}) must be >= 1")
        for t in (scores, logits):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != (int(max_new), int(rows), V)
                                  or t.device != torch.device(self.device)):
                raise ValueError(f"set_scores: buffers must be contiguous fp32 [max_new={max_new}, rows={rows}, {V}] tensors on {self.device}, "
                                 f"got {tuple(t.shape)} {t.dtype} on {t.device}")
        _lib.check(self.lib.emmax_session_set_scores(self._session, scores.data_ptr() if scores is not None else None,
                                                     logits.data_ptr() if logits is not None else None, int(max_new), _lib.current_stream()),
                   "emmax_session_set_scores")
        self._score_bufs = (scores, logits)

    # ---- top-N and watched-token log-probabilities in the decode step (include/emmax.h: emmax_session_set_top_logprobs) ------
    def set_top_logprobs(self, n_top: int, watch_ids: Optional[Sequence[int]] = None, max_new: int = 1):
        """Bind buffers that every emitted token's top-`n_top` (id, log-probability) pairs and the log-probabilities of `watch_ids` are written
        into, at [row, t]: top_ids int32 / top_logprobs fp32 [rows, max_new, n_top] and watch_logprobs fp32 [rows, max_new, W], rows =
        max_batch + stage_rows (row = decode row or slot; staging row k = max_batch + k), filled with -1 / NaN: entries no token was emitted
        for keep that.  Needs sampling or processing on (greedy rows: temperature 0) and no beams.  Returns the three tensors; the engine
        keeps them alive while they are bound."""
        from .sampling import check_top_logprobs

        n, ids = check_top_logprobs(n_top, watch_ids, self.cfg.llm.vocab_size, "set_top_logprobs")
        W, T, R = len(ids), int(max_new), self.max_batch + self.stage_rows
        if n == 0 and W == 0:
            raise ValueError("set_top_logprobs: neither top_logprobs nor watch_ids asked for (clear_top_logprobs unbinds)")
        if T < 1:
            raise ValueError(f"set_top_logprobs: max_new ({max_new}) must be >= 1")
        bufs = (torch.full((R, T, n), -1, dtype=torch.int32, device=self.device), torch.full((R, T, n), float("nan"), dtype=torch.float32, device=self.device),
                torch.full((R, T, W), float("nan"), dtype=torch.float32, device=self.device))
        wi = (C.c_int32 * max(1, W))(*ids)
        _lib.check(self.lib.emmax_session_set_top_logprobs(self._session, n, bufs[0].data_ptr() if n else None, bufs[1].data_ptr() if n else None, W,
                                                           wi if W else None, bufs[2].data_ptr() if W else None, T, _lib.current_stream()),
                   "emmax_session_set_top_logprobs")
        self._top_bufs = bufs
        return bufs

    def _drop_unbound_top(self) -> None:
        """(the library unbinds when the logit rows are turned off: the buffers are the caller's again)"""
        if self._top_bufs is not None and not self.top_logprobs_bound:
            self._top_bufs = None

    def clear_top_logprobs(self) -> None:
        """Unbind: the session launches what it launched before, and the buffers are the caller's."""
        _lib.check(self.lib.emmax_session_clear_top_logprobs(self._session, _lib.current_stream()), "emmax_session_clear_top_logprobs")
        self._top_bufs = None

    def slot_top_logprobs(self, slot: int, n: int):
        """The first n entries of row / slot `slot` of the bound buffers, on the host: (top ids [n][N], top log-probabilities [n][N],
        watched log-probabilities [n][W]) as nested lists."""
        if self._top_bufs is None:
            raise _lib.EmmaxError("slot_top_logprobs: no buffers are bound (set_top_logprobs)")
        torch.cuda.current_stream().synchronize()
        return tuple(t[int(slot), : int(n)].cpu().tolist() for t in self._top_bufs)

    @property
    def top_logprobs_bound(self) -> bool:
        return self.lib.emmax_session_top_logprobs(self._session) == 1

    # ---- beam search inside the decode step (include/emmax.h, ABI 9) ------------------------------------------------------
    def set_beams(self, params) -> None:
        """Beams on (sampling.BeamParams): the next prefill takes G groups and generate() decodes them as G x num_beams rows on shared KV
        pages.  The session must hold G x num_beams rows (ensure_capacity first)."""
        es = {False: 0, True: 1, "never": 2}[params.early_stopping]
        _lib.check(self.lib.emmax_session_set_beams(self._session, int(params.num_beams), float(params.length_penalty), es, _lib.current_stream()),
                   "emmax_session_set_beams")
        self._beam_K = int(params.num_beams)

    def clear_beams(self) -> None:
        """Beams off: the session launches exactly what a greedy session launches, on the static page assignment."""
        _lib.check(self.lib.emmax_session_clear_beams(self._session, _lib.current_stream()), "emmax_session_clear_beams")
        self._beam_K = 0

    @property
    def beams(self) -> int:
        return max(int(self.lib.emmax_session_beams(self._session)), 0)

    def beam_result(self):
        """After generate() with beams on: (sequences int32 [G, K, T], lengths int32 [G, K], sequences_scores fp32 [G, K], beam_indices
        int32 [G, K, T]) on device, best first per group; T = the generation's max_new_tokens."""
        G, K, T = self._last_B, self._beam_K, self._beam_T
        seq = torch.empty(G, K, T, dtype=torch.int32, device=self.device)
        bix = torch.empty(G, K, T, dtype=torch.int32, device=self.device)
        lens = torch.empty(G, K, dtype=torch.int32, device=self.device)
        sc = torch.empty(G, K, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.emmax_session_beam_result(self._session, T, seq.data_ptr(), lens.data_ptr(), sc.data_ptr(), bix.data_ptr(),
                                                      _lib.current_stream()), "emmax_session_beam_result")
        return seq, lens, sc, bix

    def beam_trace(self):
        """After generate() with beams on: dict of device tensors -- tok, parent int32 [T, G, K]; score, lse fp32 [T, G, K]; cand_idx int32
        and cand_acc fp32 [T, G, 2K] (include/emmax.h: emmax_session_beam_trace)."""
        G, K, T = self._last_B, self._beam_K, self._beam_T
        i32 = lambda *sh: torch.empty(*sh, dtype=torch.int32, device=self.device)
        f32 = lambda *sh: torch.empty(*sh, dtype=torch.float32, device=self.device)
        tr = {"tok": i32(T, G, K), "parent": i32(T, G, K), "score": f32(T, G, K), "lse": f32(T, G, K), "cand_idx": i32(T, G, 2 * K),
              "cand_acc": f32(T, G, 2 * K)}
        _lib.check(self.lib.emmax_session_beam_trace(self._session, T, *[tr[k].data_ptr() for k in ("tok", "parent", "score", "lse", "cand_idx", "cand_acc")],
                                                     _lib.current_stream()), "emmax_session_beam_trace")
        return tr

    # ---- sample groups: N sampled rows per prompt (include/emmax.h: emmax_session_set_sample_groups) ------------------------
    def set_sample_groups(self, n: int) -> None:
        """Sample groups on: the next prefill takes G prompts and forks each into `n` sampled rows on the prompt's KV pages (row g n + j =
        sample j of prompt g).  Sampling must be set for all G x n rows, and the session must hold them (ensure_capacity first)."""
        _lib.check(self.lib.emmax_session_set_sample_groups(self._session, int(n), _lib.current_stream()), "emmax_session_set_sample_groups")
        self._group_N = int(n)

    def clear_sample_groups(self) -> None:
        """Groups off: a prefill's rows are independent prompts again, on the static page assignment."""
        _lib.check(self.lib.emmax_session_clear_sample_groups(self._session, _lib.current_stream()), "emmax_session_clear_sample_groups")
        self._group_N = 0

    @property
    def sample_groups(self) -> int:
        return max(int(self.lib.emmax_session_sample_groups(self._session)), 0)

    def attn_grouped(self, rows: int) -> bool:
        """Whether a decode step of `rows` rows, as the session is configured now, reads each group's shared prompt pages once
        (sample groups or forked beams; emmax_session_attn_grouped)."""
        return int(self.lib.emmax_session_attn_grouped(self._session, int(rows))) == 1

    @property
    def scores_bound(self) -> bool:
        return self._score_bufs is not None

    def slot_logprobs(self, slot: int, n: int) -> List[float]:
        """Log-probabilities of the first n tokens of `slot` (sampling on)."""
        out = torch.empty(max(1, n), dtype=torch.float32, device=self.device)
        _lib.check(self.lib.emmax_slot_logprobs(self._session, int(slot), out.data_ptr(), int(n), _lib.current_stream()), "emmax_slot_logprobs")
        return out[:n].cpu().tolist()

    # ---- early exit + slot serving (include/emmax.h "slot serving") ----------------------------------------------------
    def set_stop(self, trigger_ids: Sequence[int] = (), n_after: int = 0) -> None:
        """Device-side early exit: a row is done `n_after` tokens after it emitted `trigger_ids`; () clears the rule."""
        trig = list(trigger_ids)
        arr = (C.c_int32 * max(1, len(trig)))(*trig)
        _lib.check(self.lib.emmax_session_set_stop(self._session, arr, len(trig), int(n_after), _lib.current_stream()),
                   "emmax_session_set_stop")

    def slots_open(self, n_slots: int) -> None:
        self.ensure_decode_batch(int(n_slots))
        _lib.check(self.lib.emmax_slots_open(self._session, int(n_slots), _lib.current_stream()), "emmax_slots_open")
        self._score_bufs = None   # (emmax_slots_open unbinds scores)
        self._n_slots = int(n_slots)
        self._slot_state = torch.empty(2, n_slots, dtype=torch.int32, device=self.device)

    def slot_prefill(self, slot: int, input_ids: Sequence[int], patch_embeds: Optional[torch.Tensor], max_new_tokens: int) -> None:
        """Prefill one request (prompt ids starting with BOS, its [n_patches, hidden] bf16 patch embeddings) into `slot`."""
        ids_d = torch.as_tensor(list(input_ids), dtype=torch.int32).to(self.device)
        pe = None
        if patch_embeds is not None:
            pe = patch_embeds.contiguous()
            assert pe.dtype == self.patch_dtype and pe.numel() == self.cfg.n_patches * self.cfg.llm.hidden_size
        _lib.check(self.lib.emmax_slot_prefill(self._session, int(slot), ids_d.data_ptr(), len(input_ids), _lib.ptr(pe),
                                               int(max_new_tokens), _lib.current_stream()), "emmax_slot_prefill")
        torch.cuda.current_stream().synchronize()   # `ids_d` must outlive the embedding gather

    def slots_prefill(self, slot0: int, prompts: Sequence[Sequence[int]], patch_embeds: Optional[Sequence[torch.Tensor]],
                      max_new_tokens: Sequence[int]) -> None:
        """Prefill len(prompts) requests into the consecutive slots slot0.. in ONE packed pass (ragged prompt lengths)."""
        n = len(prompts)
        if n < 1 or len(max_new_tokens) != n:
            raise ValueError("slots_prefill: one token budget per prompt, at least one prompt")
        ids_d, lens, P, pe = self._pack_prompts("slots_prefill", prompts, 0, patch_embeds)
        lens_c = (C.c_int32 * n)(*lens)
        budget_c = (C.c_int32 * n)(*[int(v) for v in max_new_tokens])
        _lib.check(self.lib.emmax_slots_prefill(self._session, int(slot0), n, ids_d.data_ptr(), P, lens_c, _lib.ptr(pe), budget_c,
                                                _lib.current_stream()), "emmax_slots_prefill")
        torch.cuda.current_stream().synchronize()   # `ids_d` / `pe` must outlive the pass

    # ---- overlapped admission: staged prefill on a second stream + commit between two decode steps (include/emmax.h) ----
    def admission(self):
        """Context manager: everything issued inside (frame encode, staged prefill, their uploads) runs on the engine's admission
        stream, beside the decode steps of the current stream; ordered after the previous commit."""
        if self._adm_stream is None:
            self._adm_stream = torch.cuda.Stream(device=self.device)
        if self._commit_event is not None:
            self._adm_stream.wait_event(self._commit_event)
        return torch.cuda.stream(self._adm_stream)

    def slots_prefill_staged(self, prompts: Sequence[Sequence[int]], patch_embeds: Optional[Sequence[torch.Tensor]],
                             max_new_tokens: Sequence[int]):
        """Prefill len(prompts) requests into the session's STAGING rows; call inside `with engine.admission():`.  Returns a handle
        (`.ready()` -> bool, non-blocking) for `slots_commit`."""
        n = len(prompts)
        if n < 1 or len(max_new_tokens) != n:
            raise ValueError("slots_prefill_staged: one token budget per prompt, at least one prompt")
        ids_d, lens, P, pe = self._pack_prompts("slots_prefill_staged", prompts, 0, patch_embeds)
        lens_c = (C.c_int32 * n)(*lens)
        budget_c = (C.c_int32 * n)(*[int(v) for v in max_new_tokens])
        _lib.check(self.lib.emmax_slots_prefill_staged(self._session, n, ids_d.data_ptr(), P, lens_c, _lib.ptr(pe), budget_c,
                                                       _lib.current_stream()), "emmax_slots_prefill_staged")
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return _Staged(n, ev, (ids_d, pe))

    def slots_commit(self, staged: "_Staged", slots: Sequence[int], staged_idx: Optional[Sequence[int]] = None) -> None:
        """Move staged requests `staged_idx` (default: the first len(slots) not yet committed) into `slots` (idle) on the CURRENT
        (decode) stream, after the staged prefill has finished.  A batch may be committed piecemeal as slots free up."""
        k = len(slots)
        if staged_idx is None:
            staged_idx = list(range(staged.committed, staged.committed + k))
        if k < 1 or len(staged_idx) != k or max(staged_idx) >= staged.n:
            raise ValueError("slots_commit: one staged request per slot")
        torch.cuda.current_stream().wait_event(staged.event)
        sl = (C.c_int32 * k)(*[int(v) for v in slots])
        si = (C.c_int32 * k)(*[int(v) for v in staged_idx])
        _lib.check(self.lib.emmax_slots_commit(self._session, si, sl, k, _lib.current_stream()), "emmax_slots_commit")
        staged.committed += k
        self._commit_event = torch.cuda.Event()
        self._commit_event.record(torch.cuda.current_stream())
        if staged.committed >= staged.n:
            staged.keep = None

    # ---- sample groups as request slots (include/emmax.h: emmax_slots_fork) ---------------------------------------------------
    def slots_fork(self, src_slot: int, dst_slots: Sequence[int], params, seeds, subseqs, staged: Optional[int] = None) -> None:
        """Fork the freshly prefilled `src_slot` into the idle `dst_slots` on the current (decode) stream: they read its complete prompt
        pages and each draws its own token 0 from the prompt's logit row with its (params, seed, subseq).  `staged`: the index of the
        staged request the source was committed from (slots_commit), None for a source prefilled in place."""
        k, T, tk, tp, sd, sb = self._sampling_arrays(params, seeds, subseqs, len(dst_slots))
        if k != len(dst_slots):
            raise ValueError("slots_fork: one set of sampling parameters per destination slot")
        dst = (C.c_int32 * max(1, k))(*[int(v) for v in dst_slots])
        _lib.check(self.lib.emmax_slots_fork(self._session, int(src_slot), -1 if staged is None else int(staged), dst, k, T, tk, tp, sd, sb,
                                             _lib.current_stream()), "emmax_slots_fork")
        if staged is not None:   # the fork read the staging row's logits: the next staged prefill waits for it as it waits for the commit
            self._commit_event = torch.cuda.Event()
            self._commit_event.record(torch.cuda.current_stream())

    def slots_page_state(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """(page table, hidden pages) of every row, staging rows included: int32 [rows, max_pages] on the host; hidden is -1 where a row
        hides no page (tests: emmax_slots_page_state)."""
        rows, pages = self.max_batch + self.stage_rows, (self.max_ctx + 63) // 64   # (session.h: PAGE = 64 tokens)
        out = torch.empty(2, rows, pages, dtype=torch.int32, device=self.device)
        _lib.check(self.lib.emmax_slots_page_state(self._session, out[0].data_ptr(), out[1].data_ptr(), _lib.current_stream()), "emmax_slots_page_state")
        host = out.cpu()
        return host[0], host[1]

    def slots_step(self, n_steps: int) -> None:
        _lib.check(self.lib.emmax_slots_step(self._session, int(n_steps), _lib.current_stream()), "emmax_slots_step")

    def slots_state(self) -> Tuple[List[int], List[int]]:
        """(done flags, generated-token counts) of every slot; synchronises with the device."""
        st = self._slot_state
        _lib.check(self.lib.emmax_slots_state(self._session, st[0].data_ptr(), st[1].data_ptr(), _lib.current_stream()),
                   "emmax_slots_state")
        host = st.cpu()
        return host[0].tolist(), host[1].tolist()

    def slot_output(self, slot: int, n: int) -> List[int]:
        out = torch.empty(max(1, n), dtype=torch.int32, device=self.device)
        _lib.check(self.lib.emmax_slot_output(self._session, int(slot), out.data_ptr(), int(n), _lib.current_stream()),
                   "emmax_slot_output")
        return out[:n].cpu().tolist()

    def slot_release(self, slot: int) -> None:
        _lib.check(self.lib.emmax_slot_release(self._session, int(slot), _lib.current_stream()), "emmax_slot_release")

    def graph_active(self) -> bool:
        return bool(self.lib.emmax_session_graph_active(self._session))

    def profile_decode_stage(self, stage: int, reps: int = 3) -> float:
        """Mean duration (microseconds) of one launch of decode stage `stage` (see include/emmax.h), HIP-event timed."""
        us = C.c_float()
        _lib.check(self.lib.emmax_profile_decode_stage(self._session, stage, reps, C.byref(us), _lib.current_stream()),
                   "emmax_profile_decode_stage")
        return float(us.value)
