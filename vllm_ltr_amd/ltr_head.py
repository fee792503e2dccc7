"""Hidden-state learning-to-rank head on the device (``ltr_head_*`` of libltr_hip.so).

Mirrors ``vllm/model_executor/predictor.py`` (``predictor_model`` / ``LTRModel.score``) and the
``PredictorConfig`` JSON (``vllm/config_predictor.py:78-117``); the state dict uses the reference's
parameter names (``input_layer.input_norm.*``, ``input_layer.layers.<i>.*``, ``output_layer.w_1.*``).

With ``transformer`` (the ``ModelConfig.transformer`` block, ``vllm/config_predictor.py:8-38``) allRank's slate encoder runs
between the FC stack and the output layer (``train/allrank/models/model.py:147-161``, ``transformer.py``); its parameters
use allRank's names: ``encoder.layers.<i>.self_attn.linears.<0-3>.*``, ``encoder.layers.<i>.feed_forward.w_<1|2>.*``,
``encoder.layers.<i>.sublayer.<0|1>.norm.{a_2,b_2}``, ``encoder.norm.{a_2,b_2}``.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib


class HipLTRHead:
    def __init__(self, n_features: int, fc_model: Optional[dict], post_model: dict, state: Dict[str, np.ndarray],
                 device: str = "cuda:0", weight_dtype: str = "f16", transformer: Optional[dict] = None):
        if not torch.cuda.is_available():
            raise _lib.LtrError("HipLTRHead needs a ROCm GPU (no CPU fallback on the product path)")
        self.lib = _lib.load()
        self.device = torch.device(device)
        wt = torch.float16 if weight_dtype == "f16" else torch.float32
        f32 = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32)).to(self.device).contiguous()
        mat = lambda a: torch.from_numpy(np.asarray(a).astype(np.float32)).to(self.device, wt).contiguous()
        sizes = list(fc_model["sizes"]) if fc_model else []
        norm = bool(fc_model and fc_model.get("input_norm"))
        t = [f32(state["input_layer.input_norm.weight"]) if norm else None,
             f32(state["input_layer.input_norm.bias"]) if norm else None]
        for i in range(len(sizes)):
            t += [mat(state[f"input_layer.layers.{i}.weight"]), f32(state[f"input_layer.layers.{i}.bias"])]
        t += [mat(state["output_layer.w_1.weight"]), f32(state["output_layer.w_1.bias"])]
        self._tensors = t
        self.n_features = n_features
        self._ws = None                      # workspace of the batched path: grows, never shrinks
        desc = _lib.HeadDesc()
        desc.n_features, desc.n_fc = n_features, len(sizes)
        for i, s in enumerate(sizes):
            desc.fc_sizes[i] = s
        desc.input_norm = 1 if norm else 0
        desc.activation = _lib.ACTIVATIONS[fc_model.get("activation") if fc_model else None]
        desc.d_output = post_model["d_output"]
        desc.output_activation = _lib.ACTIVATIONS[post_model.get("output_activation")]
        desc.weight_dtype = _lib.LTR_W_F16 if weight_dtype == "f16" else _lib.LTR_W_F32
        ptrs = (C.c_void_p * len(t))(*[(x.data_ptr() if x is not None else None) for x in t])
        self._h = C.c_void_p()
        _lib.check(self.lib.ltr_head_create(C.byref(desc), ptrs, len(t), C.byref(self._h)), "ltr_head_create")
        self._enc = None
        if transformer:
            self._create_encoder(transformer, state, f32, mat)

    def _create_encoder(self, cfg: dict, state, f32, mat) -> None:
        t = []
        for i in range(cfg["N"]):
            p = f"encoder.layers.{i}."
            lin = lambda j, what: np.asarray(state[f"{p}self_attn.linears.{j}.{what}"])
            t += [f32(state[p + "sublayer.0.norm.a_2"]), f32(state[p + "sublayer.0.norm.b_2"]),
                  mat(np.concatenate([lin(j, "weight") for j in range(3)], 0)),        # Q | K | V as one GEMM
                  f32(np.concatenate([lin(j, "bias") for j in range(3)], 0)),
                  mat(lin(3, "weight")), f32(lin(3, "bias")),
                  f32(state[p + "sublayer.1.norm.a_2"]), f32(state[p + "sublayer.1.norm.b_2"]),
                  mat(state[p + "feed_forward.w_1.weight"]), f32(state[p + "feed_forward.w_1.bias"]),
                  mat(state[p + "feed_forward.w_2.weight"]), f32(state[p + "feed_forward.w_2.bias"])]
        t += [f32(state["encoder.norm.a_2"]), f32(state["encoder.norm.b_2"])]
        self._enc_tensors = t
        desc = _lib.HeadEncoderDesc(cfg["N"], cfg["d_ff"], cfg["h"], 0 if cfg.get("positional_encoding") is None else 1)
        ptrs = (C.c_void_p * len(t))(*[x.data_ptr() for x in t])
        enc = C.c_void_p()
        _lib.check(self.lib.ltr_head_encoder_create(self._h, C.byref(desc), ptrs, len(t), C.byref(enc)),
                   "ltr_head_encoder_create")
        self._enc = enc

    def __del__(self):
        try:
            if getattr(self, "_enc", None):
                self.lib.ltr_head_encoder_destroy(self._enc)
                self._enc = None
            if getattr(self, "_h", None):
                self.lib.ltr_head_destroy(self._h)
                self._h = None
        except Exception:
            pass

    _HID = {torch.float32: _lib.LTR_HID_F32, torch.float16: _lib.LTR_HID_F16, torch.bfloat16: _lib.LTR_HID_BF16}

    def reserve(self, n: int) -> None:
        """Size the batched path's workspace for calls of up to ``n`` rows (it only grows; do it before a graph capture)."""
        need = int(self.lib.ltr_head_encoder_workspace_bytes(self._enc, n) if self._enc
                   else self.lib.ltr_head_workspace_bytes(self._h, n))
        if self._ws is None or self._ws.numel() < need:
            if torch.cuda.is_current_stream_capturing():
                raise _lib.LtrError(f"HipLTRHead: the workspace must grow to {need} bytes for {n} rows while the stream is "
                                    "capturing; call reserve(n) before the capture")
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)

    def score(self, hidden: torch.Tensor, row_index: Optional[torch.Tensor] = None,
              residual: Optional[torch.Tensor] = None, batched: Optional[bool] = None,
              cu_slates: Optional[torch.Tensor] = None, max_slate: Optional[int] = None) -> torch.Tensor:
        """hidden f32 / fp16 / bf16 [rows, n_features] on the device; row_index int32 (or int64) [N] or None; residual None or a
        tensor like hidden (the rows scored are ``residual + hidden`` in hidden's dtype, opt.py:250-255).

        f32 hidden without residual runs the row kernel (``ltr_head_score``) unless ``batched=True``; fp16 / bf16 hidden
        or a residual run the batched MFMA path (``ltr_head_score_batched``), which ``batched=False`` therefore refuses.

        A head with an encoder always runs ``ltr_head_encoder_score``.  ``cu_slates`` int32 [B + 1] on the device groups the
        N rows into slates (ascending, from 0 to N); None: the whole call is one slate, the queue.  ``max_slate`` is the
        longest slate, a grid-sizing hint that is never wrong, only slow when too small.  With ``max_slate=None`` the
        array is read back once to find it and to check its ends (not during a stream capture: pass ``max_slate`` there)."""
        assert hidden.is_cuda and hidden.is_contiguous() and hidden.dim() == 2 and hidden.shape[1] == self.n_features
        if hidden.dtype not in self._HID:
            raise ValueError(f"HipLTRHead.score: hidden dtype {hidden.dtype} (float32, float16 or bfloat16)")
        if row_index is not None and row_index.dtype != torch.int32:
            row_index = row_index.to(torch.int32)              # selected_token_indices arrives as int64
        n = hidden.shape[0] if row_index is None else row_index.numel()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        idx = row_index.data_ptr() if row_index is not None else None
        if self._enc is None and (cu_slates is not None or max_slate is not None):
            raise ValueError("HipLTRHead.score: cu_slates / max_slate need a head with a transformer encoder")
        if self._enc is not None:
            if batched is False:
                raise ValueError("HipLTRHead.score: the encoder has no row kernel (batched=False)")
            batched = True
        if batched is None:
            batched = hidden.dtype != torch.float32 or residual is not None
        if not batched:
            if hidden.dtype != torch.float32 or residual is not None:
                raise ValueError("HipLTRHead.score: batched=False is the f32 row kernel; it takes no fp16 / bf16 hidden "
                                 "and no residual")
            out = torch.empty(n, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.ltr_head_score(self._h, hidden.data_ptr(), idx, n, out.data_ptr(), stream), "ltr_head_score")
            return out
        if residual is not None:
            assert residual.is_cuda and residual.is_contiguous()
            if residual.dtype != hidden.dtype or residual.shape != hidden.shape:
                raise ValueError("HipLTRHead.score: residual must have hidden's dtype and shape")
        self.reserve(n)
        out = torch.empty(n, dtype=torch.float32, device=self.device)
        if self._enc is not None:
            n_slates = 1
            if cu_slates is not None:
                assert cu_slates.is_cuda and cu_slates.is_contiguous() and cu_slates.dtype == torch.int32 and cu_slates.dim() == 1
                n_slates = cu_slates.numel() - 1
                if n_slates < 0:
                    raise ValueError("HipLTRHead.score: cu_slates is empty")
                if max_slate is None and not torch.cuda.is_current_stream_capturing():
                    cu = cu_slates.cpu().numpy()
                    if cu[0] != 0 or cu[-1] != n or (np.diff(cu) < 0).any():
                        raise ValueError(f"HipLTRHead.score: cu_slates must ascend from 0 to N = {n}")
                    max_slate = int(np.diff(cu).max()) if n_slates else 0
            _lib.check(self.lib.ltr_head_encoder_score(
                self._enc, hidden.data_ptr(), residual.data_ptr() if residual is not None else None, self._HID[hidden.dtype],
                idx, n, cu_slates.data_ptr() if cu_slates is not None else None, n_slates,
                n if max_slate is None else int(max_slate), out.data_ptr(), self._ws.data_ptr(), self._ws.numel(), stream),
                "ltr_head_encoder_score")
            return out
        _lib.check(self.lib.ltr_head_score_batched(self._h, hidden.data_ptr(),
                                                   residual.data_ptr() if residual is not None else None,
                                                   self._HID[hidden.dtype], idx, n, out.data_ptr(), self._ws.data_ptr(),
                                                   self._ws.numel(), stream), "ltr_head_score_batched")
        return out
