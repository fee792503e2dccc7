"""Training of the hidden-state learning-to-rank head on the device (``ltr_head_train_*`` of libltr_hip.so).

The reference only Xavier-initialises this head (``vllm/model_executor/predictor.py:126-145``); its classes are the
encoder-less copy of allRank's ``FCModel`` / ``OutputLayer`` / ``LTRModel`` (``train/allrank/models/model.py:28-166``),
which allRank's loop trains (``train/allrank/training/train_utils.py:34-45``: loss, ``backward``, ``clip_grad_norm_``,
``opt.step``).  ``HipLTRHeadTrainer.step`` is one such step on stored hidden states; ``to_head`` hands the weights to
``HipLTRHead``.  The state dict uses the reference's parameter names, as ``HipLTRHead`` does.

With ``transformer`` (``ModelConfig.transformer``) allRank's slate encoder is trained between the FC stack and the output
layer (``ltr_head_train_create_encoder``): each row of the ``[B, S]`` labels is one slate, and an item whose label is
``pad_value`` is masked as a key (``transformer.py:166-167``; not under loss ``"given"``, which has no labels)."""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, metrics
from .ltr_head import HipLTRHead
from .train_loss import DEFAULT_EPS, PADDED_Y_VALUE


def _init_state(n_features: int, sizes: List[int], norm: bool, d_output: int) -> Dict[str, np.ndarray]:
    """predictor_model (predictor.py:126-145): xavier_uniform_ on every matrix, torch's defaults elsewhere."""
    sd = {}
    if norm:
        sd["input_layer.input_norm.weight"] = np.ones(n_features, np.float32)
        sd["input_layer.input_norm.bias"] = np.zeros(n_features, np.float32)
    dims = [n_features] + sizes
    names = [f"input_layer.layers.{i}" for i in range(len(sizes))] + ["output_layer.w_1"]
    for name, fan_in, fan_out in zip(names, dims, sizes + [d_output]):
        lin = torch.nn.Linear(fan_in, fan_out)
        torch.nn.init.xavier_uniform_(lin.weight)
        sd[name + ".weight"] = lin.weight.detach().numpy().copy()
        sd[name + ".bias"] = lin.bias.detach().numpy().copy()
    return sd


def _init_encoder_state(d_model: int, cfg: dict) -> Dict[str, np.ndarray]:
    """make_transformer (transformer.py:246-263): xavier_uniform_ on every matrix, torch's defaults on the biases; LayerNorm
    starts at a_2 = 1, b_2 = 0 (:79-81)."""
    sd = {}
    for i in range(cfg["N"]):
        p = f"encoder.layers.{i}."
        dims = [(p + f"self_attn.linears.{j}", d_model, d_model) for j in range(4)]
        dims += [(p + "feed_forward.w_1", d_model, cfg["d_ff"]), (p + "feed_forward.w_2", cfg["d_ff"], d_model)]
        for name, fan_in, fan_out in dims:
            lin = torch.nn.Linear(fan_in, fan_out)
            torch.nn.init.xavier_uniform_(lin.weight)
            sd[name + ".weight"] = lin.weight.detach().numpy().copy()
            sd[name + ".bias"] = lin.bias.detach().numpy().copy()
    for p in [f"encoder.layers.{i}.sublayer.{j}.norm." for i in range(cfg["N"]) for j in range(2)] + ["encoder.norm."]:
        sd[p + "a_2"], sd[p + "b_2"] = np.ones(d_model, np.float32), np.zeros(d_model, np.float32)
    return sd


def _encoder_names(cfg: dict) -> list:
    """The encoder's tensors in the order of ltr_head_encoder_create; a tuple names the three tensors stacked into one."""
    names = []
    for i in range(cfg["N"]):
        p = f"encoder.layers.{i}."
        qkv = lambda what: tuple(f"{p}self_attn.linears.{j}.{what}" for j in range(3))
        names += [p + "sublayer.0.norm.a_2", p + "sublayer.0.norm.b_2", qkv("weight"), qkv("bias"),
                  p + "self_attn.linears.3.weight", p + "self_attn.linears.3.bias",
                  p + "sublayer.1.norm.a_2", p + "sublayer.1.norm.b_2",
                  p + "feed_forward.w_1.weight", p + "feed_forward.w_1.bias",
                  p + "feed_forward.w_2.weight", p + "feed_forward.w_2.bias"]
    return names + ["encoder.norm.a_2", "encoder.norm.b_2"]


class HipLTRHeadTrainer:
    def __init__(self, n_features: int, fc_model: Optional[dict], post_model: dict,
                 state: Optional[Dict[str, np.ndarray]] = None, lr: float = 1e-3, weight_decay: float = 0.0,
                 loss: str = "listMLE", clip_norm: Optional[float] = None, device: str = "cuda:0",
                 betas=(0.9, 0.999), eps: float = 1e-8, listmle_eps: float = DEFAULT_EPS,
                 pad_value: float = PADDED_Y_VALUE, transformer: Optional[dict] = None, loss_args: Optional[dict] = None):
        """``loss_args``: allRank's ``loss.args`` of ``"lambdaLoss"`` (lambdaLoss.py:23-24: weighing_scheme, k, sigma, mu, reduction,
        reduction_log, eps, padded_value_indicator); eps and the padding value default to ``listmle_eps`` and ``pad_value``."""
        if transformer and (transformer.get("dropout") or transformer.get("positional_encoding") is not None):
            raise NotImplementedError("HipLTRHeadTrainer: the slate encoder is trained without dropout and without "
                                      "positional encoding; neither is built")
        if fc_model and fc_model.get("dropout"):
            raise NotImplementedError("HipLTRHeadTrainer: FCModel's dropout is not built (the device training step covers "
                                      "the dense layers, the input LayerNorm and the six activations)")
        if loss not in _lib.HEAD_LOSSES:
            raise ValueError(f"HipLTRHeadTrainer: loss {loss!r} (one of {sorted(_lib.HEAD_LOSSES)})")
        if loss_args and loss != "lambdaLoss":
            raise ValueError(f"HipLTRHeadTrainer: loss_args configure lambdaLoss, not {loss!r}")
        try:
            lam = (_lib.lambdaloss_config(**{"eps": listmle_eps, "padded_value_indicator": pad_value, **(loss_args or {})})
                   if loss == "lambdaLoss" else _lib.LambdaLossConfig())
        except TypeError as e:
            raise ValueError(f"HipLTRHeadTrainer: loss_args {sorted(loss_args)}: {e}") from None
        if not torch.cuda.is_available():
            raise _lib.LtrError("HipLTRHeadTrainer needs a ROCm GPU (no CPU fallback on the product path)")
        self.lib = _lib.load()
        self.device = torch.device(device)
        self.n_features, self.fc_model, self.post_model, self.loss = n_features, fc_model, post_model, loss
        self.transformer, self.pad_value = transformer, float(pad_value)
        sizes = list(fc_model["sizes"]) if fc_model else []
        norm = bool(fc_model and fc_model.get("input_norm"))
        if state is None:
            state = _init_state(n_features, sizes, norm, post_model["d_output"])
            if transformer:
                state.update(_init_encoder_state(sizes[-1] if sizes else n_features, transformer))
        self._names = (["input_layer.input_norm.weight", "input_layer.input_norm.bias"] if norm else [None, None])
        for i in range(len(sizes)):
            self._names += [f"input_layer.layers.{i}.weight", f"input_layer.layers.{i}.bias"]
        self._names += ["output_layer.w_1.weight", "output_layer.w_1.bias"]
        if transformer:
            self._names += _encoder_names(transformer)
        self._shapes = {k: tuple(np.shape(state[k])) for ks in self._names if ks for k in ([ks] if isinstance(ks, str) else ks)}
        stacked = lambda ks: np.asarray(state[ks]) if isinstance(ks, str) else np.concatenate([np.asarray(state[k]) for k in ks], 0)
        t = [torch.from_numpy(stacked(ks).astype(np.float32)).to(self.device).contiguous() if ks else None for ks in self._names]
        desc = _lib.HeadDesc()
        desc.n_features, desc.n_fc = n_features, len(sizes)
        for i, s in enumerate(sizes):
            desc.fc_sizes[i] = s
        desc.input_norm = 1 if norm else 0
        desc.activation = _lib.ACTIVATIONS[fc_model.get("activation") if fc_model else None]
        desc.d_output = post_model["d_output"]
        desc.output_activation = _lib.ACTIVATIONS[post_model.get("output_activation")]
        desc.weight_dtype = _lib.LTR_W_F32
        cfg = _lib.HeadTrainConfig(lr, betas[0], betas[1], eps, weight_decay, _lib.HEAD_LOSSES[loss], listmle_eps,
                                   pad_value, float(clip_norm) if clip_norm else 0.0, lam)
        ptrs = (C.c_void_p * len(t))(*[(x.data_ptr() if x is not None else None) for x in t])
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            if transformer:
                enc = _lib.HeadEncoderDesc(transformer["N"], transformer["d_ff"], transformer["h"], 0)
                _lib.check(self.lib.ltr_head_train_create_encoder(C.byref(desc), C.byref(enc), ptrs, len(t), C.byref(cfg),
                                                                  self._stream(), C.byref(self._h)), "ltr_head_train_create_encoder")
            else:
                _lib.check(self.lib.ltr_head_train_create(C.byref(desc), ptrs, len(t), C.byref(cfg), self._stream(),
                                                          C.byref(self._h)), "ltr_head_train_create")
        self._ws = None                      # grows, never shrinks
        self.scores: Optional[torch.Tensor] = None       # [B, S] of the last step, before its update
        self.grad_norm: Optional[torch.Tensor] = None    # [1] global L2 norm of the last step's gradients, before clipping

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self.lib.ltr_head_train_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def step(self, hidden: torch.Tensor, labels: torch.Tensor, row_index: Optional[torch.Tensor] = None,
             residual: Optional[torch.Tensor] = None, shuffle: Optional[torch.Tensor] = None,
             apply_update: bool = True) -> torch.Tensor:
        """hidden f32 / fp16 / bf16 [rows, n_features]; labels f32 [B, S] (loss "given": dLoss/dscore); row_index int32
        [B * S] or None (then rows == B * S).  Returns the loss, f32 [1] on the device (left 0 under "given")."""
        assert hidden.is_cuda and hidden.is_contiguous() and hidden.dim() == 2 and hidden.shape[1] == self.n_features
        if hidden.dtype not in HipLTRHead._HID:
            raise ValueError(f"HipLTRHeadTrainer.step: hidden dtype {hidden.dtype} (float32, float16 or bfloat16)")
        assert labels.dim() == 2
        B, S = labels.shape
        labels = labels.to(device=self.device, dtype=torch.float32).contiguous()
        if row_index is not None:
            row_index = row_index.to(device=self.device, dtype=torch.int32).contiguous()
        if (hidden.shape[0] if row_index is None else row_index.numel()) != B * S:
            raise ValueError("HipLTRHeadTrainer.step: labels [B, S] must name one selected row per item")
        if residual is not None and (residual.dtype != hidden.dtype or residual.shape != hidden.shape or not residual.is_contiguous()):
            raise ValueError("HipLTRHeadTrainer.step: residual must be contiguous with hidden's dtype and shape")
        if self.loss == "listMLE":
            if shuffle is None:
                shuffle = torch.randperm(S, device=self.device)          # listMLE.py:33
            shuffle = shuffle.to(device=self.device, dtype=torch.int32).contiguous()
        need = int(self.lib.ltr_head_train_workspace_bytes(self._h, B, S))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(max(need, 256), dtype=torch.uint8, device=self.device)
        loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.scores = torch.empty(B, S, dtype=torch.float32, device=self.device)
        self.grad_norm = torch.empty(1, dtype=torch.float32, device=self.device)
        ptr = lambda x: x.data_ptr() if x is not None else None
        with torch.cuda.device(self.device):
            _lib.check(self.lib.ltr_head_train_step(self._h, hidden.data_ptr(), ptr(residual), HipLTRHead._HID[hidden.dtype],
                                                    ptr(row_index), B, S, labels.data_ptr(), ptr(shuffle),
                                                    1 if apply_update else 0, loss.data_ptr(), self.scores.data_ptr(),
                                                    self.grad_norm.data_ptr(), self._ws.data_ptr(), self._ws.numel(),
                                                    self._stream()), "ltr_head_train_step")
        return loss

    def _read(self, what: int) -> Dict[str, torch.Tensor]:
        out = {}
        for i, name in enumerate(self._names):
            if name is None:
                continue
            n = C.c_size_t()
            _lib.check(self.lib.ltr_head_train_read(self._h, i, what, None, 0, C.byref(n), None), "ltr_head_train_read")
            t = torch.empty(n.value, dtype=torch.float32, device=self.device)
            _lib.check(self.lib.ltr_head_train_read(self._h, i, what, t.data_ptr(), n.value, C.byref(n), self._stream()),
                       "ltr_head_train_read")
            for k, part in zip([name] if isinstance(name, str) else name, [t] if isinstance(name, str) else t.chunk(3)):
                out[k] = part.view(self._shapes[k])
        return out

    def gradients(self) -> Dict[str, np.ndarray]:
        """The last step's gradients (after clipping), by reference parameter name."""
        return {k: v.cpu().numpy() for k, v in self._read(1).items()}

    def state_dict(self) -> Dict[str, np.ndarray]:
        return {k: v.cpu().numpy() for k, v in self._read(0).items()}

    def to_head(self, weight_dtype: str = "f16") -> HipLTRHead:
        return HipLTRHead(self.n_features, self.fc_model, self.post_model, self.state_dict(), device=str(self.device),
                          weight_dtype=weight_dtype, transformer=self.transformer)

    def evaluate(self, hidden: torch.Tensor, labels: torch.Tensor) -> float:
        """Kendall's tau-b of the labels and the current head's scores (train/trainer.py:195); the predictions stay on the
        device.  f32 hidden states are scored with the f32 weights, fp16 / bf16 ones as deployed (fp16 weights); the encoder
        always scores with fp16 weights, each row of the [B, S] labels as one slate."""
        head = self.to_head("f32" if hidden.dtype == torch.float32 and not self.transformer else "f16")
        if self.transformer:
            B, S = labels.shape
            pred = head.score(hidden, cu_slates=torch.arange(0, B * S + 1, S, dtype=torch.int32, device=self.device), max_slate=S)
        else:
            pred = head.score(hidden)
        return metrics.kendall_tau(labels.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous(), pred)

    def compute_metrics(self, hidden: torch.Tensor, labels: torch.Tensor, metrics: Dict[str, list],
                        row_index: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> Dict[str, float]:
        """allRank's epoch-end metrics of one batch (train_utils.py:48-72): ``{"ndcg": [5, 10], "mrr": [1]}`` ->
        ``{"ndcg_5": .., "ndcg_10": .., "mrr_1": ..}``, the means over the B slates of the [B, S] labels (label ``pad_value``: a
        padded item).  The scores are the current parameters', formed as in ``evaluate`` (a residual needs the batched path
        and therefore fp16 weights) and ranked on the device (``metrics.slate_metrics``; its ``mrr`` keeps the reference's
        batch-wide rule)."""
        from .metrics import slate_metrics               # (the argument carries allRank's name and hides the module)
        assert labels.dim() == 2
        B, S = labels.shape
        f32 = hidden.dtype == torch.float32 and not self.transformer and residual is None
        head = self.to_head("f32" if f32 else "f16")
        if self.transformer:
            pred = head.score(hidden, row_index, residual, max_slate=S,
                              cu_slates=torch.arange(0, B * S + 1, S, dtype=torch.int32, device=self.device))
        else:
            pred = head.score(hidden, row_index, residual)
        if pred.numel() != B * S:
            raise ValueError("HipLTRHeadTrainer.compute_metrics: labels [B, S] must name one scored row per item")
        return slate_metrics(pred.view(B, S), labels.to(device=self.device, dtype=torch.float32).contiguous(), metrics,
                             padding_indicator=self.pad_value)
