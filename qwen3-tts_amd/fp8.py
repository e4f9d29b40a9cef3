"""The row quantizer behind `TalkerEngine(weight_format="fp8")`, and the checkpoint that engine is equal to.

An fp8 engine stores the four decode operators of every talker layer (q|k|v, o, gate|up, down) as OCP e4m3fn codes with one
power-of-two scale per output row (include/qtts.h: `qtts_fp8_quantize_rows`).  It is defined without a tolerance: it computes, bit for
bit, what the bf16 engine computes on the checkpoint `effective_state_dict` returns.  Load that checkpoint into any implementation of
the model -- the reference's PyTorch model included -- to judge what the format costs in quality.

Host-only: nothing here touches a device.
"""
import ctypes as C
from typing import Any, Dict, Optional

import torch

from . import _lib
from .config import TalkerConfig


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", torch.float32).contiguous()


def quantize_rows(W: torch.Tensor, g: Optional[torch.Tensor] = None):
    """(codes uint8 (N, K), exps int32 (N)) of W (N, K), optionally scaled per input column by g (K): w' = W * g in fp32, exps[n] the
    smallest e with 448 * 2^e >= max_k |w'[n][k]| (0 for an all-zero row, clamped to [-100, 100]), codes = RNE_e4m3fn(w' * 2^-e)."""
    W = _f32(W)
    N, K = W.shape
    g = None if g is None else _f32(g)
    codes = torch.empty((N, K), dtype=torch.uint8)
    exps = torch.empty((N,), dtype=torch.int32)
    _lib.check(_lib.load_library().qtts_fp8_quantize_rows(C.c_void_p(W.data_ptr()), C.c_void_p(g.data_ptr()) if g is not None else None, N, K,
                                                          C.c_void_p(codes.data_ptr()), C.c_void_p(exps.data_ptr())))
    return codes, exps


def effective_weight(W: torch.Tensor, g: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W_eff (N, K) fp32: fl32(code * 2^e / g[k]), W[n][k] where g[k] == 0.  A bf16 engine bound with it (and the same g) packs exactly
    the numbers the fp8 engine multiplies with."""
    W = _f32(W)
    N, K = W.shape
    g = None if g is None else _f32(g)
    out = torch.empty((N, K), dtype=torch.float32)
    _lib.check(_lib.load_library().qtts_fp8_effective_rows(C.c_void_p(W.data_ptr()), C.c_void_p(g.data_ptr()) if g is not None else None, N, K,
                                                           C.c_void_p(out.data_ptr())))
    return out


# Linear weight of a talker layer -> the RMSNorm weight folded into its packed operator (None: nothing is folded)
_FOLDED_NORM = {"self_attn.q_proj.weight": "input_layernorm.weight", "self_attn.k_proj.weight": "input_layernorm.weight",
                "self_attn.v_proj.weight": "input_layernorm.weight", "self_attn.o_proj.weight": None,
                "mlp.gate_proj.weight": "post_attention_layernorm.weight", "mlp.up_proj.weight": "post_attention_layernorm.weight",
                "mlp.down_proj.weight": None}


def effective_state_dict(config: Any, state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A copy of `state_dict` in which the Linear weights of every talker layer (q, k, v, o, gate, up, down) are replaced by their W_eff
    (fp32), each with the norm weight it is folded with taken from the same dict.  Every other entry -- the code predictor, codec_head,
    embeddings, text projection, norms -- is returned as it is.  Keys with or without the checkpoint's `talker.` prefix."""
    cfg = TalkerConfig.from_any(config)
    prefix = "talker." if any(k.startswith("talker.") for k in state_dict) else ""
    out = dict(state_dict)
    for layer in range(int(cfg.num_hidden_layers)):
        base = f"{prefix}model.layers.{layer}."
        for lin, norm in _FOLDED_NORM.items():
            out[base + lin] = effective_weight(state_dict[base + lin], None if norm is None else state_dict[base + norm])
    return out
