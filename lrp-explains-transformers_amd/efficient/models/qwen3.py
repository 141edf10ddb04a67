"""Qwen3: Llama-style decoder with q/k RMSNorm inside the attention block (ref wiring: lxt/efficient/models/qwen3.py)"""
from transformers.models.qwen3 import modeling_qwen3 as MODELING_MODULE

from ._maps import decoder_maps

attnLRP, cp_LRP = decoder_maps(MODELING_MODULE, MODELING_MODULE.Qwen3MLP, MODELING_MODULE.Qwen3RMSNorm)

# the whole decoder layer as one fused autograd node where it applies, as models/llama.py does (patches._fused_layer_weights takes the q / k / v
# bias of Qwen2 and the q / k head norms of Qwen3); cp_LRP stays per-module
from functools import partial  # noqa: E402

from .. import patches as _P  # noqa: E402

for _tbl in (attnLRP,):
    _mod_patch = _tbl.pop(MODELING_MODULE)
    _tbl[MODELING_MODULE.Qwen3DecoderLayer] = partial(_P.patch_method, _P.decoder_layer_forward, keep_original=True)
    _tbl[MODELING_MODULE] = _mod_patch               # the modeling module stays last (ref lxt/efficient/models/__init__.py)
