"""Qwen2: Llama-style decoder with biased q/k/v projections (ref wiring: lxt/efficient/models/qwen2.py)"""
from transformers.models.qwen2 import modeling_qwen2 as MODELING_MODULE

from ._maps import decoder_maps

attnLRP, cp_LRP = decoder_maps(MODELING_MODULE, MODELING_MODULE.Qwen2MLP, MODELING_MODULE.Qwen2RMSNorm)

# the whole decoder layer as one fused autograd node where it applies, as models/llama.py does (patches._fused_layer_weights takes the q / k / v
# bias of Qwen2 and the q / k head norms of Qwen3); cp_LRP stays per-module
from functools import partial  # noqa: E402

from .. import patches as _P  # noqa: E402

for _tbl in (attnLRP,):
    _mod_patch = _tbl.pop(MODELING_MODULE)
    _tbl[MODELING_MODULE.Qwen2DecoderLayer] = partial(_P.patch_method, _P.decoder_layer_forward, keep_original=True)
    _tbl[MODELING_MODULE] = _mod_patch               # the modeling module stays last (ref lxt/efficient/models/__init__.py)
