"""Qwen3-MoE: Qwen3 attention + sparse MoE blocks (ref wiring: lxt/efficient/models/qwen3_moe.py).  The routed experts
(Qwen3MoeExperts) run on the grouped HIP GEMMs of efficient/moe.py; the dense layers of `mlp_only_layers` (Qwen3MoeMLP) take
the gated-MLP patch; the router stays HF's own module on ATen, as in the reference.  No CP-LRP map: the reference's is
commented out."""
from functools import partial

from transformers.models.qwen3_moe import modeling_qwen3_moe as MODELING_MODULE

from .. import patches as P
from ..moe import experts_forward
from ._maps import decoder_maps

_attn, _ = decoder_maps(MODELING_MODULE, MODELING_MODULE.Qwen3MoeMLP, MODELING_MODULE.Qwen3MoeRMSNorm)
attnLRP = {MODELING_MODULE.Qwen3MoeExperts: partial(P.patch_method, experts_forward), **_attn}
