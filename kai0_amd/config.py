"""Model configuration with openpi's field names (src/openpi/models/pi0_config.py:19-40,
src/openpi/models/gemma.py:43-109) so callers written against `Pi0Config` / `gemma.get_config` keep working."""

from __future__ import annotations

import dataclasses
import math
from typing import Literal

PALIGEMMA_VOCAB_SIZE = 257_152  # models/gemma.py:40

Variant = Literal["dummy", "gemma_300m", "gemma_2b", "gemma_2b_lora", "gemma_300m_lora", "dummy_lora"]


@dataclasses.dataclass(frozen=True)
class LoRAConfig:
    """`openpi.models.lora.LoRAConfig` (models/lora.py:11-30): rank, alpha and rank-stabilised scaling.  Both adapter matrices are
    initialised normal(0, 0.01) (:20) — lora_b is NOT zero."""

    rank: int
    alpha: float = 1.0
    rslora: bool = False
    init_std: float = 0.01

    @property
    def scaling_value(self) -> float:
        return self.alpha / math.sqrt(self.rank) if self.rslora else self.alpha / self.rank


@dataclasses.dataclass
class GemmaConfig:
    """`openpi.models.gemma.Config` (models/gemma.py:43-52).  `lora_configs`: {"attn": LoRAConfig, "ffn": LoRAConfig} as the reference
    keys them (gemma.py:185-199 the attention einsums, :238-244 the MLP); empty = no adapters."""

    width: int
    depth: int
    mlp_dim: int
    num_heads: int
    num_kv_heads: int
    head_dim: int
    lora_configs: dict = dataclasses.field(default_factory=dict)


def get_config(variant: str) -> GemmaConfig:
    """`openpi.models.gemma.get_config` (models/gemma.py:58-109).  Not in the reference: "dummy_lora" = "dummy" with rank-8 adapters
    of alpha 16 on attention and MLP — scaling_value 2 on the attention projections (and none in the MLP, which ignores alpha,
    lora.py:144-148), so that a misplaced scale is visible in tests; both shipped LoRA variants have scaling_value 1."""
    if variant == "dummy":
        return GemmaConfig(width=64, depth=4, mlp_dim=128, num_heads=8, num_kv_heads=1, head_dim=16)
    if variant == "gemma_300m":
        return GemmaConfig(width=1024, depth=18, mlp_dim=4096, num_heads=8, num_kv_heads=1, head_dim=256)
    if variant == "gemma_2b":
        return GemmaConfig(width=2048, depth=18, mlp_dim=16_384, num_heads=8, num_kv_heads=1, head_dim=256)
    if variant == "gemma_2b_lora":
        return dataclasses.replace(get_config("gemma_2b"), lora_configs={"attn": LoRAConfig(rank=16, alpha=16.0), "ffn": LoRAConfig(rank=16, alpha=16.0)})
    if variant == "gemma_300m_lora":
        return dataclasses.replace(get_config("gemma_300m"), lora_configs={"attn": LoRAConfig(rank=32, alpha=32.0), "ffn": LoRAConfig(rank=32, alpha=32.0)})
    if variant == "dummy_lora":
        return dataclasses.replace(get_config("dummy"), lora_configs={"attn": LoRAConfig(rank=8, alpha=16.0), "ffn": LoRAConfig(rank=8, alpha=16.0)})
    raise ValueError(f"Unknown variant: {variant}")


class FreezeFilter:
    """`Pi0Config.get_freeze_filter()`'s result: a picklable predicate over torch state-dict names, True = frozen.  `prefixes`: the
    name prefixes that are frozen; `keep`: a substring that exempts a name (the adapters)."""

    def __init__(self, prefixes: tuple = (), keep: str | None = None):
        self.prefixes, self.keep = tuple(prefixes), keep

    def __call__(self, name: str) -> bool:
        if self.keep is not None and self.keep in name:
            return False
        return any(name.startswith(p) for p in self.prefixes)

    def __eq__(self, other):
        return isinstance(other, FreezeFilter) and (self.prefixes, self.keep) == (other.prefixes, other.keep)

    def __repr__(self):
        return f"FreezeFilter(prefixes={self.prefixes!r}, keep={self.keep!r})"


_PALIGEMMA_LLM = ("paligemma_with_expert.paligemma.model.language_model.", "paligemma_with_expert.paligemma.lm_head.")
_EXPERT_LLM = ("paligemma_with_expert.gemma_expert.",)


@dataclasses.dataclass
class SiglipConfig:
    """SigLIP So400m/14 as the reference's PyTorch path always builds it (gemma_pytorch.py:24-41; HF
    SiglipVisionConfig defaults; models/siglip.py:318-363).  Only tests shrink it."""

    hidden_size: int = 1152
    num_layers: int = 27
    num_heads: int = 16
    intermediate_size: int = 4304
    patch_size: int = 14
    image_size: int = 224
    projection_dim: int = 2048
    layer_norm_eps: float = 1e-6


@dataclasses.dataclass
class Pi0Config:
    """`openpi.models.pi0_config.Pi0Config` fields (pi0_config.py:19-40).  pi05=True: pi0.5 (200 prompt slots, the state discretised
    into the prompt, adaRMS expert); pi05=False: pi0 (48 slots, `state` a model input — one state token in front of the action tokens,
    plain RMSNorm expert).  Both run on the HIP path (kai0_amd.model.PI0Pytorch)."""

    dtype: str = "bfloat16"
    paligemma_variant: str = "gemma_2b"
    action_expert_variant: str = "gemma_300m"
    action_dim: int = 32
    action_horizon: int = 50
    max_token_len: int | None = None
    pi05: bool = True
    discrete_state_input: bool | None = None
    # not in the reference: lets tests build a small vision tower / vocabulary
    siglip: SiglipConfig = dataclasses.field(default_factory=SiglipConfig)
    vocab_size: int = PALIGEMMA_VOCAB_SIZE

    def __post_init__(self):
        if self.max_token_len is None:
            self.max_token_len = 200 if self.pi05 else 48
        if self.discrete_state_input is None:
            self.discrete_state_input = self.pi05

    @property
    def model_type(self) -> str:
        """`ModelType` value (models/model.py:27-35; pi0_config.py:43-47)."""
        return "pi05" if self.pi05 else "pi0"

    def get_freeze_filter(self) -> FreezeFilter:
        """`Pi0Config.get_freeze_filter` (pi0_config.py:80-109) over torch state-dict names.  The reference's `.*llm.*` is every
        parameter of the two Gemma towers — here `paligemma.model.language_model.*` + `paligemma.lm_head.*` and `gemma_expert.*`:
        embedding, norms and the adaRMS `dense` layers included — `.*llm.*_1.*` the expert's, and `.*lora.*` any `.lora_` name.
        Both towers LoRA: both frozen; PaliGemma only: the expert stays trainable; expert only: the expert's base is frozen.  The
        adapters, SigLIP, the projector and the action / time / state heads are trainable in every case; without a LoRA variant
        nothing is frozen."""
        if "lora" in self.paligemma_variant:
            both = "lora" in self.action_expert_variant
            return FreezeFilter(_PALIGEMMA_LLM + (_EXPERT_LLM if both else ()), keep=".lora_")
        if "lora" in self.action_expert_variant:
            return FreezeFilter(_EXPERT_LLM, keep=".lora_")
        return FreezeFilter()

    def _model_class(self):
        from .model import PI0Pytorch

        return PI0Pytorch

    def load_pytorch(self, train_config, weight_path: str):
        """`BaseModelConfig.load_pytorch` (models/model.py:276-280): build the torch-protocol model from `train_config.model`
        and load `model.safetensors` (strict, tied `lm_head` forgiven as `safetensors.torch.load_model` does).  The weights
        are read before any trainer / inference engine exists, as both require (kai0_amd.sharded / kai0_amd.infer)."""
        import logging

        from .checkpoint import load_model_safetensors

        logging.getLogger("kai0_amd").info(f"train_config: {train_config}")
        model = train_config.model._model_class()(train_config.model)
        load_model_safetensors(model, weight_path)
        return model


@dataclasses.dataclass
class AdvantageEstimatorConfig(Pi0Config):
    """`openpi.models.pi0_config.AdvantageEstimatorConfig` (pi0_config.py:138-142): the two loss weights of the
    Stage-Advantage estimator (training/config.py:1225-1226 trains it with value 1 / action 0)."""

    loss_action_weight: float = 1.0
    loss_value_weight: float = 1.0

    def _model_class(self):
        from .model import AdvantageEstimator

        return AdvantageEstimator
