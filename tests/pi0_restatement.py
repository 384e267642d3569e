"""CPU restatement of the reference's pi0 branch (`pi05=False`, pi0_pytorch.py:96-109, 243-297, 316-461), assembled from the blocks of
`oracle.pi0_oracle` (imported, not edited): the same PaliGemmaWithExpertModel with a NON-adaptive expert (`use_adarms=[False, False]`:
GemmaRMSNorm's `cond is None` path and ungated residuals), `state_proj` / `action_time_mlp_in` / `action_time_mlp_out` heads, a suffix
of one state token + H action-time tokens with att = [1, 1, 0, ...], and the last H suffix rows as the output.

tests/test_pi0_cpu.py pins it to tests/golden/reference_pi0.safetensors (vectors made by executing the reference's own code,
tests/golden/make_reference_pi0_golden.py); it is the arbiter at the real widths, where the fixture cannot go."""

import dataclasses
import os

import torch
import torch.nn.functional as F  # noqa: N812
from torch import nn

from oracle import pi0_oracle as O

PI0_ONLY_PREFIXES = ("state_proj.", "action_time_mlp_in.", "action_time_mlp_out.")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_pi0.safetensors")


class RestatedPI0(O.OraclePI0):
    """OraclePI0 with the pi0 branch's heads, suffix and output slice; everything else (prefix embedding, the joint forward, the KV-cache
    denoise pass, the Euler loop) is inherited."""

    def __init__(self, config: O.OracleConfig):
        nn.Module.__init__(self)
        assert not config.pi05
        self.config = config
        vlm = O.get_gemma_config(config.paligemma_variant)
        exp = O.get_gemma_config(config.action_expert_variant)
        self.paligemma_with_expert = O.PaliGemmaWithExpertModel(
            vlm, exp, use_adarms=[False, False], precision=config.dtype, vocab=config.vocab_size, sc=config.siglip
        )
        self.action_in_proj = nn.Linear(config.action_dim, exp.width)
        self.action_out_proj = nn.Linear(exp.width, config.action_dim)
        self.state_proj = nn.Linear(config.action_dim, exp.width)  # :107-109
        self.action_time_mlp_in = nn.Linear(2 * exp.width, exp.width)
        self.action_time_mlp_out = nn.Linear(exp.width, exp.width)
        self._state = None

    def embed_suffix_state(self, state, noisy_actions, timestep):  # :237-314, `not self.pi05`
        if self.state_proj.weight.dtype == torch.float32:
            state = state.to(torch.float32)
        state_emb = self.state_proj(state)
        b = state_emb.shape[0]
        width = self.action_in_proj.out_features
        te = O.create_sinusoidal_pos_embedding(timestep, width, min_period=4e-3, max_period=4.0)
        te = te.type(dtype=timestep.dtype)
        action_emb = self.action_in_proj(noisy_actions)
        te = te[:, None, :].expand_as(action_emb)
        x = self.action_time_mlp_out(F.silu(self.action_time_mlp_in(torch.cat([action_emb, te], dim=2))))
        embs = torch.cat([state_emb[:, None, :], x], dim=1)
        n = embs.shape[1]
        pad = torch.ones(b, n, dtype=torch.bool, device=timestep.device)
        att = torch.tensor([1, 1] + [0] * (self.config.action_horizon - 1), dtype=embs.dtype, device=embs.device)
        return embs, pad, att[None, :].expand(b, n), None

    def embed_suffix(self, noisy_actions, timestep):  # the inherited forward / denoise_step call it without the state
        return self.embed_suffix_state(self._state, noisy_actions, timestep)

    def forward(self, observation, actions, noise, time):
        self._state = observation.state
        return super().forward(observation, actions, noise, time)

    @torch.no_grad()
    def sample_actions(self, observation, noise, num_steps: int = 10):
        self._state = observation.state
        return super().sample_actions(observation, noise, num_steps)


def pi0_cfg(ocfg: O.OracleConfig) -> O.OracleConfig:
    return dataclasses.replace(ocfg, pi05=False)


def pi0_only_keys(sd) -> list[str]:
    """the state-dict keys the pi0.5 oracle does not have: the three pi0 heads and the expert's plain norm weights"""
    return [k for k in sd if k.startswith(PI0_ONLY_PREFIXES) or (".gemma_expert.model." in k and k.endswith("norm.weight"))]


def seeded_pi0_only(model: nn.Module, seed: int, std: float) -> dict:
    """Explicitly seeded values for the pi0-only tensors, in state-dict order: N(0, std) matrices, N(0, 0.02) biases, N(0, 0.1) norm
    weights (non-zero so that x_hat (1 + w) and its gradient are exercised)."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    sd = model.state_dict()
    for k in pi0_only_keys(sd):
        s = std if sd[k].dim() >= 2 else (0.1 if k.endswith("norm.weight") else 0.02)
        out[k] = (s * torch.randn(sd[k].shape, generator=g, dtype=torch.float32)).to(sd[k].dtype)
    return out


def shared_weights(ocfg05: O.OracleConfig, std: float, seed: int = 0) -> dict:
    """The pi0.5 oracle's synthetic weights (tests/tiny.build_pair's rescale of the matrices to `std`) for every key pi0 shares."""
    base = O.OraclePI0(ocfg05)
    O.synthetic_weights_(base, seed=seed)
    with torch.no_grad():
        for _, p in base.named_parameters():
            if p.dim() >= 2:
                p.mul_(std / 0.02)
    return {k: v.detach().clone() for k, v in base.state_dict().items()}


def build_restated(ocfg05: O.OracleConfig, pi0_only: dict, std: float, seed: int = 0) -> RestatedPI0:
    """RestatedPI0 on `ocfg05`'s shapes with the shared synthetic weights + the given pi0-only tensors (strict)."""
    m = RestatedPI0(pi0_cfg(ocfg05))
    sd = shared_weights(ocfg05, std, seed)
    keys = set(m.state_dict())
    m.load_state_dict({**{k: v for k, v in sd.items() if k in keys}, **pi0_only}, strict=True)
    return m.eval()


def bf16_ulp(x: torch.Tensor) -> torch.Tensor:
    """one unit in the last place of bf16 (8 significant bits) at the magnitude of x (f32 tensor): 2^(floor(log2 |x|) - 7)"""
    _, e = torch.frexp(x.float().abs().clamp_min(2.0**-126))  # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float32), e - 8)


def within_one_bf16_ulp(got: torch.Tensor, ref_f32: torch.Tensor, mag: torch.Tensor):
    """`got` (bf16) against bf16(ref_f32) where ref_f32 is an f32 sum of products whose terms' magnitudes add up to `mag`.
    -> (ok: bool tensor, share of elements that are bit-equal).

    Criterion: |got - bf16(ref)| <= 1 bf16 ulp(ref) + 2^-22 mag.  The second term is the f32 level itself: two f32 evaluations of the same
    sum in different orders are each within ~2 eps32 mag of the exact value (torch's own single-`cat` form measures 1.3e-7 mag = 2.2 eps32
    mag against float64 at K = 2048 + 1024), so they differ by up to 4 eps32 mag = 2^-22 mag.  Where |ref| >> mag 2^-15 that is a
    thousandth of an ulp and the criterion is "within one bf16 ulp"; at a zero crossing of the output (|ref| < ~1e-4 here: 4 of 102400
    elements between torch's cat form and torch's split form on the CPU, up to 10 ulps of a 5e-5 value apart while 1e-7 mag apart in f32)
    one ulp of the tiny result is BELOW the f32 uncertainty of the reference, and no summation order can meet it."""
    rb = ref_f32.to(torch.bfloat16)
    d = (got.float() - rb.float()).abs()
    ok = d <= bf16_ulp(rb.float()) + 2.0**-22 * mag.float()
    return ok, float((got == rb).float().mean())
