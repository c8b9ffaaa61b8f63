"""Host-side mirror of refiners' StyleAligned adapter (`foundationals/latent_diffusion/style_aligned.py:15-330`, arXiv:2312.02133):
a batch of images shares the style of the first one through its self-attentions.

The adapter works on a classifier-free-guidance batch of 2n rows = two halves of n rows; the reference row of row b is the
first row of its half, r(b) = (b // n) * n.  Inside every `fl.SelfAttention`, between the three projections and the SDPA:

    Q_b <- AdaIN(Q_b | Q_r(b))                                    (moments over the tokens, per channel)
    K_b <- [AdaIN(K_b | K_r(b)) ; s_b K_r(b)]                     (concatenated along the tokens: 2L keys)
    V_b <- [V_b ; s_b V_r(b)]
    s_b  = 1 for the reference rows, `scale` for the others.

Class names, child order and printed attributes follow the reference (`repr`, inject / eject, the `scale` accessors); on the
MI355X the whole insertion is two kernels per attention (mi355x_adain_stats, mi355x_style_aligned_pack) in front of an
unchanged 2L-key attention launch, see refiners_amd.engine.lowering_blocks.BlockLowering.shared_attention.  The scale is NOT
baked into the lowered program: the engine keeps it in device memory and refreshes it before every replay, so assigning
`adapter.scale` on a live tree costs no re-lowering.
"""
from functools import cached_property
from typing import Any, Generic, Optional, TypeVar

import torch
from torch import Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.adapters import Adapter

T = TypeVar("T", bound=fl.Chain)


def _halves(rows: int) -> int:
    assert rows >= 2 and rows % 2 == 0, f"StyleAligned works on a classifier-free-guidance batch (two equal halves), got {rows} row(s)"
    return rows // 2


class ExtractReferenceFeatures(fl.Module):
    """(2n, L, C) -> (2n, L, C): every row replaced by the first row of its half of the CFG batch."""

    def forward(self, features: Tensor) -> Tensor:
        n = _halves(features.shape[0])
        return features[0::n].repeat_interleave(n, dim=0)


class AdaIN(fl.Module):
    """(targets, reference) -> (targets with the reference's per-channel token statistics, reference)   [arXiv:1703.06868].
    The standard deviation is torch's default (unbiased) one and `epsilon` is added to IT, not to the variance."""

    def __init__(self, epsilon: float = 1e-8) -> None:
        super().__init__()
        self.epsilon = epsilon

    def forward(self, targets: Tensor, reference: Tensor) -> tuple[Tensor, Tensor]:
        t_std, t_mean = torch.std_mean(targets, dim=-2, keepdim=True)
        r_std, r_mean = torch.std_mean(reference, dim=-2, keepdim=True)
        return (targets - t_mean) / (t_std + self.epsilon) * r_std + r_mean, reference


class ScaleReferenceFeatures(fl.Module):
    """Multiplies the reference features that rows OTHER than the reference rows will attend to by `scale`."""

    def __init__(self, scale: float = 1.0) -> None:
        super().__init__()
        self.scale = scale

    def forward(self, features: Tensor) -> Tensor:
        n = _halves(features.shape[0])
        out = features * self.scale
        out[0::n] = features[0::n]
        return out


class StyleAligned(fl.Chain):
    """features -> (features, reference) -> [AdaIN] -> (features', s * reference) -> [features' ; s * reference] or features'."""

    def __init__(self, adain: bool, concatenate: bool, scale: float = 1.0) -> None:
        steps: list[Any] = [fl.Parallel(fl.Identity(), ExtractReferenceFeatures())]
        if adain:
            steps.append(AdaIN())
        steps.append(fl.Distribute(fl.Identity(), ScaleReferenceFeatures(scale=scale)))
        steps.append(fl.Concatenate(fl.GetArg(index=0), fl.GetArg(index=1), dim=-2) if concatenate else fl.GetArg(index=0))
        super().__init__(*steps)

    @property
    def scale(self) -> float:
        return self.ensure_find(ScaleReferenceFeatures).scale

    @scale.setter
    def scale(self, value: float) -> None:
        self.ensure_find(ScaleReferenceFeatures).scale = value


class SharedSelfAttentionAdapter(fl.Chain, Adapter[fl.SelfAttention]):
    """Wraps one `fl.SelfAttention` and, while injected, keeps Distribute(StyleAligned_q, StyleAligned_k, StyleAligned_v) in front of its SDPA."""

    #: (adain, concatenate) of the query, key and value branches
    BRANCHES = ((True, False), (True, True), (False, True))

    def __init__(self, target: fl.SelfAttention, scale: float = 1.0) -> None:
        with self.setup_adapter(target):
            super().__init__(target)
        self._style_aligned_layers = [StyleAligned(adain=a, concatenate=c, scale=scale) for a, c in self.BRANCHES]

    @cached_property
    def style_aligned_layers(self) -> fl.Distribute:
        return fl.Distribute(*self._style_aligned_layers)

    def inject(self, parent: Optional[fl.Chain] = None) -> "SharedSelfAttentionAdapter":
        self.target.insert_before_type(fl.ScaledDotProductAttention, self.style_aligned_layers)
        return super().inject(parent)

    def eject(self) -> None:
        self.target.remove(self.style_aligned_layers)
        super().eject()

    @property
    def scale(self) -> float:
        return self._style_aligned_layers[0].scale

    @scale.setter
    def scale(self, value: float) -> None:
        for branch in self._style_aligned_layers:
            branch.scale = value


class StyleAlignedAdapter(Generic[T], fl.Chain, Adapter[T]):
    """One SharedSelfAttentionAdapter per `fl.SelfAttention` of the UNet (70 on SDXL), injected and ejected together."""

    def __init__(self, target: T, scale: float = 1.0) -> None:
        with self.setup_adapter(target):
            super().__init__(target)
        self.shared_self_attention_adapters = tuple(SharedSelfAttentionAdapter(target=sa, scale=scale) for sa in self.target.layers(fl.SelfAttention))

    def inject(self, parent: Optional[fl.Chain] = None) -> "StyleAlignedAdapter[T]":
        for site in self.shared_self_attention_adapters:
            site.inject()
        return super().inject(parent)

    def eject(self) -> None:
        for site in self.shared_self_attention_adapters:
            site.eject()
        super().eject()

    @property
    def scale(self) -> float:
        return self.shared_self_attention_adapters[0].scale

    @scale.setter
    def scale(self, value: float) -> None:
        for site in self.shared_self_attention_adapters:
            site.scale = value
