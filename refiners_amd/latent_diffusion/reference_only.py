"""Reference-only control: condition SD1.5 on a guide image through its self-attentions, without a ControlNet
(reference latent_diffusion/reference_only_control.py; the "reference_only" preprocessor of sd-webui-controlnet).

Same class names, tree shape and context names as the reference:

* `SelfAttentionInjectionPassthrough`, at index 0 of the UNet, runs a structural copy of the UNet (`guide_unet`: the same leaf modules, so
  the same weights) on `reference_only_control.guide`.  In the copy every `CrossAttentionBlock`'s `SelfAttention` sits in a
  `SaveLayerNormAdapter`, which stores the attention's input -- the block's LayerNorm output -- as `self_attention_context_{i}.norm`.
  The copy's residual slots are set aside and its output is dropped.
* In the real pass every `SelfAttention` sits in a `SelfAttentionInjectionAdapter`: keys and values are projected from
  cat(x, norm_i) along the tokens, and row 0 of the CFG pair (the unconditional one) becomes
  `style_cfg * guided + (1 - style_cfg) * plain`.  `style_cfg` is a plain attribute read at forward time.

The adapter assumes a CFG pair: a batch of 2, [unconditional ; conditional], and a guide of the UNet input's shape (the caller passes
cat(guide, guide), noised for the step).  refiners_amd.engine.reference_only lowers both passes into one step program; the stock forward
of these classes is the fallback and the CPU parity subject.
"""
from __future__ import annotations

from typing import Any

from torch import Tensor

import refiners_amd.fluxion.layers as fl
from refiners_amd.fluxion.adapters import Adapter

from .blocks import CrossAttentionBlock


def context_name(i: int) -> str:
    return f"self_attention_context_{i}"


class SaveLayerNormAdapter(fl.Chain, Adapter[fl.SelfAttention]):
    """Guide pass: keep the self-attention's input for the real pass."""

    def __init__(self, target: fl.SelfAttention, context: str) -> None:
        self.context = context
        with self.setup_adapter(target):
            super().__init__(fl.SetContext(self.context, "norm"), target)


class SelfAttentionInjectionAdapter(fl.Chain, Adapter[fl.SelfAttention]):
    """Real pass: attend to the sample's own tokens and the guide's; blend row 0 with the plain attention."""

    def __init__(self, target: fl.SelfAttention, context: str, style_cfg: float = 0.5) -> None:
        self.context = context
        self.style_cfg = style_cfg

        sa_guided = target.structural_copy()  # (shares the Linears with `target`)
        assert isinstance(sa_guided[0], fl.Parallel)
        sa_guided.replace(
            sa_guided[0],
            fl.Parallel(
                fl.Identity(),
                fl.Concatenate(fl.Identity(), fl.UseContext(self.context, "norm"), dim=1),
                fl.Concatenate(fl.Identity(), fl.UseContext(self.context, "norm"), dim=1),
            ),
        )

        with self.setup_adapter(target):
            super().__init__(
                fl.Parallel(sa_guided, fl.Chain(fl.Lambda(lambda x: x[:1]), target)),
                fl.Lambda(self.compute_averaged_unconditioned_x),
            )

    def compute_averaged_unconditioned_x(self, x: Tensor, unguided_unconditioned_x: Tensor) -> Tensor:
        """Row 0 (the unconditional one) <- style_cfg * guided + (1 - style_cfg) * plain, in place; row 1 stays fully guided."""
        s = self.style_cfg
        x[0] = s * x[0] + (1.0 - s) * unguided_unconditioned_x
        return x


class SelfAttentionInjectionPassthrough(fl.Passthrough):
    """The guide pass, as the UNet's first child."""

    def __init__(self, target: Any) -> None:
        guide_unet = target.structural_copy()
        for i, block in enumerate(guide_unet.layers(CrossAttentionBlock)):
            sa = block.ensure_find(fl.SelfAttention)
            assert sa.parent is not None
            SaveLayerNormAdapter(sa, context=context_name(i)).inject()

        super().__init__(
            fl.Lambda(self._copy_diffusion_context),
            fl.UseContext("reference_only_control", "guide"),
            guide_unet,
            fl.Lambda(self._restore_diffusion_context),
        )

    def _copy_diffusion_context(self, x: Tensor) -> Tensor:
        """Set the residual slots aside for the length of the guide pass (a ControlNet may have filled them for the real pass) and hand the copy empty ones."""
        slots = self.use_context("unet")["residuals"]
        self.set_context("self_attention_residuals_buffer", {"buffer": slots})
        self.set_context("unet", {"residuals": [0.0 for _ in slots]})
        return x

    def _restore_diffusion_context(self, x: Tensor) -> Tensor:
        """Put the slots back: what the guide pass accumulated is dropped with its output."""
        kept = self.use_context("self_attention_residuals_buffer")["buffer"]
        self.set_context("unet", {"residuals": kept})
        return x


class ReferenceOnlyControlAdapter(fl.Chain, Adapter[Any]):
    """`style_cfg`: the weight of the guided attention in the unconditional row (0.5 is sd-webui-controlnet's recommendation)."""

    def __init__(self, target: Any, style_cfg: float = 0.5) -> None:
        self.sub_adapters: list[SelfAttentionInjectionAdapter] = []
        self._passthrough = [SelfAttentionInjectionPassthrough(target)]  # (in a list: not a child of the adapter)

        with self.setup_adapter(target):
            super().__init__(target)

        for i, block in enumerate(target.layers(CrossAttentionBlock)):
            self.set_context(context_name(i), {"norm": None})
            sa = block.ensure_find(fl.SelfAttention)
            assert sa.parent is not None
            self.sub_adapters.append(SelfAttentionInjectionAdapter(sa, context=context_name(i), style_cfg=style_cfg))

    def inject(self, parent: fl.Chain | None = None) -> "ReferenceOnlyControlAdapter":
        passthrough = self._passthrough[0]
        assert passthrough not in self.target, "the guide pass is already injected into this UNet"
        for adapter in self.sub_adapters:
            adapter.inject()
        self.target.insert(0, passthrough)
        return super().inject(parent)

    def eject(self) -> None:
        passthrough = self._passthrough[0]
        assert self.target[0] is passthrough, "the guide pass is no longer the UNet's first child: eject what was put in front of it first"
        for adapter in self.sub_adapters:
            adapter.eject()
        self.target.pop(0)
        super().eject()

    def set_controlnet_condition(self, condition: Tensor) -> None:
        self.set_context("reference_only_control", {"guide": condition})

    def structural_copy(self) -> "ReferenceOnlyControlAdapter":
        raise RuntimeError("a UNet under reference-only control cannot be copied (its guide pass is a copy of it already): eject the adapter first")
