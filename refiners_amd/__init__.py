"""refiners_amd: MI355X-native hot path for refiners' SDXL UNet step behind the fluxion Chain / Adapter API."""


def namespace():
    """The mirror's public classes under the names `synth.apply_adapters` expects (same as refiners' own)."""
    from types import SimpleNamespace

    from .fluxion import layers as fl
    from .fluxion.adapters import Conv2dLora, LinearLora, LoraAdapter
    from .latent_diffusion.adapters import ConditionEncoder, ControlLoraAdapter, SDXLIPAdapter, ZeroConvolution
    from .latent_diffusion.multi_diffusion import (DiffusionTarget, MultiDiffusion, SD1DiffusionTarget, SD1MultiDiffusion, SDXLMultiDiffusion, SDXLTarget, Size,
                                                   Tile)
    from .latent_diffusion.style_aligned import StyleAlignedAdapter

    return SimpleNamespace(fl=fl, LinearLora=LinearLora, Conv2dLora=Conv2dLora, LoraAdapter=LoraAdapter, SDXLIPAdapter=SDXLIPAdapter,
                           ControlLoraAdapter=ControlLoraAdapter, ConditionEncoder=ConditionEncoder, ZeroConvolution=ZeroConvolution, StyleAlignedAdapter=StyleAlignedAdapter,
                           Tile=Tile, Size=Size, DiffusionTarget=DiffusionTarget, MultiDiffusion=MultiDiffusion, SDXLTarget=SDXLTarget,
                           SDXLMultiDiffusion=SDXLMultiDiffusion, SD1DiffusionTarget=SD1DiffusionTarget, SD1MultiDiffusion=SD1MultiDiffusion)


def __getattr__(name: str):
    """`from refiners_amd import CompiledTiledVAE`, resolved on first use (the engine pulls in torch and the native bindings)."""
    if name == "CompiledTiledVAE":
        from .engine.tiled_vae import CompiledTiledVAE

        return CompiledTiledVAE
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
