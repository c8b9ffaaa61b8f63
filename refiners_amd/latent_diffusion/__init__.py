from .ella import ELLA, ELLAAdapter, SD1ELLAAdapter  # noqa: F401
from .image_conditioned import ICLight, SD1Autoencoder, StableDiffusion_1_Inpainting  # noqa: F401
from .reference_only import ReferenceOnlyControlAdapter, SaveLayerNormAdapter, SelfAttentionInjectionAdapter, SelfAttentionInjectionPassthrough  # noqa: F401
