from .ella import ELLA, ELLAAdapter, SD1ELLAAdapter  # noqa: F401
