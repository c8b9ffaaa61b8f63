def __getattr__(name: str):
    # CompiledELLA beside the engines of the sub-modules (compiled, dinov2, swin, ...): resolved on first use, so that importing a sub-module of
    # this package does not load the native library's bindings of all the others
    if name == "CompiledELLA":
        from .ella import CompiledELLA

        return CompiledELLA
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
