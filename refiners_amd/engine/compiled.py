"""Run-time side of the MI355X engine: static I/O staging, (re)lowering on tree changes, HIP-graph replay.

`CompiledUNet` is what a refiners user switches to:

    unet = SDXLUNet(...)                       # refiners_amd.latent_diffusion (or refiners' own class)
    fast = CompiledUNet(unet)                  # nothing happens yet
    unet.set_timestep(t); unet.set_clip_text_embedding(e); ...   # same context API as always
    y = fast(x)                                # == unet(x), on hand-written gfx950 kernels

It keeps refiners' contract at the UNet boundary (reference latent_diffusion/model.py:128-159 calls `self.unet(latents)`
after `set_unet_context`): inputs come from the UNet's context store, the context is reset after the call exactly like
`Chain.forward` does (chain.py:245-257), adapters may be injected / ejected / rescaled between calls (the lowering is
redone when `tree_epoch()` moved).  `CompiledSDXL` adds the classifier-free-guidance + DDIM update as one more kernel and
replays a whole denoising step as ONE HIP graph launch.

There is no silent fallback: if the native library is missing this module raises.  A tree shape the lowering does not know follows the
reference's own convention for unknown children -- the stock child loop runs (fluxion/layers/chain.py:226-257; SURVEY.md section 8(b):
"unsupported => fall back, never error") -- at two levels, both reported: a context-free sub-tree inside a UNet stage runs through its own
torch forward inside the recorded program (`.stats["fallback_nodes"]`); anything else (a node that needs the Chain's context store at run
time, an unknown top-level layout) makes the WHOLE call run `unet(x)`, with a `RuntimeWarning` naming the reason and
`.stats["whole_fallback"]` set.  Adapters outside SURVEY.md section 8 (FreeU ...) therefore keep working, unfused.
StyleAlignedAdapter is lowered (`.stats["style_aligned_sites"]`): its scale lives in device memory and is refreshed before every replay.
"""
from __future__ import annotations

import os

import warnings
from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .packing import PackCache, Unsupported, isa, kids, launches  # noqa: F401
from .unet_lowering import UNetIO, UNetLowering  # noqa: F401

TOKEN_CONTEXTS = (("cross_attention_block", "clip_text_embedding"), ("ip_adapter", "clip_image_embedding"), ("adapted_cross_attention_block", "llm_text_embedding"))


def _ident(t: Optional[Tensor]) -> Any:
    """Identity of a prompt-side input.  The key alone is not enough: once the caller drops the tensor the allocator may hand
    the same block (same data_ptr, same _version) to the NEXT prompt's embedding, so whoever stores this key also stores the
    tensor itself (CompiledUNet.prologue_refs) -- a live tensor's address cannot be recycled."""
    return None if t is None else (id(t), t.data_ptr(), t._version, tuple(t.shape), t.dtype)


def _weights_version(unet: Any, cache: Optional[dict] = None, epoch: Any = None) -> int:
    """Changes whenever a parameter is updated IN PLACE (load_state_dict / load_from_safetensors without assign,
    parallel.broadcast_module, optimizer steps): converted, merged and K-blocked copies must then be rebuilt.  `cache` (owned by
    the CompiledUNet, so it dies with it) keeps the parameter list of a mirror tree per tree epoch: the walk over ~2 900 modules
    costs more than the sum."""
    if cache is None or epoch is None:
        return sum(p._version for p in unet.parameters())
    if cache.get("epoch") != epoch:
        cache["epoch"], cache["params"] = epoch, list(unet.parameters())
    return sum(p._version for p in cache["params"])


class Program:
    """A lowered launch list replayed directly the first time and as ONE HIP graph afterwards (every buffer is static)."""

    def __init__(self, ops: list, use_graph: bool, weight_prefetch: Optional[bool] = None, low: Any = None) -> None:
        # `low`: the Lowering the launches came from.  Given, every run ends with a look at its hand-over error words (in-launch LoRA, stream-K):
        # these programs -- text / image encoders, SAM -- run once per prompt or picture and their callers read the result next, so the host
        # round trip costs nothing that is not paid anyway
        self.ops, self.use_graph, self.low = ops, use_graph, low
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        if weight_prefetch is None:
            weight_prefetch = os.environ.get("REFINERS_AMD_WEIGHT_PREFETCH", "1") != "0"
        self.prefetch = native.link_weight_prefetch(ops, enable=weight_prefetch)  # every GEMM pulls the next one's weights into the Infinity Cache

    def run(self) -> None:
        if self.use_graph and self.graph is not None:
            self.graph.replay()
        else:
            native.replay(self.ops)  # also the warm-up: first-launch work (function attributes) must not be captured
            if self.use_graph:
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    native.replay(self.ops)
                self.graph = g
        if self.low is not None:
            bad = self.low.handover_pending()
            if bad and bool((bad[0] if len(bad) == 1 else torch.stack(bad).any()).item()):
                self.low.handover_raise()


class CompiledUNet:
    def __init__(self, unet: Any, use_graph: bool = True, lora_mode: str = "fused") -> None:
        native.load()  # fail loudly: there is no fallback for a missing HIP library
        self.unet = unet
        self.use_graph = use_graph
        self.lora_mode = lora_mode  # see Lowering.__init__
        self.weight_prefetch = os.environ.get("REFINERS_AMD_WEIGHT_PREFETCH", "1") != "0"
        self.cache = PackCache()
        self.io_override: Optional[tuple[Tensor, Tensor]] = None  # (x, out) buffers owned by the caller instead of fresh ones (see _build)
        self.low: Optional[UNetLowering] = None
        self.io: Optional[UNetIO] = None
        self.key: Any = None
        self.bad_key: Any = None  # the (tree state, geometry) key whose lowering raised Unsupported: those calls run the stock forward
        # the modules whose live attributes the lowered program reads from device memory, as the last lowering met them -- StyleAligned's ScaleReferenceFeatures
        # (`scale`) and reference-only control's SelfAttentionInjectionAdapters (`style_cfg`) -- and their values when the tree was last refused: assigning one
        # bumps no tree epoch, so a refusal is retried when these values moved
        self.style_watch: list = []
        self.ro_watch: list = []
        self.bad_values: Any = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.prologue_key: Any = None
        self.prologue_refs: Any = None  # the staged source tensors themselves (see _ident)
        self.stats: dict[str, Any] = {}
        self.lowerings, self.prologue_runs = 0, 0  # over this engine's life; shown in `stats` (a re-lowering replaces the dict, not the counts)

    # -- context plumbing ----------------------------------------------------------------------------------
    def _tree(self) -> Any:
        """The UNet itself when the engine was given the chain of an adapter that is the UNet's parent (ELLAAdapter = Chain(unet))."""
        u = self.unet
        if isa(u, "ELLAAdapter") and len(kids(u)) == 1:
            u = kids(u)[0]
        return u

    def _contexts(self) -> dict[str, dict[str, Any]]:
        # Chain.set_context REPLACES the top-level dict but MERGES into every descendant's (context.py:16-46,
        # chain.py:131-156), so after set_timestep / set_time_ids / ... only a child Chain sees
        # all of them -- read where the UseContext nodes read, not at unet.provider.
        # (not at an ELLA encoder or a reference-only guide pass at index 0 either: they joined the tree at inject() and have seen only the contexts set since)
        tree = self._tree()
        child = next((m for m in kids(tree) if isa(m, "Chain") and not isa(m, "ELLA", "SelfAttentionInjectionPassthrough")), None)
        return (child if child is not None else tree).provider.contexts

    def reference_only(self) -> bool:
        """The tree carries reference-only control: its guide pass is the UNet's first child."""
        return any(isa(m, "SelfAttentionInjectionPassthrough") for m in kids(self._tree())[:1])

    def _gather(self) -> dict[str, Any]:
        c = self._contexts()
        diff = c.get("diffusion", {})
        got: dict[str, Any] = {"timestep": diff.get("timestep"), "pooled": diff.get("pooled_text_embedding"), "time_ids": diff.get("time_ids"), "tokens": {}, "conditions": {},
                               "t2i": {}}
        assert got["timestep"] is not None, "context diffusion.timestep is unset (call unet.set_timestep first)"
        ella = any(isa(m, "ELLA") for m in kids(self._tree()))  # (its LLM embedding outlives an eject() in the context store: without the encoder nothing reads it)
        for ctx, key in TOKEN_CONTEXTS:
            v = c.get(ctx, {}).get(key)
            if v is not None and (ella or ctx != "adapted_cross_attention_block"):
                got["tokens"][(ctx, key)] = v
        for name, d in c.items():
            if name.startswith("control_lora_") and d.get("condition") is not None:
                got["conditions"][name] = d["condition"]
            if name == "controlnet":  # SD1.5 Controlnet adapters share one context, one key per adapter (sd1/controlnet.py:200-204)
                for key, v in d.items():
                    if key.startswith("condition_") and v is not None:
                        got["conditions"][f"controlnet.{key}"] = v
        if self.reference_only():  # (the guide outlives an eject() in the context store)
            got["guide"] = c.get("reference_only_control", {}).get("guide")  # a STEP input: read and copied on every call
        for key, feats in c.get("t2iadapter", {}).items():  # T2IAdapter.set_condition_features (t2i_adapter.py:201-202)
            if key.startswith("condition_features_") and feats is not None:
                got["t2i"][key.removeprefix("condition_features_")] = tuple(feats)
        return got

    # -- lowering ----------------------------------------------------------------------------------------------
    def _build(self, x_shape: tuple, dev: torch.device, got: dict[str, Any]) -> None:
        dtype = self.unet.dtype
        assert dtype in (torch.float32, torch.bfloat16), f"the MI355X path computes in float32 or bfloat16, not {dtype}"
        B, _, H, W = x_shape
        xbuf, obuf = self.io_override if self.io_override is not None else (None, None)  # CompiledSDXL's split CFG pair: halves of ONE 2n-row buffer
        if xbuf is None:
            xbuf = torch.empty(tuple(x_shape), device=dev, dtype=dtype)
            obuf = torch.empty(B, self._out_channels(), H, W, device=dev, dtype=dtype)
        assert tuple(xbuf.shape) == tuple(x_shape) and tuple(obuf.shape) == (B, self._out_channels(), H, W) and xbuf.is_contiguous() and obuf.is_contiguous() and xbuf.dtype == obuf.dtype == dtype
        io = UNetIO(x=xbuf, timestep=torch.empty(B, device=dev, dtype=torch.float32), out=obuf)
        if got["pooled"] is not None:
            io.pooled = torch.empty(B, got["pooled"].shape[1], device=dev, dtype=dtype)
            io.time_ids = torch.empty(B, got["time_ids"].shape[1], device=dev, dtype=torch.float32)
        if got.get("timesteps_all") is not None:  # CompiledSDXL: the solver's whole timestep list -> the timestep-embedding chain becomes a prologue table
            S = int(got["timesteps_all"].numel())
            io.timesteps = torch.empty(B * S, device=dev, dtype=torch.float32)
            io.step_rows = torch.zeros(B, device=dev, dtype=torch.int32)
            self.rows_table = (torch.arange(B, dtype=torch.int32).unsqueeze(0) * S + torch.arange(S, dtype=torch.int32).unsqueeze(1)).to(dev)  # [S, B]: b*S + s
        for ck, v in got["tokens"].items():
            assert v.shape[0] == B, f"context {ck} has batch {v.shape[0]}, latents have {B}"
            L, width = v.shape[1], v.shape[2]
            lp = (L + 63) // 64 * 64
            io.tokens[ck] = (torch.zeros(B * lp, width, device=dev, dtype=dtype), L)
        for name, v in got["conditions"].items():
            io.conditions[name] = torch.empty(tuple(v.shape), device=dev, dtype=dtype)
        for name, feats in got.get("t2i", {}).items():
            io.t2i[name] = [torch.empty(tuple(f.shape), device=dev, dtype=dtype) for f in feats]
        if got.get("guide") is not None:
            io.guide = torch.empty(tuple(got["guide"].shape), device=dev, dtype=dtype)
        low = UNetLowering(dev, dtype, self.cache, self.lora_mode)
        low.sag_capture = getattr(self, "sag_capture", True)
        low.style_half_batch = self.io_override is not None  # StyleAligned: this program is ONE half of the CFG pair, all its rows share row 0
        self.style_watch = low.style_modules  # (filled while lowering; kept when it raises Unsupported)
        try:
            low.lower(self._tree(), io)
        finally:
            self.ro_watch = getattr(low, "ro_adapters", [])
        self.cache.sweep()
        # the step program is replayed step after step: let every GEMM / conv pull the weights of the launches behind it into
        # the Infinity Cache (weights are read exactly once per step, so otherwise every kernel starts on DRAM misses)
        pf = native.link_weight_prefetch(low.step, enable=self.weight_prefetch)
        self.low, self.io, self.graph, self.prologue_key, self.prologue_refs = low, io, None, None, None
        from . import tuning

        self.lowerings += 1
        self.stats = dict(low.stats, step_ops=launches(low.step), prologue_ops=launches(low.prologue), pool_bytes=low.step_pool.bytes() + low.prologue_pool.bytes(),
                          weight_prefetch=pf, gemm_tuning=tuning.summary(), ln_fuse=low.ln_fuse, qkv_merge=low.qkv_merge,
                          lowerings=self.lowerings, prologue_runs=self.prologue_runs)

    def _out_channels(self) -> int:
        last = [m for m in self.unet.modules() if isa(m, "Conv2d")][-1]
        return last.out_channels

    def _stage_inputs(self, got: dict[str, Any]) -> bool:
        """Copy the user's side inputs into the static buffers; returns True when a prompt-side input changed."""
        io = self.io
        assert io is not None
        ts = got["timestep"].to(device=io.timestep.device, dtype=torch.float32).reshape(-1)
        io.timestep.copy_(ts.expand(io.timestep.shape[0]) if ts.numel() == 1 else ts)
        if io.step_rows is not None:
            io.step_rows.copy_(self.rows_table[int(got["step_index"])])
        if io.guide is not None:
            io.guide.copy_(got["guide"])
        lcm = getattr(self.low, "lcm_scale", None)  # SDXLLcmAdapter's condition scale: a prologue input (UNetLowering._fold_condition_scale)
        pk = (_ident(got.get("timesteps_all")), _ident(got["pooled"]), _ident(got["time_ids"]), tuple(_ident(v) for v in got["tokens"].values()), tuple(_ident(v) for v in got["conditions"].values()),
              tuple(_ident(f) for feats in got.get("t2i", {}).values() for f in feats), None if lcm is None else lcm())
        if pk == self.prologue_key:
            return False
        if io.pooled is not None:
            io.pooled.copy_(got["pooled"])
            io.time_ids.copy_(got["time_ids"])  # type: ignore[union-attr]
        if io.timesteps is not None:
            B = io.timestep.shape[0]
            io.timesteps.view(B, -1).copy_(got["timesteps_all"].to(device=io.timesteps.device, dtype=torch.float32).reshape(1, -1).expand(B, -1))
        for ck, v in got["tokens"].items():
            buf, L = io.tokens[ck]
            B = v.shape[0]
            buf.view(B, -1, v.shape[2])[:, :L].copy_(v)
        for name, v in got["conditions"].items():
            io.conditions[name].copy_(v)
        for name, feats in got.get("t2i", {}).items():
            for buf, f in zip(io.t2i[name], feats):
                buf.copy_(f)
        self.prologue_key = pk
        self.prologue_refs = (got.get("timesteps_all"), got["pooled"], got["time_ids"], tuple(got["tokens"].values()), tuple(got["conditions"].values()),
                              tuple(f for feats in got.get("t2i", {}).values() for f in feats))
        return True

    # -- execution ---------------------------------------------------------------------------------------------
    def prepare(self, x: Tensor) -> bool:
        """Make sure a program matching the tree and the input geometry exists and its inputs are staged (inputs taken
        from the UNet's context store, as refiners' pipeline leaves them)."""
        got = self._gather()
        changed = self.prepare_explicit(tuple(x.shape), x.device, got)
        self.io.x.copy_(x)  # type: ignore[union-attr]
        return changed

    def _tree_state(self) -> Any:
        """What invalidates a lowered program.  Trees built from refiners_amd.fluxion bump a global epoch on every
        structural change and scale assignment; trees built from refiners' own classes have no such counter, so their
        state is a signature of the module identities and the live scales (a ~1 ms walk per call)."""
        from ..fluxion.tree import Chain as MirrorChain

        if isinstance(self.unet, MirrorChain):
            ep = tree_epoch()
            return (ep, _weights_version(self.unet, self.__dict__.setdefault("_params_cache", {}), ep))
        sig: list[Any] = [_weights_version(self.unet)]
        for m in self.unet.modules():
            sig.append(id(m))
            if isa(m, "Multiply", "T2IFeatures"):  # nodes whose live scale is baked into the program
                sig.append(float(m.scale))
            if isa(m, "Controlnet"):
                sig.extend([float(m.scale), float(m.scale_decay)])
        return hash(tuple(sig))

    def prepare_explicit(self, x_shape: tuple, device: torch.device, got: dict[str, Any]) -> bool:
        """Same, with the side inputs given explicitly: {"timestep", "pooled", "time_ids", "tokens": {(ctx, key): t},
        "conditions": {ctx_name: t}}.  Does not stage x (the caller fills io.x).  Returns True when the prologue must run."""
        key = (self._tree_state(), tuple(x_shape), self.unet.dtype, None if got.get("timesteps_all") is None else int(got["timesteps_all"].numel()),
               tuple((k, tuple(v.shape)) for k, v in got["tokens"].items()),
               tuple((k, tuple(v.shape)) for k, v in got["conditions"].items()), got["pooled"] is not None,
               tuple((k, tuple(tuple(f.shape) for f in feats)) for k, feats in got.get("t2i", {}).items()), self.io_override is not None,
               None if got.get("guide") is None else tuple(got["guide"].shape))
        if key == self.bad_key and self.bad_values != self._live_values():
            self.bad_key = None  # a StyleAligned scale was assigned since the refusal: look at the tree again
        if key != self.key:
            if key == self.bad_key:
                raise Unsupported(self.stats.get("whole_fallback", "this tree could not be lowered"))
            try:
                self._build(x_shape, device, got)
            except Unsupported as exc:
                # remembered per (tree state, geometry): the next call does not walk the tree again; any inject / eject / scale change retries
                # (StyleAligned scales and reference-only style_cfg bump no epoch: they are compared by value, see bad_values)
                self.bad_key, self.key, self.low, self.io, self.graph = key, None, None, None, None
                self.bad_values = self._live_values()
                self.stats = {"whole_fallback": str(exc), "fallback_nodes": ["<whole UNet>"], "step_ops": 0, "prologue_ops": 0}
                warnings.warn(f"refiners_amd: this UNet tree is not lowered to the MI355X kernels ({exc}); running the stock Chain forward instead", RuntimeWarning, stacklevel=3)
                raise
            self.key, self.bad_key = key, None
        self._refresh_style_scale(key)
        return self._stage_inputs(got)

    def _live_values(self) -> tuple:
        return tuple(float(m.scale) for m in self.style_watch) + tuple(float(m.style_cfg) for m in self.ro_watch)

    def _refresh_style_scale(self, key: Any) -> None:
        """StyleAligned's scale is a live attribute of the tree and the step is a captured graph: the kernels read it from one float in device
        memory, rewritten here (on the replaying stream, in front of the replay) whenever the tree's value moved.  The lowered pattern has ONE
        scale; a tree whose ScaleReferenceFeatures were set apart by hand is no longer that pattern and is refused like any other tree the
        lowering does not know (stock forward behind the warning, retried once the scales change again)."""
        low = self.low
        if low is not None and low.ro_mix is not None:  # reference-only control: the same arrangement for `style_cfg` (ro_mix = [style_cfg, 1])
            cfgs = {float(m.style_cfg) for m in low.ro_adapters}
            if len(cfgs) != 1:
                self._refuse(key, "the self-attention injections of one UNet carry different style_cfg")
            v = cfgs.pop()
            if v != low.ro_mix_value:
                low.ro_mix[:1].fill_(v)
                low.ro_mix_value = v
        if low is None or not low.style_modules:
            return
        vals = set(float(m.scale) for m in self.style_watch)
        if len(vals) != 1:
            self._refuse(key, "the StyleAligned layers carry different scales")
        v = vals.pop()
        if v != low.style_scale_value:
            low.style_scale.fill_(v)
            low.style_scale_value = v

    def _refuse(self, key: Any, why: str) -> None:
        """A live attribute moved the tree out of the lowered pattern: the stock forward behind the warning, retried once the values change again."""
        self.bad_key, self.key, self.low, self.io, self.graph = key, None, None, None, None
        self.bad_values = self._live_values()
        self.stats = {"whole_fallback": why, "fallback_nodes": ["<whole UNet>"], "step_ops": 0, "prologue_ops": 0}
        warnings.warn(f"refiners_amd: this UNet tree is not lowered to the MI355X kernels ({why}); running the stock Chain forward instead", RuntimeWarning, stacklevel=5)
        raise Unsupported(why)

    def run_prologue(self) -> None:
        assert self.low is not None
        native.replay(self.low.prologue)
        self.prologue_runs += 1
        self.stats["prologue_runs"] = self.prologue_runs
        self.check_handovers()  # once per prompt: a host round trip here is nothing next to the prologue's ~290 launches

    CHECK_EVERY = 16  # replays of the step program between two looks at the hand-over error words (one stacked .any() + one host sync)

    def check_handovers(self, every: int = 1) -> None:
        """The in-launch LoRA hand-over and the stream-K collect are bounded waits: a tile that gives up after 2 s raises an error word in device
        memory and goes on with undefined operands (a trap would kill the process's HIP context).  Nothing on the device can raise into Python, so
        the engine looks at those words at its host sync points -- after the prologue, every CHECK_EVERY-th step replay (`every`), at the end of a
        sampling run -- and turns a raised word into NativeError (round-5 advisor: until round 6 only the tests looked)."""
        self._replays = getattr(self, "_replays", 0) + 1
        if self.low is None or self._replays % max(every, 1):
            return
        bad = self.low.handover_pending()
        if bad and bool((bad[0] if len(bad) == 1 else torch.stack(bad).any()).item()):
            self.low.handover_raise()

    def run_step(self) -> None:
        """Replay the per-step program (directly the first time, as a HIP graph afterwards)."""
        assert self.low is not None
        if not self.use_graph:
            native.replay(self.low.step)
            return
        if self.graph is None:
            native.replay(self.low.step)  # warm-up: first-launch work (function attributes, workspace) must not be captured
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                native.replay(self.low.step)
            self.graph = g
            return
        self.graph.replay()

    @torch.no_grad()
    def __call__(self, x: Tensor) -> Tensor:
        try:
            changed = self.prepare(x)
        except Unsupported:
            return self.unet(x)  # the stock child loop: reads the same context store, resets it itself (chain.py:245-257)
        if changed:
            self.run_prologue()
        self.check_handovers(self.CHECK_EVERY)  # (looks at what the PREVIOUS replays left: no wait for this one)
        self.run_step()
        assert self.io is not None
        self.unet._reset_context()  # what Chain.forward does after running its children (chain.py:256)
        return self.io.out.clone()


class CompiledSDXL:
    """One classifier-free-guidance denoising step per call: UNet on cat(x, x) + CFG combine + solver update
    (reference latent_diffusion/model.py:128-159, solvers/ddim.py:56-95), latents resident in HBM across steps.

    `solver`: None = DDIM over `num_inference_steps` (SDXL's default); or an `Euler` / `DPMSolver` of
    refiners_amd.latent_diffusion.solvers (anything with `linear_step`): guidance + update + the next step's model-input
    scaling then run as ONE kernel (mi355x_cfg_linear_step) and the two cat(x, x) copies disappear from the step.
    SD1.5 UNets work too: leave `pooled_text_embedding` / `time_ids` out of `set_inputs`.
    A stochastic `DPMSolver` (`sde_variance=1.0`) ends its step in mi355x_cfg_sde_step / mi355x_sde_step, the same update with the step's Gaussian
    draw as a fifth operand.  The draw is made per step BEFORE the graph is replayed, from `set_inputs`' generator, into a buffer the graph reads.

    `classifier_free_guidance=False` (the reference's `sdxl.classifier_free_guidance = False`, model.py:128-159: LCM, LCM-LoRA, SDXL-Lightning):
    the UNet runs on x alone -- embeddings of n rows, a program lowered for (n, C, H, W) -- and the update is mi355x_ddim_step /
    mi355x_linear_step, the same arithmetic with eps = the UNet's output.  `condition_scale` and `cfg_split` are then ignored and an injected
    SAG adapter gets no second pass (the reference evaluates it inside the CFG branch only).  It is a live attribute: assigning it drops the
    captured graph and the priming state, as assigning `solver` does.

    The per-step host work is: two tiny device copies (timestep, solver coefficients) and one hipGraphLaunch.  The Chain
    tree's context store is not touched per step (the reference spends ~19 000 Python calls per step on it)."""

    def __init__(self, unet: Any, num_inference_steps: int = 50, condition_scale: float = 5.0, use_graph: bool = True, lora_mode: str = "fused",
                 solver: Any = None, cfg_split: Optional[bool] = None, classifier_free_guidance: bool = True) -> None:
        from ..latent_diffusion.sampling import DDIM

        self.unet = unet
        self.engine = CompiledUNet(unet, use_graph=False, lora_mode=lora_mode)
        # cfg_split: the two halves of the classifier-free-guidance pair never meet before the guidance kernel (model.py:128-159 runs them as one
        # batch only because that is one module call), so they are lowered as TWO batch-n programs and replayed on two streams -- two branches of
        # the one captured HIP graph.  At one image per GPU every launch of the pair is short of workgroups (M = 2048 rows: 160 tiles on 256 CUs)
        # and a third of the step is fill / epilogue / launch boundary; two independent launch sequences fill each other's gaps.
        # None = REFINERS_AMD_CFG_SPLIT (default: see _split_wanted).  Self-Attention Guidance keeps the single program (its tap reads both halves).
        self.cfg_split = cfg_split if cfg_split is not None else {"0": False, "1": True}.get(os.environ.get("REFINERS_AMD_CFG_SPLIT", ""), None)
        self.engine_c: Optional[CompiledUNet] = None  # split mode: the conditional half (self.engine then runs the negative half)
        self.pair_x: Optional[Tensor] = None  # split mode: [2n, C, H, W] model input / UNet output, halves owned by the two engines
        self.pair_out: Optional[Tensor] = None
        self.side_stream: Optional[torch.cuda.Stream] = None
        self.use_graph = use_graph
        self.coef_table: Optional[Tensor] = None
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.solver = solver if solver is not None else DDIM(num_inference_steps)
        self.hist: Optional[Tensor] = None
        self.primed, self.primed_key = False, None
        self._condition_scale = condition_scale
        self._cfg = bool(classifier_free_guidance)
        self._inputs_guided: Optional[bool] = None  # the mode the staged inputs were given in (see the classifier_free_guidance setter)
        self.x: Optional[Tensor] = None
        self.graph_key: Any = None
        self.inputs: dict[str, Any] = {}
        self.engine2: Optional[CompiledUNet] = None  # self-attention guidance: the second (unconditional, batch n) UNet pass
        # step-constant UNet input channels (inpainting: mask + masked-image latents, IC-Light: the condition latents): an engine-owned buffer at a
        # stable address, [1 or n, E, h, w]; the UNet then reads (2n or n, 4 + E, h, w) and x stays (n, 4, h, w)
        self.cond: Optional[Tensor] = None
        self.in_scale: Optional[Tensor] = None  # one float32 on the device: the solver's input scale of the step that primes the model input
        self.sde_noise: Optional[Tensor] = None

    @property
    def condition_scale(self) -> float:
        return self._condition_scale

    @condition_scale.setter
    def condition_scale(self, value: float) -> None:  # baked into the device coefficient table: rebuild it on the next set_inputs / step
        self._condition_scale = value
        self.coef_table = None
        self.graph = None  # self-attention guidance bakes sag.scale / condition_scale into the captured launches as a host scalar

    @property
    def classifier_free_guidance(self) -> bool:
        return self._cfg

    @classifier_free_guidance.setter
    def classifier_free_guidance(self, value: bool) -> None:  # another batch (n against 2n rows), another update kernel
        if bool(value) != self._cfg:
            self._cfg = bool(value)
            self.graph, self.graph_key = None, None
            self.primed, self.primed_key = False, None

    @property
    def solver(self) -> Any:
        return self._solver

    @solver.setter
    def solver(self, value: Any) -> None:
        self._solver = value
        self.linear = hasattr(value, "linear_step")
        # SDE DPM-Solver++: nine-column rows, the draw in a buffer of its own (LCM's `needs_noise` lends it the history slot; this update keeps its history)
        self.sde = self.linear and float(getattr(value, "sde_variance", 0.0) or 0.0) != 0.0
        self.coef_table, self.graph = None, None  # other coefficients, possibly another update kernel

    def _tables(self, device: torch.device) -> None:
        rows = []
        # a DDIM whose `timesteps` were replaced (Restart sampling: fewer timesteps than num_inference_steps) takes len(timesteps) - 1 steps, each
        # towards the next timestep; `coefficients` compares the step with num_inference_steps as the reference does
        steps = self.solver.num_inference_steps
        if not self.linear and len(self.solver.timesteps) != steps:
            steps = len(self.solver.timesteps) - 1
        for s in range(steps):
            if self.linear:
                rows.append([self.condition_scale, *self.solver.linear_step(s)])
            else:
                cur, sig, prev, nf = self.solver.coefficients(s)
                rows.append([self.condition_scale, cur, sig, prev, nf, 0.0, 0.0, 0.0])
        self.coef_table = torch.tensor(rows, dtype=torch.float32, device=device)
        self.coef = torch.zeros(self.coef_table.shape[1], dtype=torch.float32, device=device)  # (nine floats for the SDE form; the other kernels read eight)
        # a solver whose input scale is 1 at every step (DDIM, DPM-Solver++, LCM) leaves the constant input channels as priming wrote them; Euler's
        # are rescaled by every step's last launch (mi355x_cond_step with the constants given)
        self.scales_input = self.linear and any(float(self.solver.input_scale(s)) != 1.0 for s in range(self.solver.num_inference_steps))
        self.in_scale = torch.ones(1, dtype=torch.float32, device=device)
        self.ts_table = self.solver.timesteps.to(device=device, dtype=torch.float32)
        if 0 < steps < self.solver.num_inference_steps and self.ts_table.numel() < self.solver.num_inference_steps:
            # (a Restart segment: padded to the trajectory's length, which is what sizes the lowered program's timestep-embedding table --
            # the segment then runs on the caller's program and buffers, and the caller's captured graph stays valid)
            self.ts_table = torch.cat((self.ts_table, self.ts_table[-1:].expand(self.solver.num_inference_steps - self.ts_table.numel())))
        # Self-Attention Guidance degrades the latents through Solver.remove_noise / add_noise: (-, scale_t, std_t) per step, for mi355x_sag_degrade.
        # A solver whose add_noise / remove_noise the reference itself cannot evaluate (Euler: float timesteps) has no table; SAG then raises.
        # The one refusal that is the reference's own: a solver whose timesteps are floats (Euler) cannot index the integer train-time tables
        # in add_noise / remove_noise -- torch raises IndexError there too.  Anything else (a solver without the method, a bug in its tables)
        # propagates instead of being turned into "no SAG" (round-3 advisor finding).
        ts = self.solver.timesteps
        if not hasattr(self.solver, "sag_coefficients") or (torch.is_tensor(ts) and ts.is_floating_point()):
            self.sag_table = None
        else:
            try:
                self.sag_table = torch.tensor([[0.0, *self.solver.sag_coefficients(s)] for s in range(steps)], dtype=torch.float32, device=device)
            except IndexError:  # the mirror's Euler refuses for every spacing (its trailing timesteps are integers, but that combination has no golden yet)
                self.sag_table = None
        self.sag_coef = torch.zeros(3, dtype=torch.float32, device=device)

    def set_inputs(self, x: Tensor, *, clip_text_embedding: Tensor, pooled_text_embedding: Optional[Tensor] = None, time_ids: Optional[Tensor] = None,
                   clip_image_embedding: Optional[Tensor] = None, conditions: Optional[dict[str, Tensor]] = None,
                   t2i_features: Optional[dict[str, Any]] = None, generator: Optional[torch.Generator] = None, llm_text_embedding: Optional[Tensor] = None,
                   input_condition: Optional[Tensor] = None) -> None:
        """x: (N, 4, H, W) initial latents; embeddings are [negative ; conditional] stacks of 2N rows;
        `conditions` maps a ControlLora name to its control image, (2N, 3, 8H, 8W) or ONE picture (1, 3, 8H, 8W) for the whole batch; `t2i_features` maps a T2I-Adapter name to
        the tuple its `compute_condition_features` returned (batch 1 or 2N); `llm_text_embedding` (2N, T, width): the LLM's token embeddings an injected ELLA adapter reads
        (ELLAAdapter.set_llm_text_embedding).
        With `classifier_free_guidance=False` there is no negative half: embeddings have N rows, pictures and features 1 or N.
        `input_condition` (1 or N, E, H, W): the channels the UNet reads BEHIND the latents and that do not change over a trajectory -- inpainting's
        cat(mask_latents, target_image_latents), IC-Light's condition latents.  x stays (N, 4, H, W); the UNet's first convolution must read 4 + E
        channels.  New values of the same shape keep the lowered program and the captured graph (the model input is primed again); another shape
        or leaving it out drops the graph."""
        if not self._cfg:
            n = x.shape[0]
            for what, t in (("clip_text_embedding", clip_text_embedding), ("pooled_text_embedding", pooled_text_embedding), ("time_ids", time_ids),
                            ("clip_image_embedding", clip_image_embedding), ("llm_text_embedding", llm_text_embedding)):
                assert t is None or t.shape[0] == n, f"classifier_free_guidance=False: {what} has {t.shape[0]} rows, the latents have {n} (no [negative ; conditional] stack)"
            for what, t in [(k, v) for k, v in (conditions or {}).items()] + [(k, f) for k, feats in (t2i_features or {}).items() for f in feats]:
                assert t.shape[0] in (1, n), f"classifier_free_guidance=False: condition '{what}' has {t.shape[0]} rows, expected 1 or {n}"
        self._inputs_guided = self._cfg
        self.generator = generator  # stochastic solvers (LCM) draw their per-step noise from it, in the reference's order
        tokens = {("cross_attention_block", "clip_text_embedding"): clip_text_embedding}
        if clip_image_embedding is not None:
            tokens[("ip_adapter", "clip_image_embedding")] = clip_image_embedding
        if llm_text_embedding is not None:
            tokens[("adapted_cross_attention_block", "llm_text_embedding")] = llm_text_embedding
        self.inputs = {"pooled": pooled_text_embedding, "time_ids": time_ids, "tokens": tokens,
                       # ("controlnet.condition_<name>": the picture of an SD1.5 Controlnet, under the context and key its adapter reads)
                       "conditions": {(k if k.startswith("controlnet.") else f"control_lora_{k}"): v for k, v in (conditions or {}).items()},
                       "t2i": {k: tuple(v) for k, v in (t2i_features or {}).items()}}
        if self.x is None or self.x.shape != x.shape or self.x.device != x.device or self.x.dtype != self.unet.dtype:
            self.x = torch.empty(tuple(x.shape), device=x.device, dtype=self.unet.dtype)
            # the solver history lives as long as x does: a captured graph holds both addresses, so neither may be
            # re-allocated per trajectory (a fresh zeros_like() here left the graph reading / writing a freed block)
            self.hist = torch.zeros_like(self.x)
            self.sde_noise = torch.zeros_like(self.x)  # the per-step draw of a stochastic solver (and Restart's): the same lifetime, for the same reason
            self.graph = None
        self.x.copy_(x)
        if input_condition is None:
            if self.cond is not None:
                self.cond, self.graph = None, None
        else:
            assert input_condition.dim() == 4 and input_condition.shape[0] in (1, x.shape[0]) and tuple(input_condition.shape[2:]) == tuple(x.shape[2:]), (
                f"input_condition is {tuple(input_condition.shape)}: expected (1 or {x.shape[0]}, E, {x.shape[2]}, {x.shape[3]}) beside latents {tuple(x.shape)}")
            if self.cond is None or self.cond.shape != input_condition.shape or self.cond.device != x.device or self.cond.dtype != self.unet.dtype:
                self.cond = torch.empty(tuple(input_condition.shape), device=x.device, dtype=self.unet.dtype)
                self.graph = None  # the captured launches hold the buffer's address
            self.cond.copy_(input_condition)
        if self.linear or not self._cfg or self.cond is not None:
            assert self.hist is not None
            self.hist.zero_()
            self.primed = False  # the model-input buffer must be (re)filled with s_0 * x (and s_0 * the constant channels) before the next step
        if self.coef_table is None or self.coef_table.device != x.device:
            self._tables(x.device)

    # -- the CFG pair as two programs on two streams -----------------------------------------------------------------------------
    # default policy: never.  Measured at one image per GPU (profiles/r06_a_ab_cfg_split.log, r06_b_ab_cfg_split_lead.log): 26.1 ms against 25.2-25.4 ms for the
    # single program, with the tuning table's choices carried over to the halved shapes and with one half running 3 / 5 / 40 launches ahead of the other --
    # two identical launch sequences pair equal kernels, and a launch that leaves CUs idle leaves them idle in both.  Kept as an option (and as the
    # two-concurrent-programs test of the engine): `cfg_split=True` / REFINERS_AMD_CFG_SPLIT=1.
    SPLIT_MAX_IMAGES = 0

    def _split_wanted(self, n: int) -> bool:
        if not self._cfg or self._sag_adapter() is not None or self.x is None or self.x.device.type != "cuda" or self.cond is not None:
            return False  # (step-constant input channels keep the single program, as Self-Attention Guidance does)
        if self.cfg_split is None and self.engine.reference_only():
            return False  # reference-only control blends row 0 of the pair with the guide's keys: one program (an explicit cfg_split=True is refused by the lowering)
        return self.cfg_split if self.cfg_split is not None else n <= self.SPLIT_MAX_IMAGES

    def _split_got(self, got: dict[str, Any], n: int) -> tuple[dict[str, Any], dict[str, Any]]:
        """[negative ; conditional] stacks -> (negative rows, conditional rows).  The views are made once per set_inputs: a fresh view per step
        would look like a new prompt to the engines (_ident keys on id()) and re-run their prologues every step."""
        cached = getattr(self, "_pair_halves", None)
        if cached is None or cached[0] is not self.inputs:
            def cut(t: Any, h: int) -> Any:
                if t is None or t.shape[0] != 2 * n:  # ONE control picture / feature set for the whole batch broadcasts into both halves
                    return t
                return t[h * n : (h + 1) * n]

            sides = []
            for h in (0, 1):
                sides.append({"pooled": cut(got["pooled"], h), "time_ids": cut(got["time_ids"], h), "tokens": {k: cut(v, h) for k, v in got["tokens"].items()},
                              "conditions": {k: cut(v, h) for k, v in got["conditions"].items()},
                              "t2i": {k: tuple(cut(f, h) for f in feats) for k, feats in got.get("t2i", {}).items()}})
            cached = (self.inputs, sides)
            self._pair_halves = cached
        rest = {"timestep": got["timestep"], "timesteps_all": got.get("timesteps_all"), "step_index": got.get("step_index", 0)}
        return {**rest, **cached[1][0]}, {**rest, **cached[1][1]}

    def _prepare_pair(self, got: dict[str, Any], n: int) -> tuple[bool, bool]:
        """Both halves lowered / staged; (negative prologue must run, conditional prologue must run).  Raises Unsupported like prepare_explicit."""
        x = self.x
        assert x is not None
        eu = self.engine
        if self.engine_c is None:
            self.engine_c = CompiledUNet(self.unet, use_graph=False, lora_mode=eu.lora_mode)
            self.engine_c.cache = eu.cache  # one set of packed weights for both programs
        ec = self.engine_c
        shape2 = (2 * n,) + tuple(x.shape[1:])
        if self.pair_x is None or tuple(self.pair_x.shape) != shape2 or self.pair_x.device != x.device or self.pair_x.dtype != self.unet.dtype:
            self.pair_x = torch.empty(shape2, device=x.device, dtype=self.unet.dtype)
            self.pair_out = torch.empty((2 * n, eu._out_channels()) + tuple(x.shape[2:]), device=x.device, dtype=self.unet.dtype)
            eu.key = ec.key = None  # the programs hold the old buffers' addresses
        assert self.pair_out is not None
        eu.io_override, ec.io_override = (self.pair_x[:n], self.pair_out[:n]), (self.pair_x[n:], self.pair_out[n:])
        gu, gc = self._split_got(got, n)
        shape1 = (n,) + tuple(x.shape[1:])
        cu = eu.prepare_explicit(shape1, x.device, gu)
        cc = ec.prepare_explicit(shape1, x.device, gc)
        if self.side_stream is None:
            self.side_stream = torch.cuda.Stream(device=x.device)
        return cu, cc

    def _replay_pair(self) -> None:
        """The conditional half on the side stream beside the negative half on the current one (under capture: two branches of the graph)."""
        cur, side = torch.cuda.current_stream(), self.side_stream
        assert side is not None and self.engine.low is not None and self.engine_c is not None and self.engine_c.low is not None
        lead = int(os.environ.get("REFINERS_AMD_CFG_SPLIT_LEAD", "0"))  # launches the current stream's half runs ahead of the other (probing: two identical sequences in lockstep pair equal kernels)
        ops = self.engine.low.step
        if lead > 0:
            native.replay(ops[:lead])
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            native.replay(self.engine_c.low.step)
        native.replay(ops[lead:] if lead > 0 else ops)
        cur.wait_stream(side)

    def _split_step(self, step: int, got: dict[str, Any], n: int) -> Tensor:
        from types import SimpleNamespace

        try:
            cu, cc = self._prepare_pair(got, n)
        except Unsupported:
            return self._stock_step(step, got)
        eu, ec = self.engine, self.engine_c
        assert ec is not None and self.x is not None
        if cu:
            eu.run_prologue()
        if cc:
            ec.run_prologue()
        eu.check_handovers(eu.CHECK_EVERY)
        ec.check_handovers(ec.CHECK_EVERY)
        self.coef.copy_(self.coef_table[step])
        io = SimpleNamespace(x=self.pair_x, out=self.pair_out)
        gkey = ("pair", eu.key, ec.key)
        if self.linear:
            return self._linear_step(step, io, None, eu, None, gkey, run=self._replay_pair)
        return self._guided_ddim_step(io, self._replay_pair, None, gkey)

    def _guided_ddim_step(self, io: Any, run: Any, tail: Any, gkey: Any) -> Tensor:
        """Guided DDIM without step-constant channels: copy x into both halves of the model input, run the UNet program (`run`), the
        Self-Attention-Guidance pass if there is one (`tail`), and mi355x_cfg_ddim_step -- launched directly, or captured once per `gkey`."""
        assert self.x is not None

        def body(last: bool = True) -> None:
            self._fill(io)
            run()
            if tail is not None:
                tail()
            if last:
                native.cfg_ddim_step(self.x, io.out, self.coef)

        if not self.use_graph:
            body()
            return self.x
        if self.graph is None or self.graph_key != gkey:
            keep = self.x.clone()
            body(last=False)  # warm-up outside capture (first-launch attribute calls, workspaces)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            self.x.copy_(keep)
            self.graph, self.graph_key = g, gkey
        self.graph.replay()
        return self.x

    def lower_now(self) -> None:
        """Build the launch programs for the staged inputs without running anything (refiners_amd.parallel.broadcast_packs lowers on every
        rank but lets only the source compute the packed weights: the prologue must not run before they have arrived)."""
        assert self.x is not None, "call set_inputs first"
        if self.coef_table is None or self.coef_table.device != self.x.device:
            self._tables(self.x.device)
        n = self.x.shape[0]
        if self._split_wanted(n):
            try:
                self._prepare_pair(dict(self.inputs, timestep=self.ts_table[0:1], timesteps_all=self.ts_table, step_index=0), n)
            except Unsupported:
                return
            self.engine.prologue_key = None
            self.engine_c.prologue_key = None  # type: ignore[union-attr]
            return
        try:
            self.engine.prepare_explicit(self._model_shape(n), self.x.device, dict(self.inputs, timestep=self.ts_table[0:1], timesteps_all=self.ts_table, step_index=0))
        except Unsupported:
            return  # a tree this lowering does not know: nothing to stage, step() takes the stock Chain forward with its warning (the fallback contract)
        self.engine.prologue_key = None  # staged, not yet run: the first step() re-stages and runs the prologue

    def _model_shape(self, n: int, rows: Optional[int] = None) -> tuple:
        """The UNet's input: the CFG pair (or x alone) with the step-constant channels behind the latents'."""
        x = self.x
        assert x is not None
        E = 0 if self.cond is None else self.cond.shape[1]
        return (rows if rows is not None else (2 * n if self._cfg else n), x.shape[1] + E) + tuple(x.shape[2:])

    def _check_stem(self) -> None:
        """The UNet's first convolution must read the latents' channels plus the condition's."""
        from .packing import cname

        x = self.x
        assert x is not None
        down = next((m for m in kids(self.engine._tree()) if cname(m) == "DownBlocks"), None)
        conv = None if down is None else next((m for m in down.modules() if isa(m, "Conv2d")), None)
        if conv is not None and self.cond is not None:
            E = self.cond.shape[1]
            assert conv.in_channels == x.shape[1] + E, (
                f"the UNet's first convolution reads {conv.in_channels} channels, the latents have {x.shape[1]} and input_condition {E}: {x.shape[1]} + {E} != {conv.in_channels}")

    def _fill(self, io: Any = None) -> None:
        io = io if io is not None else self.engine.io
        n = self.x.shape[0]  # type: ignore[union-attr]
        if self.cond is not None:  # latents and constants into both halves, scaled by the priming step's input scale (set by the caller)
            native.cond_fill(self.x, self.cond, io.x, self.in_scale, n, self.x.shape[1])  # type: ignore[union-attr]
            return
        io.x[:n].copy_(self.x)  # type: ignore[union-attr]
        if self._cfg:
            io.x[n:].copy_(self.x)  # type: ignore[union-attr]

    def _update(self, io: Any) -> None:
        """The step's last launch: (guidance +) solver update + history + the next step's model input."""
        if self.cond is not None:
            native.cond_step(self.x, io.out, self.hist, io.x, self.cond if self.scales_input else None, self.coef, self.linear, self._cfg)
            return
        name, operands = self._UPDATES[(self.sde, self.linear, self._cfg)]  # (guided DDIM is not here: _guided_ddim_step)
        getattr(native, name)(self.x, io.out, *(getattr(self, a) for a in operands), io.x, self.coef)

    #: (stochastic, linear, guided) -> the wrapper in `native` and the operands it takes between the UNet's output and the model input
    _UPDATES = {
        (True, True, True): ("cfg_sde_step", ("hist", "sde_noise")),
        (True, True, False): ("sde_step", ("hist", "sde_noise")),
        (False, True, True): ("cfg_linear_step", ("hist",)),
        (False, True, False): ("linear_step", ("hist",)),
        (False, False, False): ("ddim_step", ()),
    }

    @torch.no_grad()
    def step(self, step: int) -> Tensor:
        assert self.x is not None, "call set_inputs first"
        assert self._inputs_guided in (None, self._cfg), (
            "classifier_free_guidance was assigned after set_inputs: call set_inputs again (embeddings of "
            f"{'2n rows, [negative ; conditional]' if self._cfg else 'n rows'})")
        if self.coef_table is None or self.coef_table.device != self.x.device:
            self._tables(self.x.device)  # condition_scale / solver changed since the last call
        eng = self.engine
        if self.sde:  # combinations without a golden are not lowered (the precedent in latent_diffusion/solvers.py)
            assert self.cond is None, "a stochastic DPMSolver (sde_variance=1.0) with input_condition is not lowered: mi355x_cond_step has no noise operand"
            assert not self._cfg or self._sag_adapter() is None, "a stochastic DPMSolver (sde_variance=1.0) with Self-Attention Guidance is not lowered"
        got = dict(self.inputs, timestep=self.ts_table[step : step + 1], timesteps_all=self.ts_table, step_index=step)
        if eng.reference_only():  # the guide is noised per step by the caller (ReferenceOnlyControlAdapter.set_controlnet_condition): read on every call
            got["guide"] = eng._contexts().get("reference_only_control", {}).get("guide")
        n = self.x.shape[0]
        if self._split_wanted(n):
            return self._split_step(step, got, n)
        eng.io_override = None
        eng.sag_capture = self._cfg  # (no guidance, no Self-Attention Guidance: the tap's column mass would be computed and never read)
        shape2 = self._model_shape(n)
        self._check_stem()
        try:
            changed = eng.prepare_explicit(shape2, self.x.device, got)
        except Unsupported:
            return self._stock_step(step, got)
        if changed:
            eng.run_prologue()
        eng.check_handovers(eng.CHECK_EVERY)
        io, low = eng.io, eng.low
        assert io is not None and low is not None
        self.coef.copy_(self.coef_table[step])
        if not self._cfg:  # the UNet program on x alone, then mi355x_linear_step / mi355x_ddim_step (DDIM too keeps its model input primed: no copy per step)
            return self._linear_step(step, io, low, eng, None, ("free", eng.key) + self._cond_id())
        sag = self._sag_adapter()
        tail = None if sag is None else self._prepare_sag(sag, got, n, io, low, step)
        # everything a captured graph holds by value or by address: both programs, and for self-attention guidance the host-side ratio
        # sag.scale / condition_scale and the blur weights' tensor (kernel_size, sigma)
        gkey = (eng.key, None if self.engine2 is None or sag is None else (self.engine2.key, float(sag.scale) / float(self.condition_scale), int(sag.kernel_size), float(sag.sigma))) + self._cond_id()
        if self.linear or self.cond is not None:  # (with step-constant channels DDIM too keeps its model input primed: mi355x_cond_step writes the next one)
            return self._linear_step(step, io, low, eng, tail, gkey)
        return self._guided_ddim_step(io, lambda: native.replay(low.step), tail, gkey)

    def _cond_id(self) -> tuple:
        """What a captured graph holds of the step-constant channels: the buffer's address and shape, and whether the last launch rescales them."""
        return () if self.cond is None else ((self.cond.data_ptr(), tuple(self.cond.shape), self.scales_input),)

    # -- whole-tree fallback ------------------------------------------------------------------------------------------------------
    def _stock_step(self, step: int, got: dict[str, Any]) -> Tensor:
        """A tree the lowering refused (CompiledUNet.prepare_explicit warned and recorded why): the step runs like the reference's
        `LatentDiffusionModel.forward` (latent_diffusion/model.py:128-159) -- contexts set on the tree, `unet(cat(x, x))` through the stock
        child loop -- and only the guidance + solver update stays on the native kernel."""
        assert not self._cfg or self._sag_adapter() is None, "Self-Attention Guidance on a tree that is not lowered: use refiners' own pipeline"
        unet, x = self.unet, self.x
        assert x is not None
        unet.set_timestep(got["timestep"])
        for (ctx, key), v in got["tokens"].items():
            unet.set_context(ctx, {key: v.to(x.dtype)})
        if got.get("pooled") is not None:
            unet.set_pooled_text_embedding(got["pooled"].to(x.dtype))
            unet.set_time_ids(got["time_ids"])
        for name, v in got.get("conditions", {}).items():
            ctx, _, key = name.partition(".")
            unet.set_context(ctx, {key or "condition": v.to(x.dtype)})
        for name, feats in got.get("t2i", {}).items():
            unet.set_context("t2iadapter", {f"condition_features_{name}": tuple(f.to(x.dtype) for f in feats)})
        self.coef.copy_(self.coef_table[step])
        # the extended input, as StableDiffusion_1_Inpainting.forward / ICLight build it: cat along the channels in front of the CFG pair
        xm = x if self.cond is None else torch.cat((x, self.cond.expand(x.shape[0], -1, -1, -1)), dim=1)
        xin = torch.cat((xm, xm)) if self._cfg else xm
        if not self.linear:
            if self._cfg:
                native.cfg_ddim_step(x, unet(xin).contiguous(), self.coef)
            else:
                native.ddim_step(x, unet(xin).contiguous(), None, self.coef)
            return x
        assert self.hist is not None
        if getattr(self.solver, "needs_noise", None) is not None and self.solver.needs_noise(step):
            noise = torch.randn(tuple(x.shape), generator=getattr(self, "generator", None), device=getattr(self.solver, "device", x.device), dtype=getattr(self.solver, "dtype", x.dtype))
            self.hist.copy_(noise)
        s0 = float(self.solver.input_scale(step))
        y = unet(xin * s0 if s0 != 1.0 else xin).contiguous()
        if self.sde:
            (native.cfg_sde_step if self._cfg else native.sde_step)(x, y, self.hist, self._draw(getattr(self, "generator", None)), None, self.coef)
            return x
        (native.cfg_linear_step if self._cfg else native.linear_step)(x, y, self.hist, None, self.coef)  # (no model-input buffer: the next step scales its input itself)
        return x

    # -- self-attention guidance (xl/model.py:164-250) ---------------------------------------------------------------------------
    def _sag_adapter(self) -> Any:
        p = getattr(self.unet, "parent", None)
        while p is not None:
            if isa(p, "SAGAdapter"):
                return p
            p = getattr(p, "parent", None)
        return None

    def _prepare_sag(self, sag: Any, got: dict[str, Any], n: int, io: Any, low: Any, step: int) -> Any:
        """Stage the second UNet pass of Self-Attention Guidance and return the closure that runs between the CFG pass and the
        guidance + DDIM kernel: degraded latents (mask from the tapped attention's column mass, Gaussian blur, re-noising: one
        kernel) -> unconditional UNet pass on them (a second lowered program, batch n) -> cond += (sag / cfg) * (uncond - degraded),
        which makes the unchanged CFG kernel produce eps_cfg + sag_scale * (eps_uncond - eps_degraded)   (model.py:147-155)."""
        if self.sag_table is None:  # the reference raises the same way (Solver.remove_noise indexes integer tables with the solver's timesteps)
            raise IndexError(f"{type(self.solver).__name__}: add_noise / remove_noise are not defined for this solver's timesteps, so Self-Attention Guidance "
                             "cannot be evaluated (refiners raises here as well)")
        assert self.condition_scale != 0.0, "SAG with a zero guidance scale is not lowered"
        # ControlLora pictures / T2I-Adapter features stay in their contexts for the second pass (xl/model.py:186-246 swaps only the text, pooled,
        # time-id and image embeddings), which has n rows after the CFG pass's 2n: batch-1 conditions broadcast into both, anything else cannot be
        # added to the n-row stem -- torch raises RuntimeError in the reference (oracle/make_golden_sag.py --conditions), so does this
        for name, rows in [(k, v.shape[0]) for k, v in got["conditions"].items()] + [(k, f.shape[0]) for k, feats in got.get("t2i", {}).items() for f in feats]:
            if rows not in (1, n):
                raise RuntimeError(f"Self-Attention Guidance runs its second UNet pass on {n} row(s): condition '{name}' has {rows} rows and cannot be "
                                   "broadcast to it (give one picture / one set of features for the whole batch; refiners fails on this shape as well)")
        self.sag_coef.copy_(self.sag_table[step])
        assert getattr(low, "sag", None) is not None and getattr(low, "sag_shape", None) is not None, "SAG adapter present but its taps were not found in the lowered tree"
        if self.engine2 is None:
            self.engine2 = CompiledUNet(self.unet, use_graph=False, lora_mode=self.engine.lora_mode)
            self.engine2.sag_capture = False  # the reference recomputes (and discards) the attention map in this pass
        e2 = self.engine2
        # [negative ; conditional] stacks -> negative half.  The views are made once per set_inputs: a fresh view per step would look like a
        # new prompt to engine2 (_ident keys on id()) and re-run its whole prologue (text / image K, V projections) every step.
        halves = getattr(self, "_sag_halves", None)
        if halves is None or halves[0] is not self.inputs:
            half = lambda t: None if t is None else t[: t.shape[0] // 2]  # noqa: E731
            halves = (self.inputs, {"pooled": half(got["pooled"]), "time_ids": half(got["time_ids"]), "tokens": {k: half(v) for k, v in got["tokens"].items()}})
            self._sag_halves = halves
        got2 = {"timestep": got["timestep"], "timesteps_all": got.get("timesteps_all"), "step_index": got.get("step_index", 0), **halves[1],
                "conditions": got["conditions"], "t2i": got.get("t2i", {})}
        x = self.x
        if e2.prepare_explicit(self._model_shape(n, rows=n), x.device, got2):
            e2.run_prologue()
        io2, low2 = e2.io, e2.low
        ks, sigma = int(sag.kernel_size), float(sag.sigma)
        key = (ks, sigma, str(x.device))
        if getattr(self, "_sag_w1_key", None) != key:
            t = torch.linspace(-(ks - 1) * 0.5, (ks - 1) * 0.5, steps=ks, dtype=torch.float32)
            pdf = torch.exp(-0.5 * (t / sigma).pow(2))
            self._sag_w1, self._sag_w1_key = (pdf / pdf.sum()).to(x.device), key
        mass, (ah, aw) = low.sag["mass"], low.sag_shape
        assert ah * aw == low.sag["tokens"]
        ratio = float(sag.scale) / float(self.condition_scale)
        u, c = io.out[:n], io.out[n:]
        cond = self.cond
        if cond is not None and (getattr(self, "_sag_deg", None) is None or self._sag_deg.shape != x.shape or self._sag_deg.dtype != x.dtype or self._sag_deg.device != x.device):
            self._sag_deg = torch.empty_like(x)  # mi355x_sag_degrade writes contiguous latents; mi355x_cond_fill re-strides them in front of the constants
        deg = self._sag_deg if cond is not None else io2.x

        def tail() -> None:
            # x is the UNSCALED latent (model.py:146: the guidance sees x, not scale_model_input(x)), and so is what the second pass is fed
            native.sag_degrade(x, u, mass, (ah, aw), self.sag_coef, self._sag_w1, deg)
            if cond is not None:  # cat(degraded, constants), unscaled (stable_diffusion_1/model.py:288-333)
                native.cond_fill(deg, cond, io2.x, None, n, x.shape[1])
            native.replay(low2.step)
            native.axpby(u, ratio, c, 1.0, c)
            native.axpby(io2.out, -ratio, c, 1.0, c)

        return tail

    def _linear_step(self, step: int, io: Any, low: Any, eng: Any, tail: Any = None, gkey: Any = None, run: Any = None) -> Tensor:
        """Euler / DPM-Solver++ / LCM: the UNet program (then the Self-Attention Guidance pass, `tail`) then ONE kernel (guidance, update,
        history, next model input).  `run`: what replays the UNet (default: `low.step` on the current stream; the split CFG pair passes its own)."""
        gkey = gkey if gkey is not None else eng.key
        if run is None:
            run = lambda: native.replay(low.step)  # noqa: E731
        if tail is None:
            tail = lambda: None  # noqa: E731
        assert self.x is not None and self.hist is not None
        if getattr(self.solver, "needs_noise", None) is not None and self.solver.needs_noise(step):
            # LCMSolver re-noises the consistency estimate (solvers/lcm.py:143-150): same draw as the reference (shape, device,
            # dtype, generator), placed in the kernel's history slot whose coefficient is the next timestep's noise std
            # drawn where and as what the reference draws it (solvers/lcm.py:143-150: the SOLVER's device and dtype), so that the same
            # generator and seed give the same stream; then cast / moved into the history slot
            sdev = getattr(self.solver, "device", self.x.device)
            sdt = getattr(self.solver, "dtype", self.x.dtype)
            noise = torch.randn(tuple(self.x.shape), generator=getattr(self, "generator", None), device=sdev, dtype=sdt)
            self.hist.copy_(noise)
        if self.sde:
            self._draw(getattr(self, "generator", None))
        if not self.primed or self.primed_key != gkey:  # first step of a trajectory, or the engine re-lowered into new buffers
            s0 = float(self.solver.input_scale(step)) if self.linear else 1.0  # (DDIM does not scale its model input)
            if self.cond is not None:
                self.in_scale.fill_(s0)  # type: ignore[union-attr]  # mi355x_cond_fill reads it from the device
            self._fill(io)  # cat(x, x) (x alone without guidance) ...
            if s0 != 1.0 and self.cond is None:
                io.x.mul_(s0)  # ... through Solver.scale_model_input for THIS step; later steps get it from the kernel
            self.primed, self.primed_key = True, gkey
        if not self.use_graph:
            run()
            tail()
            self._update(io)
            return self.x
        if self.graph is None or self.graph_key != gkey:
            run()  # warm-up outside capture; reads io.x only
            tail()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                run()
                tail()
                self._update(io)
            self.graph, self.graph_key = g, gkey
        self.graph.replay()
        return self.x

    def _draw(self, generator: Optional[torch.Generator]) -> Tensor:
        """One Gaussian draw of the latents' shape and dtype into `sde_noise`, outside any captured graph: a CPU generator cannot be captured at
        all, and a device generator would have to be registered with the graph before capture, while it changes with every set_inputs.  Drawn
        as the reference draws it (dpm.py:317-322: torch.randn of x's shape and dtype) on the generator's device -- a CPU generator draws on the
        CPU and the numbers are copied over, so a trajectory recorded on the CPU can be followed draw for draw -- or on the latents' device from
        the global stream without one."""
        x, buf = self.x, self.sde_noise
        assert x is not None and buf is not None
        dev = generator.device if generator is not None else x.device
        buf.copy_(torch.randn(tuple(x.shape), generator=generator, device=dev, dtype=x.dtype))
        return buf

    @torch.no_grad()
    def restart(self, restart: Any, generator: Optional[torch.Generator] = None) -> Tensor:
        """Restart sampling (latent_diffusion/restart.py:47-77) on the resident latents with the staged inputs: `restart` is anything with
        `timesteps` (descending train timesteps of the interval) and `num_iterations`, e.g. refiners_amd.latent_diffusion.restart.Restart.
        Per iteration: one draw, x <- factor x + sqrt(1 - factor^2) noise with factor = scale[t_first] / scale[t_last] (add_noise_interval), the
        model input primed again, then the DDIM segment under a temporary DDIM that carries those timesteps.  The caller's solver, coefficient
        tables and captured graph are put back afterwards."""
        from ..latent_diffusion.sampling import DDIM

        assert self.x is not None and self.sde_noise is not None, "call set_inputs first"
        assert isinstance(self.solver, DDIM), "Restart sampling only works with DDIM solver"
        ts = restart.timesteps.cpu()
        assert ts.numel() >= 2, "a restart interval needs two timesteps at least"
        tables = ("coef_table", "coef", "scales_input", "in_scale", "ts_table", "sag_table", "sag_coef")
        saved = (self._solver, {k: getattr(self, k, None) for k in tables}, self.graph, self.graph_key)
        programs = [(e, None if e is None else e.io) for e in (self.engine, self.engine_c)]
        inner = DDIM(self.solver.num_inference_steps)
        inner.timesteps = ts
        csf = inner.cumulative_scale_factors  # (float32, as the reference's solver computes the factor)
        factor = csf[int(ts[0])] / csf[int(ts[-1])]
        alpha, beta = float(factor), float(torch.sqrt(1 - factor ** 2))
        self.solver = inner  # (drops the table and the graph: rebuilt for the segment)
        try:
            for _ in range(int(restart.num_iterations)):
                native.axpby(self.x, alpha, self._draw(generator), beta, self.x)
                self.primed = False
                for s in range(ts.numel() - 1):
                    self.step(s)
        finally:
            self._solver, self.linear, self.sde = saved[0], hasattr(saved[0], "linear_step"), False
            for k, v in saved[1].items():
                setattr(self, k, v)
            # the caller's graph holds the programs' buffers by address: it comes back only if the segment ran on the same ones
            same = all(e is None or e.io is io for e, io in programs)
            self.graph, self.graph_key = (saved[2], saved[3]) if same else (None, None)
            self.primed = False
        return self.x

    @torch.no_grad()
    def sample(self, first_step: Optional[int] = None) -> Tensor:
        """Run the trajectory from the solver's `first_inference_step` (img2img starts later than 0).  A multistep solver
        decides between its first- and second-order update by comparing the step with ITS first_inference_step
        (solvers/dpm.py:136-152), so starting anywhere else would run a second-order update on an all-zero history."""
        first = int(getattr(self.solver, "first_inference_step", 0))
        if first_step is None:
            first_step = first
        assert first_step == first or not self.linear, (
            f"sample(first_step={first_step}) but solver.first_inference_step={first}: build the solver with first_inference_step={first_step}")
        for s in range(first_step, self.solver.num_inference_steps):
            self.step(s)
        for eng in (self.engine, self.engine_c, self.engine2):  # the trajectory's last replays (the in-loop look runs every CHECK_EVERY-th step)
            if eng is not None:
                eng.check_handovers()
        return self.x  # type: ignore[return-value]
