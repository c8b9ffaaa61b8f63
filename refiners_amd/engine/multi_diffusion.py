"""MultiDiffusion on the MI355X engine: one denoising step of a canvas larger than one UNet call.

    md = CompiledMultiDiffusion(unet)                          # the UNet of an SDXLMultiDiffusion / SD1MultiDiffusion's `sd`
    x = md(x, noise=noise, step=step, targets=targets)         # == SDXLMultiDiffusion(sd)(x, noise=noise, step=step, targets=targets)

`targets` are `SDXLTarget` / `SD1DiffusionTarget` objects of refiners_amd.latent_diffusion.multi_diffusion or of refiners itself (duck-typed).
The reference (latent_diffusion/multi_diffusion.py:98-123) runs one UNet call and a handful of torch crop / paste ops per target.  Tiles of one
step are independent until the blend, so here they are a BATCH:

    active targets of the step  --group by (tile size, timestep, update form)-->  chunks of at most `tile_batch` targets
    per chunk:   mi355x_md_gather  ->  the lowered UNet program at batch 2T  ->  mi355x_md_target_step (one coefficient row per target)
    then ONE     mi355x_md_blend over the canvas, targets in list order (the reference's summation order)

The canvas stays resident in HBM (the returned tensor IS the resident canvas: pass it back and nothing is staged), every solver's history
lives here per target (a target's solver object is asked for its tables only), and a step whose active set and chunking equal the previous
step's replays ONE captured HIP graph: per-step host work is then the descriptor / coefficient copies and one launch.

Refused with `Unsupported` -- the call then runs the mirror's host loop over the stock forward, behind a RuntimeWarning, like CompiledUNet does for
a tree it does not know: a UNet tree the lowering refuses, a solver that draws noise per step (LCM, DPM with an SDE variance), Self-Attention
Guidance on the tree, a canvas batch other than 1, more active targets than mi355x_md_blend takes.  Out of scope: per-target ControlLora /
ControlNet conditions and per-target IP-Adapter embeddings, the MultiUpscaler pipeline (the tiled VAE: engine/tiled_vae.py), and targets
without classifier-free guidance (`CompiledSDXL(classifier_free_guidance=False)` and its mi355x_ddim_step / mi355x_linear_step have no
per-target form here: every target runs the guided pair).  LoRAs are part of the tree and simply
work; so does an IP-Adapter with one embedding for every target (`md.clip_image_embedding = [negative ; conditional]`)."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Any, Optional, Sequence

import torch
from torch import Tensor

from .. import native
from .compiled import CompiledUNet, _ident
from .packing import Unsupported, isa

#: targets per UNet launch when the caller does not say.  README's batch points (23.2 ms for one image per step, 65.0 ms for 4, 125.2 ms for 8: about 16 ms
#: per image in a batch) were measured at 128 x 128 latents of whole images; NOT measured at tile shapes yet (tools/probe_multi_diffusion.py is the probe).
TILE_BATCH = 4


@dataclass(frozen=True)
class Chunk:
    indices: tuple[int, ...]  # positions in the caller's target list, ascending
    size: tuple[int, int]  # (h, w) of every tile of the chunk
    timestep: float  # the UNet timestep every target of the chunk has at this step
    linear: bool  # update form: mi355x_cfg_linear_step's arithmetic (Euler, DPM-Solver++) or mi355x_cfg_ddim_step's


# -- solvers: tables only -------------------------------------------------------------------------------------------------------------
def solver_tables(solver: Any, cache: Optional[dict] = None) -> Any:
    """What the engine asks a target's solver: `timesteps`, `coefficients` (DDIM) or `linear_step` / `input_scale` (Euler, DPM-Solver++), and the
    add_noise factors (`sag_coefficients`).  The mirror's solvers have them; one of refiners' own is restated as the mirror's class of the same name
    and schedule.  A solver that draws noise per step is refused: its update is not a function of (x, eps, history)."""
    if getattr(solver, "needs_noise", None) is not None or type(solver).__name__ == "LCMSolver":
        raise Unsupported(f"{type(solver).__name__} draws noise per step")
    if hasattr(solver, "linear_step") and float(getattr(solver, "sde_variance", 0.0) or 0.0) != 0.0:  # the mirror's SDE DPM-Solver++ (it has no needs_noise)
        raise Unsupported(f"{type(solver).__name__} with an SDE variance draws noise per step")
    if hasattr(solver, "coefficients") or hasattr(solver, "linear_step"):
        return solver
    cache = cache if cache is not None else {}
    hit = cache.get(id(solver))
    if hit is not None and hit[0] is solver:
        return hit[1]
    from ..latent_diffusion import sampling, solvers

    name, n, first = type(solver).__name__, int(solver.num_inference_steps), int(getattr(solver, "first_inference_step", 0))
    params = getattr(solver, "params", None)
    if name == "DDIM":
        mine: Any = sampling.DDIM(n, first_inference_step=first)
    elif name == "Euler":
        mine = solvers.Euler(n, first_inference_step=first)
    elif name == "DPMSolver":
        if float(getattr(params, "sde_variance", 0.0) or 0.0) != 0.0:
            raise Unsupported("DPMSolver with an SDE variance draws noise per step")
        spacing = str(getattr(getattr(params, "timesteps_spacing", None), "value", "custom")).lower()
        mine = solvers.DPMSolver(n, first_inference_step=first, last_step_first_order=bool(getattr(solver, "last_step_first_order", False)),
                                 timesteps_spacing=spacing if spacing in ("custom", "trailing") else "custom",
                                 sigma_schedule=getattr(getattr(params, "sigma_schedule", None), "value", getattr(params, "sigma_schedule", None)))
    else:
        raise Unsupported(f"solver {name} has no table form here")
    if not torch.equal(mine.timesteps.cpu().double(), solver.timesteps.cpu().double()):
        raise Unsupported(f"{name}: a schedule other than the mirrored default")
    cache[id(solver)] = (solver, mine)
    return mine


def is_active(target: Any, step: int) -> bool:
    """multi_diffusion.py:103-114: the start step of a target with init latents, or a step inside the window."""
    return (step == target.start_step and target.init_latents is not None) or target.start_step <= step <= target.end_step


def chunk_plan(step: int, targets: Sequence[Any], tile_batch: int = TILE_BATCH, cache: Optional[dict] = None) -> tuple[list[Chunk], list[int]]:
    """(chunks, skipped target positions) of one step.  Groups keep the order in which their first target appears; inside a group targets keep list order."""
    assert 1 <= tile_batch <= native.MD_MAX_TARGETS
    groups: dict[tuple, list[int]] = {}
    skipped: list[int] = []
    for i, t in enumerate(targets):
        if not is_active(t, step):
            skipped.append(i)
            continue
        tb = solver_tables(t.solver, cache)
        h, w = t.size
        groups.setdefault(((int(h), int(w)), float(tb.timesteps[step]), hasattr(tb, "linear_step")), []).append(i)
    chunks = [Chunk(tuple(idx[k : k + tile_batch]), size, ts, linear) for (size, ts, linear), idx in groups.items() for k in range(0, len(idx), tile_batch)]
    return chunks, skipped


def graph_key(chunks: Sequence[Chunk], targets: Sequence[Any]) -> tuple:
    """What a captured step holds by address or by shape: which target objects are active and how they are chunked.  The timestep and every
    coefficient are device data, so two steps with the same active set share the key."""
    return tuple((c.indices, tuple((id(targets[i]), targets[i].init_latents is not None) for i in c.indices), c.size, c.linear) for c in chunks)


class _ChunkState:
    """Static buffers of one chunk of the current plan."""

    def __init__(self, chunk: Chunk, C: int, dev: torch.device, dtype: torch.dtype, init_slots: list[int]) -> None:
        T, (h, w) = len(chunk.indices), chunk.size
        self.chunk = chunk
        self.view = torch.empty(T, C, h, w, device=dev, dtype=dtype)
        self.hist = torch.zeros(T, C, h, w, device=dev, dtype=dtype) if chunk.linear else None
        self.init_slots = init_slots  # chunk rows that own a row of `init` (targets with init latents, whatever the step)
        self.init = torch.zeros(len(init_slots), C, h, w, device=dev, dtype=dtype) if init_slots else None
        self.desc = torch.zeros(T, native.MD_GATHER_DESC_BYTES, dtype=torch.uint8, device=dev)
        self.desc_host = torch.zeros(T, native.MD_GATHER_DESC_BYTES, dtype=torch.uint8)
        self.coef = torch.zeros(T, 8, dtype=torch.float32, device=dev)
        self.emb_key: Any = None
        self.got: dict[str, Any] = {}
        self.stepped: Optional[Tensor] = None  # a view into the plan's one stepped buffer


class CompiledMultiDiffusion:
    def __init__(self, unet: Any, tile_batch: int = TILE_BATCH, use_graph: bool = True, lora_mode: str = "fused") -> None:
        assert 1 <= tile_batch <= native.MD_MAX_TARGETS
        self.unet = unet
        self.tile_batch = tile_batch  # default: see TILE_BATCH (not measured at tile shapes yet)
        self.use_graph = use_graph
        self.engine = CompiledUNet(unet, use_graph=False, lora_mode=lora_mode)  # chunk 0's program; further chunks get siblings that share its packed weights
        self.engines: list[CompiledUNet] = [self.engine]
        self.clip_image_embedding: Optional[Tensor] = None  # an IP-Adapter's ONE embedding for every target, [negative ; conditional]
        self.canvas: Optional[Tensor] = None
        self.noise: Optional[Tensor] = None
        self.noise_key: Any = None
        self.plan_key: Any = None
        self.states: list[_ChunkState] = []
        self.stepped: Optional[Tensor] = None
        self.blend_desc: Optional[Tensor] = None
        self.blend_host: Optional[Tensor] = None
        self.blend_order: list[tuple[int, int, int]] = []  # (target position, chunk, row) in list order
        self.hist_of: dict[int, tuple[Any, Tensor]] = {}  # id(target) -> (target, its row of a chunk's history buffer)
        self.masks: dict[int, tuple[Any, Any, Tensor]] = {}  # id(target) -> (its opacity mask, the mask's identity, float32 device copy)
        self.key_targets: tuple = ()  # the targets whose id() the current plan key holds
        self.ts_tables: dict[tuple, Tensor] = {}
        self.solver_cache: dict = {}
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.graph_key: Any = None
        self.warned: set[str] = set()
        self.stats: dict[str, Any] = {}

    # -- refusals ----------------------------------------------------------------------------------------------------------------------
    def check(self, x: Tensor, targets: Sequence[Any], step: Optional[int] = None) -> None:
        """Raises Unsupported for what the native path does not take (the tree itself is judged by the lowering, at the first chunk)."""
        if x.dim() != 4 or x.shape[0] != 1:
            raise Unsupported(f"a canvas batch of {x.shape[0] if x.dim() == 4 else tuple(x.shape)}: the canvas kernels take one image")
        p = getattr(self.unet, "parent", None)
        while p is not None:
            if isa(p, "SAGAdapter"):
                raise Unsupported("Self-Attention Guidance on the tree: its second UNet pass per target is not batched")
            p = getattr(p, "parent", None)
        for t in targets:
            solver_tables(t.solver, self.solver_cache)
        if step is not None and sum(is_active(t, step) for t in targets) > native.MD_MAX_TARGETS:
            raise Unsupported(f"more than {native.MD_MAX_TARGETS} active targets in one step")

    def plan(self, step: int, targets: Sequence[Any]) -> tuple[list[Chunk], list[int]]:
        return chunk_plan(step, targets, self.tile_batch, self.solver_cache)

    # -- the host loop -------------------------------------------------------------------------------------------------------------------
    def _host(self, x: Tensor, noise: Tensor, step: int, targets: Sequence[Any]) -> Tensor:
        """The mirror's MultiDiffusion over the stock forward; every target's own solver object does the update (and keeps its own history)."""
        from ..latent_diffusion import multi_diffusion as M

        sdxl = any(hasattr(t, "pooled_text_embedding") for t in targets)
        den = (M.SDXLDenoiser if sdxl else M.SD1Denoiser)(self.unet, solver=targets[0].solver if targets else None)
        dt = self.unet.dtype
        with torch.no_grad():
            return (M.SDXLMultiDiffusion if sdxl else M.SD1MultiDiffusion)(den)(x.to(dt), noise=noise.to(dt), step=step, targets=targets)

    def _refuse(self, why: str) -> None:
        self.stats = {"whole_fallback": why}
        if why not in self.warned:
            self.warned.add(why)
            warnings.warn(f"refiners_amd: MultiDiffusion is not run on the MI355X kernels ({why}); running the host loop over the stock Chain forward instead",
                          RuntimeWarning, stacklevel=3)

    # -- plan state ---------------------------------------------------------------------------------------------------------------------
    def _build_states(self, chunks: list[Chunk], targets: Sequence[Any], key: Any) -> None:
        canvas = self.canvas
        assert canvas is not None
        C, dev, dtype = canvas.shape[1], canvas.device, canvas.dtype
        old = self.hist_of
        self.hist_of, self.states, self.blend_order = {}, [], []
        total = sum(len(c.indices) * C * c.size[0] * c.size[1] for c in chunks)
        self.stepped = torch.empty(total, device=dev, dtype=dtype)
        off = 0
        for k, c in enumerate(chunks):
            st = _ChunkState(c, C, dev, dtype, [r for r, i in enumerate(c.indices) if targets[i].init_latents is not None])
            n = st.view.numel()
            st.stepped = self.stepped[off : off + n].view_as(st.view)
            st.stepped_off = off
            off += n
            for r, i in enumerate(c.indices):
                t = targets[i]
                if st.hist is not None:
                    kept = old.get(id(t))
                    if kept is not None and kept[0] is t and kept[1].shape == st.hist[r].shape:
                        st.hist[r].copy_(kept[1])  # the target moved to another chunk: its data estimate moves with it
                    self.hist_of[id(t)] = (t, st.hist[r])
                self.blend_order.append((i, k, r))
            self.states.append(st)
            while len(self.engines) <= k:
                e = CompiledUNet(self.unet, use_graph=False, lora_mode=self.engine.lora_mode)
                e.cache = self.engine.cache  # one set of packed weights for every chunk's program
                self.engines.append(e)
        self.blend_order.sort()
        n = len(self.blend_order)
        self.blend_desc = torch.zeros(n, native.MD_BLEND_DESC_BYTES, dtype=torch.uint8, device=dev)
        self.blend_host = torch.zeros(n, native.MD_BLEND_DESC_BYTES, dtype=torch.uint8)
        self.plan_key, self.graph = key, None

    def _mask(self, t: Any, C: int, dev: torch.device) -> Optional[Tensor]:
        """The target's opacity mask as float32 on the device, broadcast (by strides) over the channels; converted once per mask tensor."""
        m = t.opacity_mask
        if m is None:
            return None
        hit = self.masks.get(id(t))
        if hit is None or hit[0] is not m or hit[1] != _ident(m):
            h, w = t.size
            f = m.detach().to(device=dev, dtype=torch.float32)
            hit = self.masks[id(t)] = (m, _ident(m), f.expand(1, C, h, w) if f.dim() == 4 else f.expand(C, h, w))
        return hit[2]

    def _embeddings(self, st: _ChunkState, targets: Sequence[Any]) -> None:
        """[negatives ; conditionals] stacks of the chunk's rows, rebuilt only when a target's embedding is another tensor (a fresh stack per step would look
        like a new prompt to the engine and re-run its prologue)."""
        ts = [targets[i] for i in st.chunk.indices]
        names = ("clip_text_embedding", "pooled_text_embedding", "time_ids")
        key = (tuple(_ident(getattr(t, n, None)) for t in ts for n in names), _ident(self.clip_image_embedding))
        if key == st.emb_key:
            return
        dev, dt = st.view.device, st.view.dtype

        def stack(name: str, dtype: Any) -> Optional[Tensor]:
            vals = [getattr(t, name, None) for t in ts]
            if vals[0] is None:
                return None
            for v in vals:
                assert v is not None and v.shape[0] == 2, f"target.{name}: [negative ; conditional], two rows"
            return torch.cat([v[:1] for v in vals] + [v[1:] for v in vals]).to(device=dev, dtype=dtype).contiguous()

        tokens = {("cross_attention_block", "clip_text_embedding"): stack("clip_text_embedding", dt)}
        if self.clip_image_embedding is not None:
            e, T = self.clip_image_embedding, len(ts)
            tokens[("ip_adapter", "clip_image_embedding")] = torch.cat((e[:1].expand(T, -1, -1), e[1:].expand(T, -1, -1))).to(device=dev, dtype=dt).contiguous()
        st.got = {"pooled": stack("pooled_text_embedding", dt), "time_ids": stack("time_ids", torch.float32), "tokens": tokens, "conditions": {}, "t2i": {}}
        st.emb_key = key
        st.emb_refs = [getattr(t, n, None) for t in ts for n in names]  # (see compiled._ident: a live tensor's address cannot be recycled)

    def _timesteps(self, tb: Any, dev: torch.device) -> Tensor:
        vals = tuple(float(v) for v in tb.timesteps.tolist())
        tab = self.ts_tables.get(vals)
        if tab is None or tab.device != dev:
            tab = self.ts_tables[vals] = torch.tensor(vals, dtype=torch.float32, device=dev)
        return tab

    def _fill_tables(self, step: int, targets: Sequence[Any], noise: Tensor) -> None:
        """The per-step host work: descriptor and coefficient rows of every chunk and of the blend, init latents of the targets that start now."""
        canvas = self.canvas
        assert canvas is not None and self.blend_host is not None and self.blend_desc is not None
        C, dev = canvas.shape[1], canvas.device
        need_noise = False
        for st in self.states:
            rows, coefs = [], []
            for r, i in enumerate(st.chunk.indices):
                t = targets[i]
                tb = solver_tables(t.solver, self.solver_cache)
                s = float(tb.input_scale(step)) if hasattr(tb, "input_scale") else 1.0
                top, left = t.offset
                if step == t.start_step and t.init_latents is not None:
                    a, b = tb.sag_coefficients(step)  # (scale, std) of Solver.add_noise at this step
                    slot = st.init_slots.index(r)
                    st.init[slot].copy_(t.init_latents.reshape(st.init[slot].shape))  # type: ignore[index]
                    rows.append((native.MD_SRC_INIT, top, left, slot, a, b, s))
                    need_noise = True
                else:
                    rows.append((native.MD_SRC_CANVAS, top, left, 0, 1.0, 0.0, s))
                if st.chunk.linear:
                    coefs.append([float(t.condition_scale), *tb.linear_step(step)])
                else:
                    cur, sig, prev, nf = tb.coefficients(step)
                    coefs.append([float(t.condition_scale), cur, sig, prev, nf, 0.0, 0.0, 0.0])
            st.desc_host.copy_(native.md_gather_rows(rows))
            st.desc.copy_(st.desc_host, non_blocking=True)
            st.coef.copy_(torch.tensor(coefs, dtype=torch.float32), non_blocking=True)
        nk = _ident(noise)
        if self.noise is None or self.noise.shape != canvas.shape:
            self.noise, self.noise_key, self.graph = torch.empty_like(canvas), None, None
        if need_noise and nk != self.noise_key:  # read by the targets that start now only
            self.noise.copy_(noise.reshape(canvas.shape))
            self.noise_key, self.noise_ref = nk, noise
        brows = []
        for i, k, r in self.blend_order:
            t, st = targets[i], self.states[k]
            (top, left), (h, w) = t.offset, t.size
            brows.append((top, left, h, w, float(t.weight), st.stepped_off + r * C * h * w, self._mask(t, C, dev)))
        self.blend_host.copy_(native.md_blend_rows(brows))
        self.blend_desc.copy_(self.blend_host, non_blocking=True)

    # -- one step -----------------------------------------------------------------------------------------------------------------------
    def _launch_chunk(self, k: int, unet_only: bool = False) -> None:
        st, eng = self.states[k], self.engines[k]
        assert eng.io is not None and eng.low is not None
        native.md_gather(self.canvas, self.noise, st.init, st.desc, st.desc_host, st.view, eng.io.x)  # type: ignore[arg-type]
        native.replay(eng.low.step)
        if not unet_only:
            native.md_target_step(st.view, eng.io.out, st.stepped, st.hist, st.coef, st.chunk.linear)  # type: ignore[arg-type]

    def _launch_all(self) -> None:
        for k in range(len(self.states)):
            self._launch_chunk(k)
        native.md_blend(self.canvas, self.stepped, self.blend_desc, self.blend_host, len(self.blend_order))  # type: ignore[arg-type]

    def _native(self, x: Tensor, noise: Tensor, step: int, targets: Sequence[Any]) -> Tensor:
        dt = self.unet.dtype
        chunks, skipped = self.plan(step, targets)
        if self.canvas is None or x is not self.canvas:
            if self.canvas is None or self.canvas.shape != x.shape or self.canvas.device != x.device or self.canvas.dtype != dt:
                self.canvas, self.noise, self.plan_key, self.graph = torch.empty(tuple(x.shape), device=x.device, dtype=dt), None, None, None
            self.canvas.copy_(x)
        canvas = self.canvas
        self.stats = {"chunks": [(c.indices, c.size, c.linear) for c in chunks], "skipped": skipped, "graph_replayed": False}
        if not chunks:
            return canvas
        key = graph_key(chunks, targets)
        if key != self.plan_key:
            self._build_states(chunks, targets, key)
            self.key_targets = tuple(targets)  # the key holds their id(): while it is kept they stay alive, so that no new target can be mistaken for one of them
        engine_keys = []
        for k, st in enumerate(self.states):
            self._embeddings(st, targets)
            tb = solver_tables(targets[st.chunk.indices[0]].solver, self.solver_cache)
            table = self._timesteps(tb, canvas.device)
            eng = self.engines[k]
            eng.io_override = None
            got = dict(st.got, timestep=table[step : step + 1], timesteps_all=table, step_index=step)
            if eng.prepare_explicit((2 * len(st.chunk.indices), canvas.shape[1]) + st.chunk.size, canvas.device, got):  # raises Unsupported for a tree it refuses
                eng.run_prologue()
            eng.check_handovers(eng.CHECK_EVERY)
            engine_keys.append(eng.key)
        self._fill_tables(step, targets, noise)
        if not self.use_graph:
            self._launch_all()
            return canvas
        gkey = (key, tuple(engine_keys))
        if self.graph is None or self.graph_key != gkey:
            for k in range(len(self.states)):
                self._launch_chunk(k, unet_only=True)  # warm-up outside capture (first-launch attribute calls, workspaces); writes the views and the UNet buffers only
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._launch_all()
            self.graph, self.graph_key = g, gkey
        else:
            self.stats["graph_replayed"] = True
        self.graph.replay()
        return canvas

    @torch.no_grad()
    def __call__(self, x: Tensor, /, noise: Tensor, step: int, targets: Sequence[Any]) -> Tensor:
        try:
            self.check(x, targets, step)
            return self._native(x, noise, step, targets)
        except Unsupported as exc:
            self._refuse(str(exc))
            return self._host(x, noise, step, targets)
