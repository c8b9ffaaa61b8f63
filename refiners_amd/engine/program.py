"""What a single-pass engine (text, image prompt, SAM ViT, Swin, MVANet, DINOv2, lineart, T2I, ELLA) keeps between calls: the lowered
`Program` of every input shape it has seen, behind one `ProgramCache`.  The rules of that cache -- when the programs are dropped, how many
are kept, which refusals are remembered and when the packed weights nothing uses any more may be swept -- live here and nowhere else."""
from __future__ import annotations

import os
import warnings
from types import SimpleNamespace
from typing import Any, Callable, Optional

import torch

from .. import native
from .packing import PackCache, Unsupported, launches

MAX_PROGRAMS = 8  # lowered shapes kept by an engine that serves several


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


class Entry(SimpleNamespace):
    """One lowered shape.  The engine's `build` sets `low` (the finished lowering), `use_graph` and the static buffers it copies into and
    out of (`x`, `out`, ...); `ProgramCache.get` adds `program` and `stats`, the part of the engine's `stats` that is fixed with the lowering
    (the engine adds its own keys: `dict(e.stats, lowerings=...)`)."""


class ProgramCache:
    """The programs of one engine, for one state of its tree: `entries` (key -> Entry, oldest first, at most `capacity`), the keys whose
    lowering was `refused`, the `PackCache` every lowering packs its weights through, and `lowerings`, counted over the engine's life.
    `last` is what the latest `get` returned."""

    def __init__(self, owner: str, capacity: int = 1, fallback: bool = False) -> None:
        assert capacity >= 1
        self.owner, self.capacity, self.fallback = owner, capacity, fallback
        self.cache = PackCache()
        self.version: Any = None
        self.entries: dict[Any, Entry] = {}
        self.refused: set = set()
        self.lowerings = 0
        self.last: Optional[Entry] = None

    def get(self, version: Any, key: Any, build: Callable[[PackCache], Entry]) -> Optional[Entry]:
        """The entry of `key`, lowered by `build(pack_cache)` when it is not held.  `version` is the engine's token for the state of its tree
        and weights: when it moves, every program and every refusal goes.  None: the lowering of `key` raised Unsupported, now or earlier under
        this version, and the engine runs its stock forward (`fallback` engines only: the others let Unsupported through and remember nothing)."""
        if version != self.version:
            self.entries.clear()
            self.refused.clear()
            self.cache.used.clear()
            self.version = version
        self.last = self.entries.get(key)
        if self.last is None and key not in self.refused:
            try:
                e = build(self.cache)
            except Unsupported as err:
                if not self.fallback:
                    raise
                # (stacklevel: this frame, the engine's __call__, then whoever called that)
                warnings.warn(f"{self.owner}: {err}; running the stock forward", RuntimeWarning, stacklevel=3)
                self.refused.add(key)
                return None
            e.program = Program(e.low.step, e.use_graph, low=e.low)
            e.stats = dict(e.low.stats, step_ops=launches(e.low.step), pool_bytes=e.low.step_pool.bytes())
            self.lowerings += 1
            while len(self.entries) >= self.capacity:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = self.last = e
            # the packs nothing used since the programs were last dropped go -- but only while no other program is held: a lowering marks
            # the packs IT uses, so a sweep beside a live entry would take that entry's packs out of the store
            if len(self.entries) == 1:
                self.cache.sweep()
        return self.last


class HasPrograms:
    """What an engine shows of its `self.programs`: nothing is copied."""

    programs: ProgramCache
    cache = property(lambda self: self.programs.cache)
    entries = property(lambda self: self.programs.entries)
    lowerings = property(lambda self: self.programs.lowerings)
    low = property(lambda self: self.programs.last.low if self.programs.last is not None else None, doc="the lowering of the last call")
    program = property(lambda self: self.programs.last.program if self.programs.last is not None else None, doc="the program of the last call, None after a stock fallback")
