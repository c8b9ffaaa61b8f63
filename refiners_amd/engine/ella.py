"""MI355X lowering of ELLA's timestep-aware text connector (refiners_amd.latent_diffusion.ella, or refiners' own
foundationals.latent_diffusion.ella_adapter classes): the first token stream the engine produces INSIDE the step.

Every other text or image token stream is prompt-side: its K / V^T projections run once per prompt, in the prologue.  ELLA's 64 latents
come out of a Perceiver resampler whose AdaLayerNorms, and the latents themselves, are modulated by the step's timestep embedding, so the
resampler and the UNet's K / V^T projections that read its output are step work (captured in the step's HIP graph), while the prologue keeps
what depends on the prompt alone.

  prologue   input Linear over the LLM's token embeddings [B * Tp, input_dim] -> x [B * Tp, width]   (Tp = T rounded up to 64)
             table mode (the engine knows the solver's S timesteps): RangeEncoder -> SiLU -> the time-table GEMM for all B * S rows
  step       time table: RangeEncoder -> SiLU -> ONE GEMM against the row-stacked weights of every Linear that reads ella.timestep_embedding
             (3 AdaLayerNorm Linears of 2 * width columns per layer + the latents' Linear); consumers take column slices.  Table mode: one
             mi355x_gather_rows of the step's B rows instead.
             latents = Parameter rows + their time row: one GEMM of one-hot rows against the transposed Parameter, time row as `rowbias`
             per TransformerLayer (7 launches):
               mi355x_ella_adaln      [AdaLN(latents) ; AdaLN(x) ; zero rows] -> packed [B * Lp, width], Lp = Nl + T rounded up to 64
               Q|K|V^T GEMM           stacked weights over the packed rows, V stored transposed (Q of the text rows is computed and unused)
               mi355x_attention_general   Lq = Nl, Lk = Nl + T, non-causal, batch strides over Lp
               out-projection         + latents as residual, in place
               mi355x_ella_adaln      T = 0: the feed-forward's AdaLayerNorm
               FF1                    squared-ReLU epilogue (mi355x_gemm code 5)
               FF2                    + residual, in place
             OutputProjection (Linear + mi355x_layernorm) when the encoder has an output width
  result     [B * Nlp, out_width], Nlp = Nl rounded up to 64, padding rows zero: the layout of the engine's token buffers

`EllaLowering` is the mixin `UNetLowering` takes these emitters from; `CompiledELLA` runs the resampler alone.
Refused (Unsupported): any child the patterns above do not name, run-time LoRAs on the encoder's own Linears (lora_mode="merged" folds them),
widths that are no multiple of 64, head dims the attention kernel does not serve.
"""
from __future__ import annotations

import os
import warnings
from types import SimpleNamespace
from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from ..fluxion.tree import tree_epoch
from .packing import LinSpec, PackCache, Unsupported, _expect, cname, isa, kids, launches

LLM_TOKENS = ("adapted_cross_attention_block", "llm_text_embedding")
ELLA_TOKENS = ("ella", "latents")
MAX_PROGRAMS = 8  # lowered (B, T) shapes kept per CompiledELLA


def pad64(n: int) -> int:
    return (n + 63) // 64 * 64


class _TimeLinear:
    """One Linear(SiLU(ella.timestep_embedding)) of the tree: its spec, the AdaLayerNorm's epsilon and, once the time table is laid out, its columns."""

    def __init__(self, lin: LinSpec, eps: float = 0.0) -> None:
        self.lin, self.eps = lin, eps
        self.cols: Optional[Tensor] = None  # [B, lin.N] view of the step's time-table rows

    def halves(self) -> tuple[Tensor, Tensor]:
        """(shift, scale): the reference's chunk(2), shift first."""
        C = self.lin.N // 2
        return self.cols[:, :C], self.cols[:, C:]  # type: ignore[index]


class EllaLowering:
    """Emitters of the ELLA sub-program, for a Lowering that also has UNetLowering._range_encoder and an `io` with timestep / timesteps /
    step_rows."""

    # -- patterns -----------------------------------------------------------------------------------------------------------------
    def _ella_plain(self, node: Any) -> LinSpec:
        sp = self.linear_spec(node)
        _expect(sp.lora is None, "a run-time LoRA on one of ELLA's own Linears is not lowered (lora_mode='merged' folds it)")
        return sp

    def _ella_time_linear(self, chain: Any) -> LinSpec:
        """Chain | Residual (UseContext ella.timestep_embedding, SiLU, Linear) -> the Linear's spec."""
        ch = kids(chain)
        _expect(len(ch) == 3 and isa(ch[0], "UseContext") and (ch[0].context, ch[0].key) == ("ella", "timestep_embedding") and isa(ch[1], "SiLU"),
                f"unexpected time branch {cname(chain)} in ELLA")
        return self._ella_plain(ch[2])

    def _ella_adaln(self, node: Any, C: int) -> _TimeLinear:
        ch = kids(node)
        _expect(isa(node, "AdaLayerNorm") and len(ch) == 2 and isa(ch[0], "Parallel") and isa(ch[1], "Lambda"), f"unexpected {cname(node)} where ELLA has an AdaLayerNorm")
        pc = kids(ch[0])
        _expect(len(pc) == 2 and isa(pc[0], "LayerNormNoAffine") and isa(pc[1], "Chain") and tuple(pc[0].normalized_shape) == (C,) and not pc[0].elementwise_affine,
                "unexpected AdaLayerNorm layout")
        sp = self._ella_time_linear(pc[1])
        _expect(sp.N == 2 * C and sp.b is not None, "AdaLayerNorm's Linear does not produce (shift | scale)")
        return _TimeLinear(sp, float(pc[0].eps))

    def _ella_layer(self, layer: Any, C: int) -> SimpleNamespace:
        ch = kids(layer)
        _expect(isa(layer, "TransformerLayer") and len(ch) == 2 and all(isa(c, "Residual") for c in ch), "unexpected ELLA TransformerLayer layout")
        r1, r2 = kids(ch[0]), kids(ch[1])
        _expect(len(r1) == 2 and isa(r1[0], "Parallel") and isa(r1[1], "PerceiverAttention"), "unexpected attention residual in ELLA")
        pc = kids(r1[0])
        _expect(len(pc) == 2 and isa(pc[0], "UseContext") and (pc[0].context, pc[0].key) == ("perceiver_resampler", "x") and isa(pc[1], "Identity"),
                "ELLA's attention does not read (perceiver_resampler.x, latents)")
        pa = kids(r1[1])
        _expect(len(pa) == 3 and isa(pa[0], "Distribute") and isa(pa[1], "Parallel") and isa(pa[2], "Attention") and not isa(pa[2], "SelfAttention"), "unexpected PerceiverAttention layout")
        dc, sel = kids(pa[0]), kids(pa[1])
        _expect(len(dc) == 2 and len(sel) == 3 and isa(sel[0], "GetArg") and sel[0].index == 1 and isa(sel[1], "Lambda") and isa(sel[2], "Lambda"),
                "unexpected query / key / value selection in PerceiverAttention")
        (qn, kn, vn), sd, on, ip = self._split_attention(pa[2])
        _expect(ip is None, "image cross-attention inside ELLA")
        q, k, v, o = (self._ella_plain(n) for n in (qn, kn, vn, on))
        _expect(all((s.N, s.K) == (C, C) for s in (q, k, v, o)), "unexpected PerceiverAttention projections")
        _expect(len(r2) == 2 and isa(r2[1], "FeedForward"), "unexpected feed-forward residual in ELLA")
        ff = kids(r2[1])
        _expect(len(ff) == 3 and isa(ff[1], "SquaredReLU"), "unexpected ELLA FeedForward layout")
        f1, f2 = self._ella_plain(ff[0]), self._ella_plain(ff[2])
        _expect(f1.K == C and f2.N == C and f2.K == f1.N, "unexpected ELLA feed-forward widths")
        return SimpleNamespace(ada_x=self._ella_adaln(dc[0], C), ada_l=self._ella_adaln(dc[1], C), ada_ff=self._ella_adaln(r2[0], C), q=q, k=k, v=v, o=o, f1=f1, f2=f2,
                               heads=sd.num_heads)

    def _ella_qkv(self, L: SimpleNamespace, C: int) -> LinSpec:
        def make() -> tuple[Tensor, Optional[Tensor]]:
            w = torch.cat([L.q.w, L.k.w, L.v.w], 0).contiguous()
            if all(s.b is None for s in (L.q, L.k, L.v)):
                return w, None
            z = lambda s: s.b if s.b is not None else torch.zeros(C, device=self.device, dtype=self.dtype)  # noqa: E731
            return w, torch.cat([z(s) for s in (L.q, L.k, L.v)]).contiguous()

        return LinSpec(*self.cache.get(("ella_qkv",) + PackCache.ident(L.q.w, L.k.w, L.v.w, L.q.b, L.k.b, L.v.b), make))

    # -- the sub-program ----------------------------------------------------------------------------------------------------------
    def ella(self, node: Any, llm: Tensor, T: int, B: int) -> tuple[Tensor, int]:
        """ELLA = Passthrough(TimestepEncoder, UseContext llm_text_embedding, PerceiverResampler, SetContext ella.latents).
        llm: the static token buffer [B * Tp, input_dim] (Tp = T rounded up to 64, padding rows zero).  Called inside the step section.
        Returns (tokens [B * Nlp, out_width] with zero padding rows, Nl)."""
        ch = kids(node)
        _expect(isa(node, "ELLA") and len(ch) == 4 and isa(ch[0], "TimestepEncoder") and isa(ch[1], "UseContext") and isa(ch[2], "PerceiverResampler") and isa(ch[3], "SetContext"),
                "unexpected ELLA layout")
        _expect((ch[1].context, ch[1].key) == LLM_TOKENS and (ch[3].context, ch[3].key) == ELLA_TOKENS, "ELLA reads or writes an unexpected context")
        te = kids(ch[0])
        _expect(len(te) == 3 and isa(te[0], "UseContext") and (te[0].context, te[0].key) == ("diffusion", "timestep") and isa(te[1], "RangeEncoder") and isa(te[2], "SetContext")
                and (te[2].context, te[2].key) == ("ella", "timestep_embedding"), "unexpected ELLA TimestepEncoder layout")
        pr = kids(ch[2])
        _expect(len(pr) == 6 and isa(pr[0], "Linear", "Identity", "LoraAdapter") and isa(pr[1], "SetContext") and (pr[1].context, pr[1].key) == ("perceiver_resampler", "x")
                and isa(pr[2], "Latents") and isa(pr[3], "Residual") and isa(pr[4], "Transformer") and isa(pr[5], "OutputProjection", "Identity"), "unexpected PerceiverResampler layout")
        lc = kids(pr[2])
        _expect(len(lc) == 1 and isa(lc[0], "Parameter") and lc[0].weight.dim() == 2, "unexpected Latents layout")
        param = lc[0].weight
        Nl, C = param.shape
        Tp = llm.shape[0] // B
        _expect(T >= 1 and llm.shape[0] == B * Tp and Tp >= T, "LLM token buffer of another shape")
        _expect(C % 64 == 0, f"ELLA width {C} is no multiple of 64 (the transposed V group of the Q|K|V launch starts at column 2 C)")
        _expect(isa(pr[3], "Residual"), "unexpected latents time branch")
        lat_lin = _TimeLinear(self._ella_time_linear(pr[3]))
        _expect(lat_lin.lin.N == C and lat_lin.lin.b is not None, "the latents' time Linear has another width")
        layers = [self._ella_layer(l, C) for l in kids(pr[4])]
        _expect(len(layers) >= 1, "ELLA without layers")
        heads = layers[0].heads
        _expect(C % heads == 0 and self.head_kernel(C // heads) is not None, f"ELLA head dim {C / heads} is not served by mi355x_attention_general")

        # prompt side: the input projection of the LLM's tokens
        if isa(pr[0], "Identity"):
            _expect(llm.shape[1] == C, f"LLM embeddings of width {llm.shape[1]} into a resampler of width {C} without an input Linear")
            x = llm
        else:
            xin = self._ella_plain(pr[0])
            _expect(xin.K == llm.shape[1] and xin.N == C, f"LLM embeddings of width {llm.shape[1]}, the input Linear takes {xin.K}")
            with self.in_prologue():
                x = self.pool.get(B * Tp, C)
                self.pool.pin(x)
                self.linear(llm, xin, out=x)

        # the time table: every Linear that reads ella.timestep_embedding, as ONE GEMM
        readers = [lat_lin] + [r for L in layers for r in (L.ada_x, L.ada_l, L.ada_ff)]
        specs = [r.lin for r in readers]
        _expect(all(sp.K == specs[0].K for sp in specs), "ELLA time projections of different input widths")

        def stack() -> tuple[Tensor, Tensor]:
            return torch.cat([sp.w for sp in specs], 0).contiguous(), torch.cat([sp.b for sp in specs]).contiguous()

        tw, tb = self.cache.get(("ella_time",) + PackCache.ident(*[sp.w for sp in specs], *[sp.b for sp in specs]), stack)
        total = tw.shape[0]
        table = self.io.timesteps is not None and self.io.step_rows is not None and os.environ.get("REFINERS_AMD_TIME_TABLE", "1") != "0"
        trow = self.pool.get(B, total)
        if table:
            with self.in_prologue():
                temb = self._range_encoder(te[1], None, table=True)
                ts = self.pool.get(temb.shape[0], temb.shape[1])
                native.silu(temb, ts)
                self.pool.put(temb)
                tab = self.pool.get(ts.shape[0], total)
                self.pool.pin(tab)
                self.linear(ts, LinSpec(tw, tb), out=tab)
                self.pool.put(ts)
            native.gather_rows(tab, self.io.step_rows, trow)
        else:
            temb = self._range_encoder(te[1], None)
            ts = self.pool.get(B, temb.shape[1])
            native.silu(temb, ts)
            self.pool.put(temb)
            self.linear(ts, LinSpec(tw, tb), out=trow)
            self.pool.put(ts)
        off = 0
        for r in readers:
            r.cols = trow[:, off:off + r.lin.N]
            off += r.lin.N

        # latents = Parameter rows (broadcast over the batch) + their time row: one-hot rows against the transposed Parameter, exact in both dtypes
        Kp = (Nl + self.kblk - 1) // self.kblk * self.kblk

        def onehot() -> tuple[Tensor, Tensor]:
            pt = torch.zeros(C, Kp, device=self.device, dtype=self.dtype)
            sel = torch.zeros(B * Nl, Kp, device=self.device, dtype=self.dtype)
            if self.device.type != "meta":
                pt[:, :Nl] = param.detach().to(self.device, self.dtype).t()
                sel[torch.arange(B * Nl, device=self.device), torch.arange(B * Nl, device=self.device) % Nl] = 1.0
            return pt, sel

        pt, sel = self.cache.get(("ella_latents", B, Kp) + PackCache.ident(param), onehot)
        Nlp = pad64(Nl)
        proj = None
        if isa(pr[5], "OutputProjection"):
            oc = kids(pr[5])
            _expect(len(oc) == 2 and isa(oc[1], "LayerNorm"), "unexpected OutputProjection layout")
            proj = (self._ella_plain(oc[0]), oc[1])
            _expect(proj[0].K == C and tuple(oc[1].normalized_shape) == (proj[0].N,), "unexpected OutputProjection widths")
        # the result [B * Nlp, width'] is allocated zeroed once and only the Nl rows of every sample are ever written: its padding rows stay zero
        res = torch.zeros(B * Nlp, C if proj is None else proj[0].N, device=self.device, dtype=self.dtype)
        self.__dict__.setdefault("_keep", []).append(res)
        direct = proj is None and Nl == Nlp  # whole 64-row samples and no projection: the layers update the result buffer itself
        lat = res if direct else self.pool.get(B * Nl, C)
        native.gemm([(sel, pt)], lat, rowbias=lat_lin.cols, rows_per_group=Nl)

        Lp = pad64(Nl + T)
        lat3 = lat.view(B, Nl, C)
        x3 = x.as_strided((B, T, C), (Tp * x.stride(0), x.stride(0), 1))
        for L in layers:
            buf = self.pool.get(B * Lp, C)
            (sh_l, sc_l), (sh_x, sc_x) = L.ada_l.halves(), L.ada_x.halves()
            _expect(L.ada_l.eps == L.ada_x.eps, "the two AdaLayerNorms of one PerceiverAttention carry different epsilons")
            native.ella_adaln(lat3, sh_l, sc_l, buf.view(B, Lp, C), x=x3, shift_x=sh_x, scale_x=sc_x, eps=L.ada_l.eps)
            wqkv = self._ella_qkv(L, C)
            qk = self.pool.get(B * Lp, 2 * C)
            vt = self.pool.get(C, B * Lp)
            native.gemm([(buf, self.kblocked(wqkv.w))], qk, bias=wqkv.b, out_t=vt, nt_begin=2 * C)
            self.pool.put(buf)
            o = self.pool.get(B * Nl, C)
            q3 = qk.as_strided((B, Nl, C), (Lp * qk.stride(0), qk.stride(0), 1))
            k3 = qk[:, C:].as_strided((B, Lp, C), (Lp * qk.stride(0), qk.stride(0), 1))
            native.attention_general(q3, k3, vt.view(C, B, Lp), o.view(B, Nl, C), heads, Nl + T)
            self.pool.put(qk)
            self.pool.put(vt)
            self.linear(o, L.o, res=lat, out=lat)
            self.pool.put(o)
            h = self.pool.get(B * Nl, C)
            sh, sc = L.ada_ff.halves()
            native.ella_adaln(lat3, sh, sc, h.view(B, Nl, C), eps=L.ada_ff.eps)
            f = self.pool.get(B * Nl, L.f1.N)
            native.gemm([(h, self.kblocked(L.f1.w))], f, bias=L.f1.b, squared_relu=True)
            self.pool.put(h)
            self.linear(f, L.f2, res=lat, out=lat)
            self.pool.put(f)
        self.pool.put(trow)

        if not direct:
            y = lat if proj is None else self.linear(lat, proj[0])
            for b in range(1 if Nl == Nlp else B):  # (one launch when the samples are whole 64-row blocks)
                src, dst = (y, res) if Nl == Nlp else (y[b * Nl: (b + 1) * Nl], res[b * Nlp: b * Nlp + Nl])
                if proj is None:
                    native.axpby(src, 1.0, src, 0.0, dst)
                else:
                    native.layernorm(src, self._w(proj[1].weight), self._w(proj[1].bias), proj[1].eps, dst)
            if y is not lat:
                self.pool.put(y)
            self.pool.put(lat)
        self.stats["ella_layers"] = len(layers)
        return res, Nl

    def ella_child(self, node: Any, ctx: Any) -> None:
        """A top-level ELLA child of the UNet: its tokens become the step-produced stream ella.latents."""
        got = ctx.text.get(LLM_TOKENS)
        _expect(got is not None, "ELLA is injected but context adapted_cross_attention_block.llm_text_embedding is unset (call set_llm_text_embedding first)")
        llm, T = got
        tokens, Nl = self.ella(node, llm, T, ctx.B)
        ctx.text[ELLA_TOKENS] = (tokens, Nl)
        self.step_tokens.add(ELLA_TOKENS)
        self.stats["ella_sites"] = 0


# ------------------------------------------------------------------------------------------------ the resampler alone
class _Entry:
    def __init__(self, io: Any, llm: Tensor, out: Tensor, Nl: int, low: Any, program: Any) -> None:
        self.io, self.llm, self.out, self.Nl, self.low, self.program = io, llm, out, Nl, low, program


class CompiledELLA:
    """`fast = CompiledELLA(ella); latents = fast(timestep, llm_text_embedding)`: what the reference leaves in context ella.latents after
    `ella.set_context("diffusion", {"timestep": timestep}); ella.set_context("adapted_cross_attention_block", {"llm_text_embedding": e}); ella(x)`.
    timestep: one value shared by the batch, or [B, 1] / [B] per-row values; llm_text_embedding [B, T, input_dim] -> [B, num_latents, out_width].
    One lowered program and one HIP graph per (B, T), the last MAX_PROGRAMS shapes kept; the input projection (prompt side) runs again only when
    another embedding tensor is given.  An in-place edit of a weight re-lowers.  There is no fallback: a tree the lowering does not cover raises
    Unsupported."""

    def __init__(self, ella: Any, dtype: Optional[torch.dtype] = None, use_graph: bool = True) -> None:
        native.load()
        self.ella = ella
        self.dtype = dtype
        self.use_graph = use_graph
        self.cache = PackCache()
        self.entries: dict[Any, _Entry] = {}
        self.version: Any = None
        self.lowerings, self.prologue_runs = 0, 0
        self.prompt: Any = None
        self.stats: dict[str, Any] = {}

    def _version(self) -> tuple:
        return (tree_epoch(), sum(p._version for p in self.ella.parameters()))

    @torch.no_grad()
    def __call__(self, timestep: Any, llm_text_embedding: Tensor) -> Tensor:
        from .compiled import Program, _ident
        from .unet_lowering import UNetLowering

        e_in = llm_text_embedding
        assert e_in.dim() == 3, f"llm_text_embedding of shape {tuple(e_in.shape)}, expected [B, T, width]"
        B, T, Din = e_in.shape
        dev = e_in.device
        dtype = self.dtype or next(p.dtype for p in self.ella.parameters())
        version = self._version()
        if version != self.version:
            self.entries.clear()
            self.cache.used.clear()
            self.version, self.prompt = version, None
        key = (B, T, Din, dtype, dev)
        e = self.entries.get(key)
        if e is None:
            Tp = pad64(T)
            io = SimpleNamespace(timestep=torch.empty(B, device=dev, dtype=torch.float32), timesteps=None, step_rows=None)
            llm = torch.zeros(B * Tp, Din, device=dev, dtype=dtype)
            low = UNetLowering(dev, dtype, self.cache, "merged")
            low.io = io
            low.step_tokens = set()
            try:
                with low.in_step():
                    out, Nl = low.ella(self.ella, llm, T, B)
            except Unsupported as err:
                warnings.warn(f"CompiledELLA: {err}", RuntimeWarning, stacklevel=2)
                raise
            self.cache.sweep()
            self.lowerings += 1
            e = _Entry(io, llm, out, Nl, low, Program(low.step, self.use_graph, low=low))
            while len(self.entries) >= MAX_PROGRAMS:
                self.entries.pop(next(iter(self.entries)))
            self.entries[key] = e
            self.prompt = None
        ts = torch.as_tensor(timestep, dtype=torch.float32).to(dev).reshape(-1)
        assert ts.numel() in (1, B), f"timestep of {ts.numel()} values for a batch of {B}"
        e.io.timestep.copy_(ts.expand(B) if ts.numel() == 1 else ts)
        prompt = (key, _ident(e_in))
        if prompt != self.prompt:
            e.llm.view(B, -1, Din)[:, :T].copy_(e_in)
            native.replay(e.low.prologue)
            self.prologue_runs += 1
            self.prompt, self._prompt_ref = prompt, e_in  # (the tensor itself: a live tensor's address cannot be recycled, see compiled._ident)
        e.program.run()
        self.stats = dict(e.low.stats, step_ops=launches(e.low.step), prologue_ops=launches(e.low.prologue), lowerings=self.lowerings, prologue_runs=self.prologue_runs,
                          pool_bytes=e.low.step_pool.bytes() + e.low.prologue_pool.bytes())
        Nlp = e.out.shape[0] // B
        return e.out.view(B, Nlp, -1)[:, : e.Nl].clone()
