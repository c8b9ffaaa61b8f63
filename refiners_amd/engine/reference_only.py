"""Reference-only control (reference latent_diffusion/reference_only_control.py; host mirror refiners_amd/latent_diffusion/reference_only.py)
lowered into the UNet's step program.

The adapter runs the UNet twice per step.  `SelfAttentionInjectionPassthrough`, the UNet's first child, runs a structural copy of the UNet on
the guide latents and keeps the input of every self-attention (the block's LayerNorm output, `self_attention_context_{i}.norm`); in the real
pass every `SelfAttentionInjectionAdapter` projects keys and values from cat(x, norm_i) and blends row 0 with the plain attention.

Two facts shape the lowering:

* structural_copy shares leaf modules, so the copy's Wk / Wv at site i ARE the real pass's: Wk norm_i and Wv norm_i are the K columns and the
  V^T buffer the guide pass projects for its own self-attention at that site.  They cost no GEMM and no concatenation; they are pinned until the
  real pass reaches the same site (the identity is checked per site, `Unsupported` otherwise).
* the blend happens before the out-projection (it is affine, the weights sum to 1): one `mi355x_attention_joint` launch per site gives
  s * A(q, [K ; Kg]) + (1 - s) * A(q, K) for row 0 and A(q, [K ; Kg]) for row 1, then the one out-projection GEMM with the residual as always.

The guide pass is lowered into the same step program, ahead of the real pass (one stream, one graph).  It reads the step input `io.guide`, reuses
the timestep embedding, the batched time biases and the prologue's text K / V^T (same Linears over the same tokens), and ENDS at the K | V^T
projection of the last site: the reference throws the guide pass's output away, and that site needs no Q.  `style_cfg` lives in device memory
(`ro_mix` = [style_cfg, 1]) and is refreshed by the engine before every replay."""
from __future__ import annotations

import dataclasses
from typing import Any, Optional

import torch
from torch import Tensor

from .. import native
from .packing import LinSpec, Unsupported, _expect, isa, kids, launches

#: adapters whose lowered form shares state with the self-attentions or the residual slots: not lowered together with reference-only control
_EXCLUSIVE = (("SelfAttentionMap", "Self-Attention Guidance"), ("SAGAdapter", "Self-Attention Guidance"), ("SharedSelfAttentionAdapter", "StyleAligned"),
              ("Controlnet", "a ControlNet"), ("T2IFeatures", "a T2I-Adapter"))


class GuideDone(Exception):
    """Raised by the guide pass's last self-attention site once its K | V^T are projected: nothing behind it is lowered."""


def _param_ids(*nodes: Any) -> tuple:
    return tuple(id(p) for n in nodes for p in n.parameters())


def _site_index(context: str) -> int:
    head, _, tail = context.rpartition("_")
    _expect(head == "self_attention_context" and tail.isdigit(), f"unexpected reference-only context name {context}")
    return int(tail)


class ReferenceOnlyLowering:
    """Mixin of UNetLowering: the guide pass (`reference_only_guide`) and the hooks BlockLowering.self_attention calls at an adapted site."""

    def reference_only_reset(self) -> None:
        self.ro_guide: dict[int, dict[str, Any]] = {}  # site -> the guide's K / V^T and what identifies their Linears
        self.ro_last = -1                              # index of the guide's last site (its Q is never projected)
        self.ro_time: Any = None                       # the guide copy's TimestepEncoder once lowered: the real pass's is the same computation
        self.ro_adapters: list[Any] = []               # the SelfAttentionInjectionAdapters met, for the engine to watch their style_cfg
        self.ro_mix: Optional[Tensor] = None           # float32 [2] on the device: [style_cfg, 1]
        self.ro_mix_value: Optional[float] = None
        self.kv_memo: Optional[dict] = None            # text K / V^T of the prologue by their Linears: projected once for both passes

    # -- the guide pass ------------------------------------------------------------------------------------------
    def reference_only_guide(self, node: Any, unet: Any, ctx: Any, H: int, W: int) -> None:
        from .unet_lowering import UNetContext

        io = self.io
        B = ctx.B
        _expect(B == 2, f"reference-only control assumes one classifier-free-guidance pair (a batch of 2), got a batch of {B}")
        _expect(not self.style_half_batch, "reference-only control on one half of a split classifier-free-guidance pair (cfg_split / io_override) is not lowered")
        for cls, what in _EXCLUSIVE:
            _expect(not any(isa(m, cls) for m in unet.modules()), f"reference-only control together with {what} is not lowered")
        ch = kids(node)
        _expect(len(ch) == 4 and isa(ch[0], "Lambda") and isa(ch[3], "Lambda") and isa(ch[1], "UseContext") and (ch[1].context, ch[1].key) == ("reference_only_control", "guide")
                and isa(ch[2], "Chain"), "unexpected SelfAttentionInjectionPassthrough layout")
        _expect(io.guide is not None, "context reference_only_control.guide is unset (call set_controlnet_condition first)")
        _expect(tuple(io.guide.shape) == tuple(io.x.shape), f"the guide is {tuple(io.guide.shape)}, the UNet input {tuple(io.x.shape)}: reference-only control needs a guide of the input's shape")
        guide_unet = ch[2]
        sites = [m for m in guide_unet.modules() if isa(m, "SaveLayerNormAdapter")]
        _expect(len(sites) > 0 and sorted(_site_index(m.context) for m in sites) == list(range(len(sites))), "the guide UNet's self-attentions are not numbered 0 .. n - 1")
        self.ro_last = len(sites) - 1
        self.ro_mix_value = None
        self.kv_memo = {}
        sub = UNetContext(self, B, text=ctx.text, temb_silu=ctx.temb_silu, temb_table=ctx.temb_table, time_table=ctx.time_table, residuals=[None] * len(ctx.residuals), shapes=[])
        before, lora_sites = launches(self.step), self.stats["lora_sites"]
        self.io = dataclasses.replace(io, x=io.guide)  # (the stem reads io.x)
        try:
            self.walk(guide_unet, sub, H, W)
            raise Unsupported("the guide UNet ended before its last self-attention")
        except GuideDone:
            pass
        finally:
            self.io = io
        _expect(len(self.ro_guide) == len(sites), "the guide pass did not reach every self-attention")
        self.ro_time = next((c for c in kids(guide_unet) if isa(c, "TimestepEncoder")), None)
        for a in sub.residuals:  # the copy's skip tensors die with it: back to the pool for the real pass
            if a is not None:
                self.pool.unpin(a.t)
                self.pool.put(a.t)
        self.stats["lora_sites"] = lora_sites  # (the same Linears are counted by the real pass)
        self.stats["reference_only_guide_ops"] = launches(self.step) - before

    def reference_only_same_time(self, node: Any) -> bool:
        """The real pass's TimestepEncoder when the guide pass has produced its embedding (the copy shares the leaves)."""
        return self.ro_time is not None and _param_ids(self.ro_time) == _param_ids(node)

    # -- sites ---------------------------------------------------------------------------------------------------
    def reference_only_site(self, att: Any) -> tuple[Any, tuple[str, int, Any]]:
        """SaveLayerNormAdapter | SelfAttentionInjectionAdapter -> (the SelfAttention inside, (kind, site, adapter))."""
        ch = kids(att)
        if isa(att, "SaveLayerNormAdapter"):
            _expect(len(ch) == 2 and isa(ch[0], "SetContext") and ch[0].key == "norm" and isa(ch[1], "SelfAttention"), "unexpected SaveLayerNormAdapter layout")
            _expect(self.kv_memo is not None, "SaveLayerNormAdapter outside a reference-only guide pass")
            site = _site_index(ch[0].context)
            _expect(site == len(self.ro_guide), "the guide pass meets its self-attentions out of order")
            return ch[1], ("save", site, att)
        _expect(len(ch) == 2 and isa(ch[0], "Parallel") and isa(ch[1], "Lambda") and len(kids(ch[0])) == 2, "unexpected SelfAttentionInjectionAdapter layout")
        guided, plain = kids(ch[0])
        pc = kids(plain)
        _expect(isa(guided, "SelfAttention") and isa(plain, "Chain") and len(pc) == 2 and isa(pc[0], "Lambda") and isa(pc[1], "SelfAttention"), "unexpected SelfAttentionInjectionAdapter branches")
        gc = kids(guided)
        _expect(len(gc) == 4 and isa(gc[0], "Parallel") and len(kids(gc[0])) == 3 and isa(kids(gc[0])[0], "Identity"), "unexpected guided SelfAttention layout")
        contexts = set()
        for cat in kids(gc[0])[1:]:
            cc = kids(cat)
            _expect(isa(cat, "Concatenate") and cat.dim == 1 and len(cc) == 2 and isa(cc[0], "Identity") and isa(cc[1], "UseContext") and cc[1].key == "norm",
                    "the guided keys / values are not Concatenate(Identity, UseContext norm) along the tokens")
            contexts.add(cc[1].context)
        _expect(len(contexts) == 1 and contexts == {att.context}, "keys and values of one site read different guide contexts")
        _expect(_param_ids(*gc[1:]) == _param_ids(*kids(pc[1])[1:]), "the guided and the plain SelfAttention of one site do not share their Linears")
        site = _site_index(att.context)
        _expect(site in self.ro_guide, f"no guide pass has produced the keys of {att.context} (SelfAttentionInjectionPassthrough is not the UNet's first child)")
        self.ro_adapters.append(att)
        return pc[1], ("inject", site, att)

    def reference_only_keep(self, site: int, owner: Tensor, k: Tensor, vt: Tensor, L: int, kn: Any, vn: Any) -> None:
        """Guide pass: K (a column slice of `owner` where Q | K are one buffer) and V^T of this site outlive it, until the real pass's same site."""
        self.pool.pin(owner)
        self.pool.pin(vt)
        self.ro_guide[site] = {"k": k, "vt": vt, "L": L, "owner": owner, "ids": _param_ids(kn, vn)}

    def reference_only_last(self, site: int, x: Tensor, ln: Any, ks: LinSpec, vs: LinSpec, kn: Any, vn: Any, B: int, L: int) -> None:
        """The guide's last site: K and V^T only (no Q, no attention, nothing behind it), then the guide pass is over.  Two launches on a materialised
        LayerNorm: SD1.5's last site has 320 channels, which the transposed column group of a merged K | V^T GEMM (multiples of 128) does not take."""
        C = x.shape[1]
        h = self.layernorm(x, ln)
        k = self.linear(h, ks)
        vt = self._project_vt(h, vs, B, L, C)
        self.pool.put(h)
        self.pool.put(x)  # the copy's hidden state dies here (the stage's input is released by UNetLowering.piece on the way out)
        self.reference_only_keep(site, k, k, vt, L, kn, vn)
        raise GuideDone

    def reference_only_attention(self, site: int, adapter: Any, q: Tensor, k: Tensor, vt: Tensor, B: int, heads: int, L: int, kn: Any, vn: Any) -> Tensor:
        """Real pass: the joint attention over the sample's own keys and the guide's of the same site; the guide's buffers go back to the pool."""
        g = self.ro_guide[site]
        _expect(g["ids"] == _param_ids(kn, vn), "the key / value Linears of the guide pass and the real pass are not the same modules: the guide's K / V^T are not the extra keys")
        M, C = q.shape
        _expect(g["L"] == L and g["k"].shape == k.shape, "the guide's keys have another length than the sample's")
        if self.ro_mix_value is None:  # one weight for the whole UNet, in device memory: the engine rewrites it when style_cfg is assigned
            self.ro_mix_value = float(adapter.style_cfg)
            self.ro_mix = torch.tensor([self.ro_mix_value, 1.0], device=self.device, dtype=torch.float32)
        _expect(float(adapter.style_cfg) == self.ro_mix_value, "the self-attention injections of one UNet carry different style_cfg")
        rows3 = lambda t: t.as_strided((B, L, C), (L * t.stride(0), t.stride(0), 1))  # noqa: E731  (k may be a column slice of a [Q | K] buffer)
        cols3 = lambda t: t.as_strided((C, B, t.shape[1] // B), (t.stride(0), t.shape[1] // B, 1))  # noqa: E731
        out = self.pool.get(M, C)
        native.attention_joint(rows3(q), rows3(k), cols3(vt), L, rows3(g["k"]), cols3(g["vt"]), L, out.view(B, L, C), heads, mix=self.ro_mix)
        for t in (g["owner"], g["vt"]):
            self.pool.unpin(t)
            if L % 64 == 0 or t is g["owner"]:  # (a V^T with padded samples is no pool buffer: BlockLowering._project_vt)
                self.pool.put(t)
        g["k"] = g["vt"] = g["owner"] = None
        self.stats["reference_only_sites"] = self.stats.get("reference_only_sites", 0) + 1
        return out
