"""Cases of the MVANet fixtures (tests/golden/mvanet_keys.json, mvanet.safetensors and its shards, written by tools/make_golden_mvanet.py
from the reference's own classes): the blocks at the smallest sizes they run at, the whole net at the one shape it admits, the synthetic
weight draw and the seeded inputs."""
from __future__ import annotations

import json
from functools import lru_cache
from pathlib import Path

MVANET_SEED = dict(weight_seed=17, input_seed=43)
E = 128

#: name -> (class name, keywords).  MCRM keys per view: (S / 2)^2 * 21 / 16 -> 21 (less than one 64-key tile), 84 (one tile and a tail),
#: 336 (five tiles and a tail).  NET is not reducible: the reference's geometry is hard-wired; shallow depths keep it to seconds.
MVANET_CASES = {
    "MCLM": ("MCLM", dict(emb_dim=E), 16),
    "MCRM8": ("MCRM", dict(emb_dim=E, size=8), 8),
    "MCRM16": ("MCRM", dict(emb_dim=E, size=16), 16),
    "MCRM32": ("MCRM", dict(emb_dim=E, size=32), 32),
    "NET": ("MVANet", dict(depths=[2, 2, 2, 2]), 1024),
}
BLOCK_CASES = [c for c in MVANET_CASES if c != "NET"]
#: the tensors NET's fixture keeps (what swin_cases.output_sample keeps of each): the result and two hooked intermediates
NET_TENSORS = ["logits", "pyramid", "rearrange"]
WINDOW_SIZE = 12


def case_input(case: str):
    """Blocks: (1, 5, E, S, S) views.  NET: one (1, 3, 1024, 1024) image."""
    import torch

    side = MVANET_CASES[case][2]
    g = torch.Generator().manual_seed(MVANET_SEED["input_seed"] + sum(map(ord, case)))
    return torch.randn((1, 3, side, side) if case == "NET" else (1, 5, E, side, side), generator=g)


@lru_cache(maxsize=None)
def key_shapes(case: str) -> dict[str, tuple[int, ...]]:
    gold = Path(__file__).resolve().parent / "golden"
    return {k: tuple(v) for k, v in json.loads((gold / "mvanet_keys.json").read_text())[case].items()}


def draw_weights(shapes: dict) -> dict:
    """synth.synth_state_dict over the key / shape list, except: canonical relative_position_index and bias tables of standard deviation 0.5
    (as tests/swin_cases.py); BatchNorm running_var in [0.5, ...) and an integer num_batches_tracked; PReLU slopes around 0.25; the Q and
    K rows of every in_proj_weight with gain 2, which leaves the softmax neither uniform nor one-hot on pooled keys."""
    import torch

    from refiners_amd import synth
    from refiners_amd.swin import canonical_relative_position_index

    seed = MVANET_SEED["weight_seed"]
    sd = synth.synth_state_dict(shapes, seed)
    for k, s in shapes.items():
        if k.endswith("relative_position_index"):
            sd[k] = canonical_relative_position_index(WINDOW_SIZE)
            assert tuple(sd[k].shape) == tuple(s)
        elif k.endswith("relative_position_bias_table"):
            sd[k] = synth.synth_tensor(k, s, seed, gain=0.5 * s[1] ** 0.5)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + 10 * sd[k].abs()
        elif k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3, dtype=torch.int64)
        elif k.endswith("PReLU.weight"):
            sd[k] = 0.25 + 0.5 * sd[k]
        elif k.endswith("in_proj_weight"):
            sd[k] = torch.cat([2.0 * sd[k][: 2 * s[1]], sd[k][2 * s[1] :]])
    return sd


def weights(case: str) -> dict:
    return draw_weights(key_shapes(case))


def build(case: str, namespace=None, device="cpu", dtype=None):
    """The case's model from `namespace` (default: the mirror, refiners_amd.mvanet) in eval mode with the fixture's weights loaded."""
    import torch

    if namespace is None:
        from refiners_amd import mvanet as namespace
    dtype = dtype or torch.float32
    cls, kw, _side = MVANET_CASES[case]
    model = getattr(namespace, cls)(**kw, device="meta")
    sd = {k: v.to(device=device, dtype=dtype if v.is_floating_point() else None) for k, v in weights(case).items()}
    model.load_state_dict(sd, assign=True)
    return model.eval()


def views(y):
    """A block's (1, 5, E, S, S) output as the (5, E, S, S) tensor the fixture stores whole."""
    return y.detach().float().cpu().flatten(0, 1).contiguous()


def hook_net(model, sink: dict) -> list:
    """Forward hooks that drop the Pyramid and RearrangeMultiView outputs of an MVANet into `sink` as (B, C, H, W) tensors."""
    def keep(name):
        def fn(_m, _inp, out):
            sink[name] = out.detach().flatten(0, 1) if out.dim() == 5 else out.detach()
        return fn

    mods = {type(m).__name__: m for m in model.modules()}
    return [mods["Pyramid"].register_forward_hook(keep("pyramid")), mods["RearrangeMultiView"].register_forward_hook(keep("rearrange"))]
