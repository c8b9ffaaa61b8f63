"""Golden vectors of MVANet's decoder blocks and of the whole net: the REAL reference's foundationals.swin.mvanet classes on CPU float32
in eval mode with the synthetic per-key weights of tests/mvanet_cases.py and seeded inputs.  Run where refiners' sources are
(REFINERS_SRC, else the copy __graft_entry__.build() stages under oracle/_ref/src); not on a GPU box:
    python tools/make_golden_mvanet.py
Writes tests/golden/mvanet_keys.json (per case the model's state-dict keys, in order, with their shapes) and
tests/golden/mvanet.safetensors, mvanet.1.safetensors, ... : block outputs whole as `<case>.out` (5, E, S, S), and for NET what
swin_cases.output_sample keeps of the logits and of the hooked Pyramid and RearrangeMultiView outputs.  A tensor over the shard size is
cut along dim 0; tests/support.golden joins the pieces.  Prints the softmax entropy of every attention (as a fraction of log Lk) and
refuses a draw that leaves one uniform (> 0.97) or one-hot (< 0.15)."""
from __future__ import annotations

import json
import math
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("REFINERS_SRC") or ROOT / "oracle" / "_ref" / "src")
sys.path[:0] = [str(ROOT / "oracle" / "shim"), str(REF), str(ROOT)]

import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

import refiners.foundationals.swin.mvanet.mclm as ref_mclm  # noqa: E402
import refiners.foundationals.swin.mvanet.mcrm as ref_mcrm  # noqa: E402
import refiners.foundationals.swin.mvanet.mvanet as ref_net  # noqa: E402

from tests.mvanet_cases import MVANET_CASES, NET_TENSORS, case_input, draw_weights, hook_net, views  # noqa: E402
from tests.swin_cases import output_sample  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SHARD_BYTES = 700_000
CLASSES = {"MCLM": ref_mclm.MCLM, "MCRM": ref_mcrm.MCRM, "MVANet": ref_net.MVANet}


def watch_entropy(model: torch.nn.Module, log: list) -> None:
    """A pre-hook on every MultiheadAttention that recomputes its softmax from (q, k) and records mean row entropy / log Lk."""
    def hook(m, args):
        q, k, _v = args
        e = m.embed_dim
        wq, wk = m.in_proj_weight[:e], m.in_proj_weight[e : 2 * e]
        qq = (q[:, 0] @ wq.T + m.in_proj_bias[:e]).double()
        kk = (k[:, 0] @ wk.T + m.in_proj_bias[e : 2 * e]).double()
        p = torch.softmax(qq @ kk.T / math.sqrt(e // m.num_heads), dim=-1)
        log.append((tuple(q.shape), k.shape[0], float(-(p * p.clamp_min(1e-300).log()).sum(-1).mean() / math.log(k.shape[0]))))

    for m in model.modules():
        if isinstance(m, torch.nn.MultiheadAttention):
            m.register_forward_pre_hook(hook)


def main() -> None:
    t0 = time.time()
    keys, out = {}, {}
    for name, (cls, kw, _side) in MVANET_CASES.items():
        model = CLASSES[cls](**kw).eval()
        shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
        keys[name] = {k: list(v) for k, v in shapes.items()}
        model.load_state_dict(draw_weights(shapes))
        entropies: list = []
        watch_entropy(model, entropies)
        sink: dict = {}
        if name == "NET":
            hook_net(model, sink)
        t1 = time.time()
        with torch.no_grad():
            y = model(case_input(name))
        dt = time.time() - t1
        assert torch.isfinite(y).all()
        for shape, lk, h in entropies:
            print(f"  {name}: attention {shape} x {lk} keys, entropy / log Lk = {h:.3f}")
            assert 0.15 < h < 0.97, f"degenerate attention in {name}: {h}"
        if name == "NET":
            sink["logits"] = y
            for t in NET_TENSORS:
                for k, v in output_sample(sink[t]).items():
                    out[f"{name}.{t}.{k}"] = v
                print(f"  {name}.{t} {tuple(sink[t].shape)} rms {float(sink[t].float().pow(2).mean().sqrt()):.3f}")
        else:
            out[f"{name}.out"] = views(y)
        print(name, tuple(y.shape), f"{len(shapes)} keys, {sum(v.numel() for v in model.state_dict().values()) / 1e6:.1f} M parameters, {dt:.2f}s")
    (GOLD / "mvanet_keys.json").write_text(json.dumps(keys))
    for old in GOLD.glob("mvanet*.safetensors"):
        old.unlink()
    shards: list[dict] = [{}]
    size = 0
    for k, v in out.items():
        row = v[0].numel() * v.element_size()
        i = 0
        while i < v.shape[0]:  # as many dim-0 slices as still fit (at least one), the rest into the next shard
            fit = max((SHARD_BYTES - size) // row, 0)
            if fit == 0 and shards[-1]:
                shards.append({})
                size = 0
                continue
            n = min(max(fit, 1), v.shape[0] - i)
            shards[-1][k] = v[i : i + n].contiguous()
            size += n * row
            i += n
            if i < v.shape[0]:
                shards.append({})
                size = 0
    for i, sh in enumerate(shards):
        path = GOLD / ("mvanet.safetensors" if i == 0 else f"mvanet.{i}.safetensors")
        save_file(sh, str(path))
        print(path.name, path.stat().st_size, "bytes")
    print(f"{time.time() - t0:.1f}s")


if __name__ == "__main__":
    main()
