"""Cases of the recorded solver-step bits (tests/golden/solver_step_bits.safetensors, written by tools/make_golden_step_bits.py from the library
of the commit BEFORE the six entry points moved onto one kernel; read by tests/test_solver_step_kernels_gpu.py).  2 storage types x 4 layouts x
6 entry points = 48 records, the smallest that reach every loop of the kernels on either side of that change:
    16x16   1 x 4 x 16 x 16 (1024 elements)  whole 16-byte vectors everywhere
    5x7     1 x 4 x 5 x 7 (140)              guided bfloat16: 140 % 8 != 0, the conditional half sits off a vector boundary (element loop throughout);
                                             guided float32: 35 whole vectors; guidance-free bfloat16: 17 vectors and a 4-element tail
    3x7     1 x 3 x 3 x 7 (63)               a tail in both types; guided: element loop throughout
    5x7+1   140 elements, every operand one element off a 16-byte boundary
A file holds, per (type, layout), the inputs `<type>.<layout>.in.{x,unet_out,hist,noise}` (unet_out: 2n rows, independent halves, so the guidance
fma sees c - u != 0; a guidance-free entry point reads the first half), per entry point `<type>.<layout>.<entry>.{x,hist,model_in}`, and the two
coefficient rows `coef.linear` (9 floats) and `coef.ddim` (8)."""
from __future__ import annotations

from pathlib import Path

import torch

GOLD = Path(__file__).resolve().parent / "golden" / "solver_step_bits.safetensors"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
#: layout -> (latent shape, offset of every operand from a 16-byte boundary, in elements)
LAYOUTS = {"16x16": ((1, 4, 16, 16), 0), "5x7": ((1, 4, 5, 7), 0), "3x7": ((1, 3, 3, 7), 0), "5x7+1": ((1, 4, 5, 7), 1)}
#: entry point -> (rows of unet_out and model_in per row of x, coefficient row, reads hist, reads noise, has a model-input operand)
ENTRIES = {
    "cfg_ddim_step": (2, "ddim", False, False, False),
    "cfg_linear_step": (2, "linear", True, False, True),
    "ddim_step": (1, "ddim", False, False, True),
    "linear_step": (1, "linear", True, False, True),
    "cfg_sde_step": (2, "linear", True, True, True),
    "sde_step": (1, "linear", True, True, True),
}
LINEAR_ROW = (7.5, 0.7, -0.3, 1.1, -0.4, 0.25, 0.15, 0.83, 0.37)  # (cfg, hx, he, kx, ke, kd, kp, s_next, kn): every term live
CFG = 7.5


def coefficient_rows() -> dict[str, torch.Tensor]:
    from refiners_amd.latent_diffusion.sampling import DDIM

    return {"coef.linear": torch.tensor(LINEAR_ROW, dtype=torch.float32), "coef.ddim": torch.tensor([CFG, *DDIM(4).coefficients(1), 0.0, 0.0, 0.0], dtype=torch.float32)}


def inputs(dtype: torch.dtype, layout: str) -> dict[str, torch.Tensor]:
    """The four input tensors of one (type, layout): a CPU generator with a fixed seed, cast to the storage type."""
    shape, _ = LAYOUTS[layout]
    g = torch.Generator().manual_seed(20 + list(LAYOUTS).index(layout))
    draw = lambda rows: torch.randn((rows * shape[0],) + shape[1:], generator=g).to(dtype)  # noqa: E731
    return {"x": draw(1), "unet_out": draw(2), "hist": draw(1), "noise": draw(1)}


def _place(t: torch.Tensor, off: int, device: str) -> torch.Tensor:
    """A contiguous device copy of `t` that starts `off` elements behind a 16-byte boundary."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=device)
    view = buf[off:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (off * t.element_size()) % 16 and view.is_contiguous()
    return view


def run(native, entry: str, layout: str, inp: dict[str, torch.Tensor], coefs: dict[str, torch.Tensor], device: str = "cuda") -> dict[str, torch.Tensor]:
    """Calls the public wrapper `native.<entry>` on operands rebuilt from `inp`; returns what it wrote, on the CPU."""
    rows, row, has_hist, has_noise, has_model_in = ENTRIES[entry]
    off = LAYOUTS[layout][1]
    n0 = inp["x"].shape[0]
    x = _place(inp["x"], off, device)
    uo = _place(inp["unet_out"][: rows * n0], off, device)
    coef = coefs[f"coef.{row}"].to(device)
    args = [x, uo]
    out = {"x": x}
    if has_hist:
        out["hist"] = _place(inp["hist"], off, device)
        args.append(out["hist"])
    if has_noise:
        args.append(_place(inp["noise"], off, device))
    if has_model_in:
        out["model_in"] = _place(torch.zeros_like(inp["unet_out"][: rows * n0]), off, device)
        args.append(out["model_in"])
    getattr(native, entry)(*args, coef)
    return {k: v.cpu().contiguous() for k, v in out.items()}
