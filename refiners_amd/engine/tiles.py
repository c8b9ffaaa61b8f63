"""The tile configurations of mi355x_gemm (mi355x_gemm_args.tile), one row per id: the Python copy of the table in csrc/gemm_tiles.cuh, where the fields are
described (tests/test_gemm_tiles_cpu.py keeps the two equal).  Everything on the Python side that needs to know what an id means reads it from here."""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class Tile:
    id: int
    loop: int  # 4 = the 4-wave kernel, 8 = the 8-wave / eight-phase loop
    bm: int
    bn: int
    bm2: int
    kgroups: int
    streamk: int
    f32: int
    conv: int
    lora: int
    trans: int
    plain: int
    st_lo: int
    st_hi: int
    lora_to: int
    fallback: int


# fmt: off
#         id loop  bm   bn  bm2 kg sk f32 conv lora trans plain st    lora_to fallback
TILES = (
    Tile(1,  4,  128, 128,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    1,      0),
    Tile(2,  4,  128,  64,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    2,      0),
    Tile(3,  4,   64, 128,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    3,      0),
    Tile(4,  4,   64,  64,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    4,      0),
    Tile(6,  4,  128, 128,   0, 2, 0,  1,  1,   0,   1,    0,  2, 2,    1,      1),
    Tile(7,  8,  256, 256,   0, 1, 0,  1,  1,   1,   1,    0,  0, 0,    7,      0),
    Tile(8,  8,  256, 256,   0, 1, 1,  1,  1,   1,   1,    0,  0, 0,    7,      7),
    Tile(9,  8,  192, 256,   0, 1, 0,  1,  1,   1,   0,    0,  0, 0,    9,      0),
    Tile(10, 8,  128, 256,   0, 1, 0,  0,  0,   1,   0,    0,  0, 0,    7,      0),
    Tile(11, 8,  192, 256, 128, 1, 0,  0,  0,   1,   0,    0,  0, 0,    1,      9),
    Tile(12, 8,  128, 320,   0, 1, 0,  0,  1,   0,   0,    1,  0, 0,    7,      0),
)
# fmt: on
BY_ID = {t.id: t for t in TILES}
IDS_4WAVE = tuple(t.id for t in TILES if t.loop == 4)
IDS_8WAVE = tuple(t.id for t in TILES if t.loop == 8)


def takes_whole_k(tile: int) -> bool:
    """The 8-wave loop needs no split along K (whole tiles or stream-K): mi355x_gemm drops a caller's split where this tile takes the launch."""
    return tile in BY_ID and BY_ID[tile].loop == 8


def needs_streamk_scratch(tile: int) -> bool:
    return tile in BY_ID and BY_ID[tile].streamk == 1


def g8_takes_lora(kind: str, nseg: int, groups: int, transposed: bool) -> bool:
    """The 8-wave loop's in-launch LoRA: ONE column group of a plain one-segment GEMM without a transposed group."""
    return kind == "gemm" and nseg == 1 and groups == 1 and not transposed


def takes(t: Tile, a) -> bool:
    """Does row t take launch `a` (a native.GemmArgs) as it is -- the library's rules (gemm8_ok / resolve_tile / launch_tile in csrc) on the fields a caller sets?"""
    lora, trans = bool(a.lora_b), bool(a.out_t)
    if (a.dtype == 0 and not t.f32) or (a.conv and not t.conv) or (trans and not t.trans) or (lora and not t.lora):  # (dtype 0: MI355X_F32)
        return False
    if t.plain and (lora or a.geglu == 1 or a.ln_stats or a.stats_out or a.out_f32):
        return False
    if t.loop == 8:
        if trans and a.nt_begin % 256:  # (a split along K is no obstacle: the loop takes the whole K)
            return False
        return not lora or g8_takes_lora("conv" if a.conv else "gemm", a.nseg, a.lora_groups, trans)
    return not ((a.geglu == 1 or (lora and a.lora_r > 64)) and t.bn < 128)  # the GEGLU epilogue and a stacked rank above 64 need the 128-column tiles


def lora_choice(tile: int, g8_lora: bool) -> tuple[int, int]:
    """(tile, stages) of a LoRA launch whose un-adapted shape class was measured on `tile`.  g8_lora: the 8-wave loop's LoRA takes this launch."""
    if tile not in BY_ID:
        return 0, 2
    to = BY_ID[BY_ID[tile].lora_to]
    if to.loop == 8:
        return (to.id, 0) if g8_lora else (1, 2)
    return to.id, 2  # (the 4-wave LoRA kernels have two LDS stages)


def stat(tile: int) -> str:
    """The mi355x_get_stat counter that moves when a launch runs on this id of the 8-wave loop ("g8" counts every launch of the loop)."""
    return f"g{tile}" if tile in (9, 11, 12) else "g8"
