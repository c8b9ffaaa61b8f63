"""The tile table of mi355x_gemm: csrc/gemm_tiles.cuh (what the library dispatches from) and engine/tiles.py (what tuning, the tuner and the reports read) hold the
same rows, nothing in csrc binds an id the table does not know, and the Python consumers of the table decide what they decided before it existed."""
import dataclasses
import importlib.util
import re
from pathlib import Path
from types import SimpleNamespace

import pytest

from refiners_amd.engine import tiles, tuning

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "refiners_amd" / "csrc"


def header_rows():
    src = (CSRC / "gemm_tiles.cuh").read_text()
    rows = [tuple(int(v) for v in m.group(1).split(",")) for m in re.finditer(r"^\s*TILE\(([\d,\s]+)\),", src, re.M)]
    names = [n.strip() for n in re.search(r"#define TILE\(([^)]*)\)", src).group(1).split(",")]
    return names, rows


def test_the_header_and_the_python_table_hold_the_same_rows():
    names, rows = header_rows()
    assert names == [f.name for f in dataclasses.fields(tiles.Tile)]
    assert rows == [dataclasses.astuple(t) for t in tiles.TILES]
    assert len(rows) == 11 and len({r[0] for r in rows}) == len(rows)  # one row per id
    for t in tiles.TILES:  # a row only points at rows
        assert t.lora_to in tiles.BY_ID and (t.fallback == 0 or t.fallback in tiles.BY_ID), t
        assert t.loop in (4, 8) and t.st_lo <= t.st_hi and ((t.st_lo, t.st_hi) == (0, 0)) == (t.loop == 8), t


def switch_bodies(src: str, head: str):
    for m in re.finditer(re.escape(head) + r" \{", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(src[i], 0)
            i += 1
        yield src[m.end():i]


def test_no_source_binds_an_id_the_table_does_not_list():
    """Product code names table ids only; a probing build's extra tiles (-DMI355X_PROBE_T10) sit at 20 and above, each id once, so that no build answers a
    product id with a probing tile."""
    known = set(tiles.BY_ID)
    probe = []
    for path in sorted(CSRC.glob("*.cuh")) + sorted(CSRC.glob("*.hip")):
        src = path.read_text()
        named = [int(v) for v in re.findall(r"\b(?:tile|t\.id)\s*==\s*(\d+)|find_tile\((\d+)\)", src) for v in v if v]
        for head in ("switch (tile)", "switch (t.id)"):
            for body in switch_bodies(src, head):
                named += [int(v) for v in re.findall(r"case (\d+):", body)]
        assert set(named) <= known, (path.name, sorted(set(named) - known))
        forced, hinted = ([int(v) for v in re.findall(pat + r"\s*==\s*(\d+)", src)] for pat in (r"\bg_tile", r"\btile_hint"))
        assert forced == hinted, path.name  # (a probing tile answers the option and the caller's hint alike)
        probe += forced
    assert probe and len(set(probe)) == len(probe) and min(probe) >= 20 and not set(probe) & known, probe


def launch(**kw):
    d = dict(dtype=1, conv=0, nseg=1, lora_b=None, lora_groups=0, lora_r=0, out_t=None, nt_begin=0, geglu=0, ln_stats=None, stats_out=None, out_f32=0, ksplit=1)
    d.update(kw)
    return SimpleNamespace(**d)


G8, W4 = [(7, 0), (8, 0), (9, 0)], [(t, s) for t in (1, 2, 3, 4) for s in (2, 3, 4)] + [(6, 2)]
W4_WIDE = [(t, s) for t in (1, 3) for s in (2, 3, 4)] + [(6, 2)]
LORA4 = [(1, 2), (2, 2), (3, 2), (4, 2)]
#: what tools/autotune.py's candidates() returned at the commit before the table (its own literal rules), in its order
CANDIDATES = {
    "plain": (launch(), G8 + [(12, 0)] + W4),
    "lora, one group": (launch(lora_b=1, lora_groups=1, lora_r=32), [(7, 0), (9, 0)] + LORA4),
    "lora, one group, rank 128": (launch(lora_b=1, lora_groups=1, lora_r=128), [(7, 0), (9, 0), (1, 2), (3, 2)]),
    "lora, three groups": (launch(lora_b=1, lora_groups=3, lora_r=32, out_t=1, nt_begin=256), LORA4),
    "lora, two segments": (launch(nseg=2, lora_b=1, lora_groups=1, lora_r=64), LORA4),
    "transposed from a multiple of 256": (launch(out_t=1, nt_begin=512), [(7, 0), (8, 0)] + W4),
    "transposed from 384": (launch(out_t=1, nt_begin=384), W4),
    "geglu": (launch(geglu=1), G8 + W4_WIDE),
    "gelu": (launch(geglu=2), G8 + [(12, 0)] + W4),
    "ln-folded": (launch(ln_stats=1), G8 + W4),
    "row statistics": (launch(stats_out=1), G8 + W4),
    "float32 output": (launch(out_f32=1), G8 + W4),
    "conv": (launch(conv=1), G8 + [(12, 0)] + W4),
    "conv with lora": (launch(conv=1, lora_b=1, lora_groups=1, lora_r=32), LORA4),
    "float32": (launch(dtype=0), G8 + W4),
    "float32 conv": (launch(dtype=0, conv=1), G8 + W4),
    "split-K conv": (launch(conv=1, ksplit=3), G8 + [(12, 0)]),
    "split-K float32": (launch(dtype=0, ksplit=2), G8),
}


@pytest.fixture(scope="module")
def autotune():
    spec = importlib.util.spec_from_file_location("autotune_under_test", ROOT / "tools" / "autotune.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("name", list(CANDIDATES))
def test_the_tuner_proposes_what_it_proposed(autotune, name):
    a, want = CANDIDATES[name]
    assert autotune.candidates(a) == want
    assert autotune.candidates(a, {1, 7, 8}) == [c for c in want if c[0] in (1, 7, 8)]


def test_the_split_and_the_scratch_follow_the_table():
    assert [t for t in range(16) if tiles.takes_whole_k(t)] == [7, 8, 9, 10, 11, 12] == list(tiles.IDS_8WAVE)
    assert [t for t in range(16) if tiles.needs_streamk_scratch(t)] == [8]
    assert tiles.IDS_4WAVE == (1, 2, 3, 4, 6)


#: tuning.lookup at the commit before the table, for an un-adapted entry (id, stages): the LoRA launch of a plain one-segment GEMM, of any other launch (two
#: segments, convolution, transposed group), and the same two with tuning.lora_g8 off
LORA_LOOKUP = {
    1: ((1, 2), (1, 2), (1, 2), (1, 2)),
    2: ((2, 2), (2, 2), (2, 2), (2, 2)),
    3: ((3, 2), (3, 2), (3, 2), (3, 2)),
    4: ((4, 2), (4, 2), (4, 2), (4, 2)),
    6: ((1, 2), (1, 2), (1, 2), (1, 2)),
    7: ((7, 0), (1, 2), (1, 2), (1, 2)),
    8: ((7, 0), (1, 2), (1, 2), (1, 2)),
    9: ((9, 0), (1, 2), (1, 2), (1, 2)),
    10: ((7, 0), (1, 2), (1, 2), (1, 2)),
    11: ((1, 2), (1, 2), (1, 2), (1, 2)),
    12: ((7, 0), (1, 2), (1, 2), (1, 2)),
}
SIGNATURES = {"gemm:bf16:8x8x8:s1:": 0, "gemm:bf16:8x8x16:s2:": 1, "conv:bf16:8x8x72:s1:": 1, "gemm:bf16:8x24x8:s1:T16ln": 1}


@pytest.mark.parametrize("tile", [t.id for t in tiles.TILES])
def test_lookup_hands_lora_launches_what_it_handed_them(monkeypatch, tile):
    assert set(LORA_LOOKUP) == set(tiles.BY_ID)
    monkeypatch.setattr(tuning, "enabled", True)
    row = tiles.BY_ID[tile]
    for stages in range(row.st_lo, row.st_hi + 1):
        for sig, col in SIGNATURES.items():
            monkeypatch.setattr(tuning, "_table", {sig: (tile, stages)})
            monkeypatch.setattr(tuning, "lora_g8", True)
            assert tuning.lookup(sig) == (tile, stages)
            assert tuning.lookup(sig + "lora") == LORA_LOOKUP[tile][col], (sig, stages)
            monkeypatch.setattr(tuning, "lora_g8", False)
            assert tuning.lookup(sig + "lora") == LORA_LOOKUP[tile][2 + col], (sig, stages)
