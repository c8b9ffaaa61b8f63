"""Index arithmetic of tile id 12 -- the 8-wave loop on 128 x 320 tiles (refiners_amd/csrc/gemm8_kernel.cuh with NT = 5) -- restated in Python and checked on
the CPU: the W-slot loader against the fragment reads and the 16 + 4 columns a lane hands to the epilogue, the counted waits, the LDS budget, the 4-column
column-statistics reduction, and the grid (plan_grid + tile_coords) for every SDXL shape it is meant for: whole dispatch rounds on 256 CUs, every output
element covered exactly once, the same number of tiles on each of the 8 XCDs."""
import pytest

NT, MT = 5, 4
BM, BN, WC = 32 * MT, 64 * NT, 16 * NT
NW0, NW1 = 3, 2  # 16-row W blocks per wave in W half 0 / 1 (= loads per thread of that half tile)


def w_rb(h, s2, wid):  # gemm8_kernel.cuh w_rb: the 8-row block of the W slot that wave wid fills with load s2 of W half h
    nb8 = 2 * (NW1 if h else NW0)
    q = 8 * s2 + wid
    return (WC // 8) * (q // nb8) + 2 * NW0 * h + q % nb8


def w_src(R):  # gemm8_kernel.cuh wrow (NT = 5): the weight row (output column) LDS row R of the W slot holds
    wc, rl = divmod(R, WC)
    j, rr = rl >> 4, rl & 15
    return wc * WC + (16 * (rr >> 2) + 4 * j + (rr & 3) if j < 4 else 64 + rr)


def staged_w_slot():
    holds, phys = {}, {}
    for h in range(2):
        for s2 in range(NW1 if h else NW0):
            for wid in range(8):
                for lane in range(64):
                    R = 8 * w_rb(h, s2, wid) + (lane >> 3)
                    assert ((R >> 1) & 7) == 4 * (wid & 1) + (lane >> 4), "the loader's one-offset-per-thread swizzle"
                    assert holds.setdefault(R, (w_src(R), h)) == (w_src(R), h)
                    key = (R, lane & 7)
                    assert key not in phys
                    phys[key] = (lane & 7) ^ (4 * (wid & 1) + (lane >> 4))  # logical chunk stored at physical chunk lane & 7
    return holds, phys


def test_w_slot_every_row_is_staged_once_by_the_half_that_reads_it():
    holds, phys = staged_w_slot()
    assert sorted(holds) == list(range(BN)) and sorted(v[0] for v in holds.values()) == list(range(BN))
    assert len(phys) == BN * 8
    # fragment reads (read_w): wave column wn, half h, block j < NWh: rows WC wn + 16 NW0 h + 16 j + c16, logical chunk 4 kk + g at (4 kk + g) ^ ((c16 >> 1) & 7)
    for wn in range(4):
        for h in range(2):
            for j in range(NW1 if h else NW0):
                for c16 in range(16):
                    R = WC * wn + 16 * NW0 * h + 16 * j + c16
                    assert holds[R][1] == h, "a half tile's rows must be staged in that half's phase"
                    for kk in range(2):
                        for g in range(4):
                            assert phys[(R, (4 * kk + g) ^ ((c16 >> 1) & 7))] == 4 * kk + g


def test_a_lane_owns_sixteen_consecutive_columns_then_four():
    holds, _ = staged_w_slot()
    cover = set()
    for wn in range(4):
        for ge in range(4):
            # acc[i][j][r] of lane group ge: MMA row 4 ge + r of block j = LDS row WC wn + 16 j + 4 ge + r of the W slot
            cols = [holds[WC * wn + 16 * j + 4 * ge + r][0] for j in range(5) for r in range(4)]
            first, tail = cols[:16], cols[16:]
            nl_a = wn * WC + 0 + 16 * ge  # tile_epilogue<.., NT = 4, .., WNC = 80, COFF = 0>: nl = wn WNC + COFF + RUN g
            nl_b = wn * WC + 64 + 4 * ge  # tile_epilogue<.., NT = 1, .., WNC = 80, COFF = 64>
            assert sorted(first) == first == list(range(nl_a, nl_a + 16))
            assert tail == list(range(nl_b, nl_b + 4))
            assert (2 * nl_a) % 16 == 0 and (2 * nl_b) % 8 == 0, "bf16 runs: two 16-byte stores, then one 8-byte store"
            cover.update(cols)
    assert cover == set(range(BN))


def test_counted_waits_keep_the_three_youngest_half_tiles_in_flight():
    x_half = 2  # stage_x: two loads per thread whatever MT (MT = 4: waves 4..7 land zeros in the spare area)
    issued = []  # (K tile, part, loads) in issue order over two trips, as the phases of trip() stage them
    for t in range(0, 4, 2):
        issued += [(t + 1, "X1", x_half), (t + 2, "W0", NW0), (t + 2, "X0", x_half), (t + 2, "W1", NW1)]
        issued += [(t + 2, "X1", x_half), (t + 3, "W0", NW0), (t + 3, "X0", x_half), (t + 3, "W1", NW1)]
    vmw = NW0 + NW1 + 2
    for idx in (3, 7, 11, 15):  # the wait of phases 4 / 8: behind the stage of W1
        younger = sum(n for _, _, n in issued[idx - 2: idx + 1])
        assert younger == vmw == 7
        done_tile = issued[idx][0] - 1
        assert all(k > done_tile for k, _, _ in issued[idx - 2: idx + 1]), "everything of the tile the next phases read is older than the last three"


def test_lds_budget():
    lds = 2 * (32 * MT + BN) * 128 + 2 * (256 * 8 + 2 * BN * 4) + 4096
    assert lds == 128000 and lds <= 160 * 1024
    epi_set = 2 * 256 + 2 * BN  # floats: rowstat [256][2] | colvec [2][BN]
    assert 2 * epi_set * 4 + 4096 == lds - 2 * (32 * MT + BN) * 128


def test_colsum_of_four_columns_reaches_all_sixteen_lanes():
    """colsum16<4>: row_mirror (c ^ 15) and row_half_mirror (c ^ 7) as full exchanges, then the quad steps (c ^ 2, c ^ 1) halving: lane c ends with the
    total of column c % 4 over the 16 lanes."""
    import random

    rnd = random.Random(7)
    a = [[rnd.randint(-100, 100) for _ in range(4)] for _ in range(16)]
    cur = [row[:] for row in a]
    for x in (15, 7):
        cur = [[cur[c][e] + cur[c ^ x][e] for e in range(4)] for c in range(16)]
    for w, x in ((2, 2), (1, 1)):
        nxt = []
        for c in range(16):
            up = (c & w) != 0
            keep = [cur[c][e + w] if up else cur[c][e] for e in range(w)]
            p = c ^ x
            pup = (p & w) != 0
            send = [cur[p][e] if pup else cur[p][e + w] for e in range(w)]
            nxt.append([keep[e] + send[e] for e in range(w)] + [0] * (4 - w))
        cur = nxt
    for c in range(16):
        assert cur[c][0] == sum(a[r][c % 4] for r in range(16))


def xcd_remap(bid, nblk):
    q, r = nblk >> 3, nblk & 7
    xcd, idx = bid & 7, bid >> 3
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + idx


def plan_grid(M, N, kx, kw):  # gemm_epilogue.cuh plan_grid: tile counts and how the 8 XCDs share the tile grid
    tiles_n, tiles_m = (N + BN - 1) // BN, (M + BM - 1) // BM
    bx, bw = M * kx, N * kw
    best, pn, hm, hn = bx + 8.0 * bw, 0, 0, 0
    if 8.0 * bx + bw < best:
        best, pn = 8.0 * bx + bw, -1
    for pm in (2, 4):
        pn_ = 8 // pm
        if tiles_m % pm or tiles_n % pn_:
            continue
        cost = pn_ * bx + pm * bw
        if cost < best:
            best, pn, hm, hn = cost, pn_, tiles_m // pm, tiles_n // pn_
    return dict(tiles_m=tiles_m, tiles_n=tiles_n, pn=pn, hm=hm, hn=hn, grid0=tiles_m * tiles_n)


def tile_coords(q, bx):  # gemm8_kernel.cuh tile_coords
    if q["pn"] > 0:
        xcd, idx = bx & 7, bx >> 3
        rm, rn = divmod(xcd, q["pn"])
        lm, ln = divmod(idx, q["hn"])
        return rm * q["hm"] + lm, rn * q["hn"] + ln
    i = xcd_remap(bx, q["grid0"])
    if q["pn"] == 0:
        return divmod(i, q["tiles_n"])
    tn, tm = divmod(i, q["tiles_m"])
    return tm, tn


# (M, N, K blocks of x per row, of w per row, tiles, dispatch rounds on 256 CUs) -- conv K blocks count one tap for x (kx) and all nine for w (kw)
SHAPES = [
    (32768, 320, 2880 // 64 / 9, 2880 // 64, 256, 1),   # level-1 convolutions of a CFG pair
    (32768, 320, 8640 // 64 / 9, 8640 // 64, 256, 1),
    (32768, 640, 5760 // 64 / 9, 5760 // 64, 512, 2),
    (8192, 1280, 11520 // 64 / 9, 11520 // 64, 256, 1),
    (8192, 5120, 10, 10, 1024, 4),                      # 4096-token FF1 (shape only: GEGLU launches do not take this tile)
    (2048, 10240, 20, 20, 512, 2),                      # FF1 of a CFG pair (likewise)
]


@pytest.mark.parametrize("M,N,kx,kw,tiles,rounds", SHAPES)
def test_grid_whole_rounds_exact_cover_and_xcd_balance(M, N, kx, kw, tiles, rounds):
    q = plan_grid(M, N, kx, kw)
    assert q["grid0"] == tiles and tiles % 256 == 0 and tiles // 256 == rounds
    seen = {}
    per_xcd = [0] * 8
    for bx in range(q["grid0"]):  # one tile per workgroup: workgroup bx runs on XCD bx % 8
        tm, tn = tile_coords(q, bx)
        assert 0 <= tm < q["tiles_m"] and 0 <= tn < q["tiles_n"]
        assert (tm, tn) not in seen, "two workgroups on one tile"
        seen[(tm, tn)] = bx & 7
        per_xcd[bx & 7] += 1
    assert len(seen) == tiles and len(set(per_xcd)) == 1
    # every output element exactly once: the tiles' row / column ranges partition [0, M) x [0, N)
    rows = sorted({tm for tm, _ in seen})
    cols = sorted({tn for _, tn in seen})
    assert [r * BM for r in rows] == list(range(0, M, BM)) and [c * BN for c in cols] == list(range(0, N, BN))
    assert rows[-1] * BM + BM >= M and cols[-1] * BN + BN == N
    if q["pn"] > 0:  # rectangular regions: an XCD's tiles share hm row tiles x hn column tiles
        for x in range(8):
            mine = [k for k, v in seen.items() if v == x]
            assert len({tm for tm, _ in mine}) == q["hm"] and len({tn for _, tn in mine}) == q["hn"]


@pytest.mark.parametrize("M", [1, 127, 129, 300, 32768 + 64])
def test_partial_row_tiles_cover_every_row_once(M):
    q = plan_grid(M, 640, 10, 90)
    covered = [0] * M
    for bx in range(q["grid0"]):
        tm, tn = tile_coords(q, bx)
        if tn:
            continue
        for wm in range(2):  # the epilogue's rows: m0 + WR wm + 16 i + c16, stores suppressed at m >= M
            for i in range(MT):
                for c16 in range(16):
                    m = tm * BM + 16 * MT * wm + 16 * i + c16
                    if m < M:
                        covered[m] += 1
    assert covered == [1] * M
