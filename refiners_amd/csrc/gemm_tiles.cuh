// The tile configurations of mi355x_gemm (mi355x_gemm_args.tile; the prose contract is in include/mi355x_refiners.h): ONE row per id, and the host-side rules
// that decide which row a request runs on.  Host code only -- nothing here reaches a kernel.  refiners_amd/engine/tiles.py holds the same rows for the
// Python side (tuning, autotune, dispatch report); tests/test_gemm_tiles_cpu.py reads the TILE(...) rows below from this file and compares them field by
// field, so keep one row per line, integers only.  A new tile = one row here, one row there and one kernel instance in launch_tile / launch_gemm8.
#pragma once
#include "gemm_params.cuh"

namespace mi355x {

struct Tile {
    int id;
    int loop;      // 4 = the 4-wave kernel (gemm_kernel.cuh), 8 = the 8-wave / eight-phase loop (gemm8_kernel.cuh)
    int bm, bn;    // rows x columns of an output tile
    int bm2;       // second tile height of a two-height launch (plan_mix), else 0
    int kgroups;   // K groups inside a workgroup (intra-workgroup split-K)
    int streamk;   // persistent stream-K launch: needs the caller's scratch (sk_ws / sk_flags / sk_slots)
    int f32, conv; // takes float32 launches / convolutions
    int lora;      // has in-launch LoRA instances (4-wave: two LDS stages; 8-wave: ONE column group of a plain one-segment GEMM, whole tiles)
    int trans;     // takes a transposed column group (8-wave: from a multiple of 256)
    int plain;     // plain / bias / row-bias / activation / residual / column-statistics epilogues only
    int st_lo, st_hi;  // LDS stage counts a caller may choose (0, 0: the loop's own two buffers)
    int lora_to;   // the id a LoRA launch inherits from an un-adapted shape class measured on this one (tuning.lookup; an 8-wave id only for the launches that loop's
                   // LoRA takes, else 1), and the 4-wave tile a LoRA launch asked onto this id runs on
    int fallback;  // the id a request this row refuses runs as; 0 = the library's own choice among the 4-wave tiles
};

#define TILE(id, loop, bm, bn, bm2, kgroups, streamk, f32, conv, lora, trans, plain, st_lo, st_hi, lora_to, fallback) \
    Tile { id, loop, bm, bn, bm2, kgroups, streamk, f32, conv, lora, trans, plain, st_lo, st_hi, lora_to, fallback }
//       id loop  bm   bn  bm2 kg sk f32 conv lora trans plain st    lora_to fallback
constexpr Tile TILES[] = {
    TILE(1,  4,  128, 128,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    1,      0),
    TILE(2,  4,  128,  64,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    2,      0),
    TILE(3,  4,   64, 128,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    3,      0),
    TILE(4,  4,   64,  64,   0, 1, 0,  1,  1,   1,   1,    0,  2, 4,    4,      0),
    TILE(6,  4,  128, 128,   0, 2, 0,  1,  1,   0,   1,    0,  2, 2,    1,      1),  // (8 waves of the 4-wave kernel; no statistics epilogue: with colstats it runs as 1)
    TILE(7,  8,  256, 256,   0, 1, 0,  1,  1,   1,   1,    0,  0, 0,    7,      0),
    TILE(8,  8,  256, 256,   0, 1, 1,  1,  1,   1,   1,    0,  0, 0,    7,      7),  // (with LoRA: whole tiles, i.e. 7)
    TILE(9,  8,  192, 256,   0, 1, 0,  1,  1,   1,   0,    0,  0, 0,    9,      0),
    TILE(10, 8,  128, 256,   0, 1, 0,  0,  0,   1,   0,    0,  0, 0,    7,      0),
    TILE(11, 8,  192, 256, 128, 1, 0,  0,  0,   1,   0,    0,  0, 0,    1,      9),  // (where plan_mix admits the shape and the "skg" option is 0)
    TILE(12, 8,  128, 320,   0, 1, 0,  0,  1,   0,   0,    1,  0, 0,    7,      0),
};
#undef TILE

constexpr const Tile* find_tile(int id) {
    for (const Tile& t : TILES)
        if (t.id == id) return &t;
    return nullptr;
}

extern int g_sk_g;  // probing: number of stream-K / persistent workgroups (0 = one per CU)

// Geometry of a two-height launch (tile id 11) for n_cu CUs, or false: rows [0, rb) in 192-row tiles over the first cb column tiles = a whole number of rounds, everything else in
// 128-row tiles = a whole number of rounds, each XCD with whole column tiles of every region (mix_coords).
inline bool plan_mix(int M, int N, int n_cu, int& rb, int& cb, int& nbig, int& nsmall) {
    if (M <= 0 || N <= 0 || M % 128 || N % 256 || n_cu <= 0 || n_cu % 8) return false;
    const int tn = N / 256;
    if (tn % 8) return false;
    for (rb = M / 384 * 384; rb >= 384; rb -= 384) {
        if ((M - rb) % 128) continue;
        const int rows_big = rb / 192;
        for (cb = tn / 8 * 8 - 8; cb >= 8; cb -= 8) {
            nbig = rows_big * cb;
            nsmall = (rb / 128) * (tn - cb) + ((M - rb) / 128) * tn;
            if (nbig % n_cu == 0 && nsmall % n_cu == 0) return true;
        }
    }
    return false;
}

// Can this launch run on the 8-phase loop, on tile row t?  (No split-K workspace protocol, transposed column groups from a multiple of 256; every operand below
// 2 GB: 32-bit buffer offsets with 0x80000000 as the out-of-range marker.)
inline bool gemm8_ok(const GemmP& p, bool conv, const Tile& t) {
    if (!t.trans && p.out_t) return false;
    if (t.plain && (p.lora_b || p.ln_stats || p.geglu || p.stats_out || p.out_f32)) return false;
    if (conv && !t.conv) return false;  // (float32 launches: resolve_tile, GemmP does not carry the dtype)
    if (p.ksplit > 1 || !p.vec_ok || p.N % 16) return false;  // (the epilogue instances of this loop are the vectorised ones)
    if (p.lora_b && (conv || p.lora_groups != 1 || p.nseg != 1 || p.out_t || (p.lora_r != 32 && p.lora_r != 64 && p.lora_r != 128) || !p.lora_t || !p.lora_flags || !p.lora_epoch)) return false;  // in-launch LoRA here: one column group of a plain GEMM
    if (p.out_t && p.nt_begin % 256) return false;  // a tile is either stored row-major or transposed
    for (int s = 0; s < p.nseg; ++s)
        if (p.seg[s].xbytes <= 0 || p.seg[s].wbytes <= 0 || p.seg[s].xbytes >= (1ll << 31) || p.seg[s].wbytes >= (1ll << 31)) return false;
    return true;
}

// The row of the 8-wave loop that request `req` (mi355x_set_option "tile", else mi355x_gemm_args.tile) runs on, or nullptr = the 4-wave kernel (pick_tile).
// n_cu: CUs of the device; sk_scratch: the caller brought the stream-K scratch.
inline const Tile* resolve_tile(int req, GemmP& p, bool conv, bool f32, int n_cu, bool sk_scratch) {
    const Tile* t = find_tile(req);
    if (req == 0 && !f32 && p.ksplit == 1 && p.N % 256 != 0) {
        // nobody chose: where 256-column tiles waste MFMA work (N = 320 / 640 / 960 / 1920) and 128 x 320 tiles of the 8-wave loop fill the CUs in whole rounds
        // (the level-1 convolutions of a CFG pair: 256 tiles), those -- hot 1.1-1.4x, in place -0.3 ms per step over the six classes
        const Tile* wide = find_tile(12);
        if (p.N % wide->bn == 0 && n_cu > 0 && (int64_t)((p.M + wide->bm - 1) / wide->bm) * (p.N / wide->bn) % n_cu == 0) t = wide;
    }
    // a row that does not take this kind of launch hands it to its fallback
    for (; t && t->loop == 8; t = find_tile(t->fallback)) {
        int rb, cb, nb, ns;
        if ((f32 && !t->f32) || (conv && !t->conv) || (t->streamk && !sk_scratch)) continue;
        if (t->bm2 && (g_sk_g != 0 || !plan_mix(p.M, p.N, n_cu, rb, cb, nb, ns))) continue;
        break;
    }
    if (!t || t->loop != 8) return nullptr;
    if (p.ksplit > 1) {
        // a caller that split K for want of tiles AND asks for the 8-wave loop (native._fill_split: the measured table replaced a heuristic split): the loop needs
        // no split (whole tiles or stream-K) -- take it unsplit where it can run, otherwise keep the split on the 128 x 128 tile of the 4-wave kernel
        GemmP q = p;
        q.ksplit = 1;
        q.kb_per_split = 0;
        q.partial = nullptr;
        if (gemm8_ok(q, conv, *t)) p = q;
        else p.tile_hint = 1;
    }
    return gemm8_ok(p, conv, *t) ? t : nullptr;
}

}  // namespace mi355x
