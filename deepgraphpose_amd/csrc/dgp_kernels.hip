// The launch layer of the convolution kernels (the kernels: dgp_conv_f32.hip, dgp_conv_split.hip; the TILES table: dgp_conv.h).
// plan_conv decides everything on the host -- the tile after the fall-backs, its family, and through the family's plan
// (plan_conv_split / plan_conv_f32) the path and the grid -- without a HIP call and for a given number of CUs; launch_conv launches
// what it says through the family's launcher, dgp_conv2d_plan (dgp_net.hip) reports it.
#include "dgp_conv.h"
#include <cstdlib>

namespace dgp {

// Tile choice, from scripts/conv_sweep.py on MI355X (ResNet-50 640x480 batch-32 shapes, TFLOP/s for
// 128x128 / 128x64 / 64x64): the small 64x64 tile (4 workgroups per CU, finest tail) wins for the
// K-heavy 3x3 convs and for 1x1 convs with a deep K and few output channels; 128x64 wins for the
// shallow-K, wide-N 1x1 convs (fewer re-reads of the activation rows); a 128x128 tile shared by 8 waves (same
// 16 waves per CU as the 64x64 tile, half the L2 traffic per FLOP) wins when Cout >= 512; 128x128 with 4 waves never won.
int pick_tile(int M, int CoutP, int K, bool have_absmax) {
    (void)M;
    if (CoutP <= 32) return TILE_128x32;
    if (const char* f = getenv("DGP_FORCE_TILE")) {     // tuning experiments only
        const int v = atoi(f);      // any tile of 64 or 128 columns that divides the panel and has the ranges it needs
        if (v >= 0 && v < N_TILES && TILES[v].BN >= 64 && (!TILES[v].needs_ranges || have_absmax) && CoutP % TILES[v].BN == 0) return v;
    }
    // rule 4 (default): fp16-split kernels where the caller tracks operand ranges (3 fp16 MFMAs per fp32-class
    //         product), bf16-split elsewhere;
    // rule 3 (DGP_CONV_MODE=bf16x6): bf16-split kernels (6 bf16 MFMAs per product, no range requirement);
    // rule 2 (DGP_CONV_MODE=f32): fp32 MFMA everywhere (bitwise fmaf chains)
    static const int rule = dgp_tune("DGP_TILE_RULE", 0) ? dgp_tune("DGP_TILE_RULE", 0)
                            : conv_mode() == ConvMode::F32 ? 2 : conv_mode() == ConvMode::BF16x6 ? 3 : 4;
    if (rule >= 4 && have_absmax) {
        // fp16 high/low split (3 MFMAs per product; needs the operand ranges).  With the MFMA work cut to a quarter
        // of the fp32 pipe's, the L2 -> L1 operand path sets the pace: the BK = 32 staging (a lane group fetches a
        // whole 128-byte line per pixel; BK = 16 fetches half lines) won every shape in scripts/split_sweep.py, and two
        // planes of fp16 leave room for two such workgroups per CU
        if (CoutP % 128 == 0) return TILE_128x128_H3K32;
        if (CoutP % 64 == 0) return TILE_128x64_H3;
    }
    if (rule >= 3) {
        // 128x128 / BK 16 (two workgroups per CU) won or tied on every shape with Cout % 128 == 0 in
        // scripts/split_sweep.py; Cout = 64 layers take the 128x64 tile
        if (CoutP % 128 == 0) return TILE_128x128_S6K16;
        if (CoutP % 64 == 0) return TILE_128x64_S6;
    }
    if (rule >= 2) {
        // loader-specialised 128x64 (4 compute + 4 loader waves, 3 workgroups per CU, loads two K-steps ahead) won or
        // tied on every Cin >= 32 layer except the very wide 1x1 convs, where the 8-wave 128x128 tile is ahead
        if (CoutP >= 1024) return TILE_128x128_W8;
        if (K >= 576) return TILE_128x64_LS;     // 3x3 convs and deep-K 1x1 reductions (MFMA-bound)
        // shallow-K 1x1 convs of block1/2 are HBM/L2-bound: all 256 threads loading beats 4 loader waves
        return CoutP >= 512 ? TILE_128x128_W8 : TILE_128x64;
    }
    if (rule >= 1 && CoutP >= 512 && !(K >= 4096)) return TILE_128x128_W8;   // wide-N 1x1 convs: 8 waves share a 128x128 tile
    if (K >= 1024 && CoutP <= 512) return TILE_64x64;      // 3x3 convs, deep-K 1x1 reductions
    if (K >= 576 && CoutP <= 256) return TILE_64x64;       // 3x3 convs of block1/2
    return TILE_128x64;
}

// Name of the kernel launch_conv will run for (args, tile) -- for the profile table / roofline accounting.
const char* conv_kernel_name(const ConvArgs& a, int tile_cfg) {
    if (tile_cfg >= 0 && tile_cfg < N_TILES && TILES[tile_cfg].family == FAM_SPLIT && (a.Cin >= 32 || a.stem) && a.out_mode == 0)
        return a.in_fmt == 2 && TILES[tile_cfg].name_h1 ? TILES[tile_cfg].name_h1 : TILES[tile_cfg].name;
    return "f32";
}

// 16-bit tier: ConvArgs describe the layer in REAL channels and fp32-sized byte extents; the cell kernels address the H1 input in 4-byte
// units (two halves each), so every quantity the loaders use is halved here, once: channels per pixel, K-steps, panel rows per tap,
// second-source split, byte extents.  The GEMM's columns (Cout, CoutP) are not touched: the O1 epilogue halves its own byte offsets.
static bool to_h1_units(ConvArgs& a) {
    if ((a.Cin & 63) || (a.in2 && (a.cin_split & 63)) || (a.nk & 1) || a.up || a.stem || !a.wh3) return false;
    a.Cin >>= 1; a.cin_split >>= 1; a.nk >>= 1; a.tap_rows >>= 1;
    a.log2cin4 = ilog2(a.Cin / 4);
    a.in_bytes >>= 1; a.in2_bytes >>= 1; a.w_bytes >>= 1; a.wh3_bytes >>= 1;
    if (a.out_fmt == 2) a.out_bytes >>= 1;
    if (a.res && a.res_fmt == 2) a.res_bytes >>= 1;
    return true;
}

hipError_t plan_conv(ConvArgs& a, int tile_cfg, int n_cu, ConvPlan& pl) {
    pl = ConvPlan{};
    pl.wide = true;
    if (a.in_fmt == 2 && !(a.out_mode == 0 && to_h1_units(a))) return hipErrorInvalidValue;
    if (a.in_fmt != 2 && (a.out_fmt == 2 || a.res_fmt == 2)) return hipErrorInvalidValue;
    const bool known = tile_cfg >= 0 && tile_cfg < N_TILES;
    if (a.Cin < 32 && !a.stem) {       // generic per-lane tap path (stem / small test shapes)
        const int small = known ? TILES[tile_cfg].small_tile : TILE_128x64;
        pl.tile = small == TILE_128x32 ? TILE_128x32 : (small == TILE_128x128 && a.CoutP % 128 == 0) ? TILE_128x128 : TILE_128x64;
        pl.family = FAM_F32; pl.wide = false;
    } else {
        if (!known) tile_cfg = TILE_128x128;
        if (a.out_mode != 0) tile_cfg = TILES[tile_cfg].f32_tile;      // (the transposed-conv scatter exists in the fp32 kernels only)
        pl.tile = tile_cfg; pl.family = TILES[tile_cfg].family;
    }
    const hipError_t e = pl.family == FAM_SPLIT ? plan_conv_split(a, n_cu, pl) : plan_conv_f32(a, pl);
    pl.mtiles = a.mtiles; pl.ntiles = a.ntiles;
    pl.tail_ksplit = a.tail_ksplit; pl.n_main = a.n_main; pl.st_gn = a.st_gn; pl.st_mc = a.st_mc; pl.st_mb = a.st_mb;
    return e;
}

hipError_t launch_conv(const ConvArgs& a_in, int tile_cfg, hipStream_t s) {
    ConvArgs a = a_in;
    ConvPlan pl;
    hipError_t e = plan_conv(a, tile_cfg, device_facts().n_cu, pl);
    if (e != hipSuccess) return e;
    return pl.family == FAM_SPLIT ? launch_conv_split(a, pl, s) : launch_conv_f32(a, pl, s);
}

}  // namespace dgp
