// What the five fc heads of DigitCNN share on the device (k_fc_head in k3_cnn.hip, k_fc_head_h2 / _h2p in k3_cnn_h2.hip, k_fc_head_bf16 /
// _bf16p in k3_cnn_bf16.hip): the tail that turns fc1 accumulators into logits, digit and confidence, the lane/tile prologue of the
// wave-tile heads, and the whole body of the two per-CU heads, of which a precision supplies only its sizes and its MFMA loop.
#pragma once
#include "sv_cnn_dev.h"
#include "sv_internal.h"

namespace {

constexpr int SV_FC_HS_LD = 129;          // leading dimension of a tile of hidden activations: 128 + 1 float of bank skew

// Lane (r, q) of a wave that owns the 16-cell M tile starting at cell0: MFMA row/column r, k-group / accumulator row group q; crow is the
// cell whose features the lane reads as row r (rows past the end of the batch read the last cell: a valid address, results dropped).
struct sv_fc_lane { int r, q; long cell0, crow; };

// the wave-tile heads: 64 cells per 256-thread workgroup, one M tile per wave
__device__ __forceinline__ sv_fc_lane sv_fc_wave_tile(int lane, int wave, long B)
{
    sv_fc_lane l;
    l.r = lane & 15;
    l.q = lane >> 4;
    l.cell0 = (long)blockIdx.x * 64 + wave * 16;
    l.crow = l.cell0 + l.r;
    if (l.crow >= B) l.crow = B - 1;
    return l;
}

// The tail of every fc head, for a wave that holds NT N tiles (hidden units n0 .. n0 + 16 NT - 1) of the M tile of cells cell0 .. cell0 + 15:
// hidden(t, reg) is the pre-bias fc1 sum of cell row 4q + reg, hidden unit n0 + 16 t + r.  Bias and ReLU into the tile's hs; then, in the
// waves with fc2_wave set (one per M tile), fc2 with lane (cell r, class group q) computing classes q, q + 4, q + 8, and digit and
// confidence of the cells below c_end.  Every wave of the workgroup must call it: it holds two workgroup barriers.
template <int NT, class Hidden>
__device__ __forceinline__ void sv_fc_tail(float (*hs)[SV_FC_HS_LD], int n0, Hidden hidden, const float *b1, const float (*w2s)[128], const float *b2,
                                           float (*lg)[12], long cell0, long c_end, bool fc2_wave, float *logits, u8 *digits, float *conf)
{
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const float bias = b1[n0 + 16 * t + r];
#pragma unroll
        for (int reg = 0; reg < 4; reg++) hs[4 * q + reg][n0 + 16 * t + r] = fmaxf(hidden(t, reg) + bias, 0.f);
    }
    __syncthreads();
    if (fc2_wave) {
        // Unrolled, with a compiler-only memory barrier per class, so that each class re-reads the cell's hidden activations from the LDS.
        // Without the barrier the compiler keeps all 128 in registers across the classes (k_fc_head: 288 VGPRs, one wave per SIMD instead of
        // three; k_fc_head_h2 spills); rolled, every head measured 1 us slower per launch.
#pragma unroll
        for (int jj = 0; jj < 3; jj++) {
            const int j = q + 4 * jj;
            if (j < 10) {
                const float s = sv_fc2_logit(hs[r], w2s, b2, j);
                lg[r][j] = s;
                if (cell0 + r < c_end) logits[(cell0 + r) * 10 + j] = s;
            }
            asm volatile("" ::: "memory");
        }
    }
    __syncthreads();
    if (fc2_wave && q == 0 && cell0 + r < c_end) sv_digit_conf(lg[r], cell0 + r, digits, conf);
}

// one LDS-DMA piece: 64 lanes x 16 B from the lanes' own addresses to lds_dst + 16 * lane (M0 carries the LDS byte address; saved and restored)
__device__ __forceinline__ void sv_glds16(const void *gsrc, unsigned lds_dst)
{
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// ---------------------------------------------------------------------------------------------------------------------
// The per-CU fc head (k_fc_head_h2p, k_fc_head_bf16p): one 768-thread workgroup per CU that streams the fc1 weight image ONCE for all of
// its cells (the wave-tile heads stream it once per 64 cells: 324 times for 256 frames, 0.52 GB of f16 pairs through the L2s).
// 12 waves = 6 M tiles (96 cells, one pass) x 2 N halves; 3 waves per SIMD.  K = 3136 in 49 stages of 64.
// What bounds an fc kernel of this shape is not the MFMA pipe (a quarter busy), the LDS or the L2s but the texture addresser:
// a wave-load of MFMA A fragments straight from the features touches 64 different 16-byte pieces in 32 lines and takes the
// TA ~55 cycles, and the waves queue up behind it in program order (tools/ubench_fc_read.hip: 62 us for the 260 MB read that
// way, 40 us with 16 adjacent lanes reading 256 contiguous bytes).  So BOTH operands go global -> LDS directly
// (global_load_lds_dwordx4, inline asm: hipcc would guard every ds_read after one with vmcnt(0)), in pieces of 1 KB (sv_glds16):
//   * weights: a stage of Fmt::W_STAGE bytes, W_PIECES pieces from each of waves 0-7 (the loaders), ring of two stages, one in flight
//     (L2 hits);
//   * features: A_ROW_B bytes of each of the 96 rows per stage; a piece is 1024 / A_ROW_B rows with lane-contiguous sources, A_PIECES
//     pieces per wave, ring of three stages, two in flight (HBM).  The image is row-major, [96 rows][A_ROW_B / 16 units of 16 B]; unit u
//     of row r sits in slot u ^ Fmt::swz(r) -- the DMA cannot scatter, so the permutation is on the source address -- which makes the 16
//     lanes of every ds_read_b128 lane group of an A-fragment fetch hit 16 different bank slots.
// One counted wait and one raw barrier per stage: at the top of stage s a wave waits until only its A_PIECES feature pieces of stage
// s + 1 are in flight (s_waitcnt vmcnt(A_PIECES): its weight pieces of stage s, issued after the features of s and before those of
// s + 1, have landed), the barrier makes everybody's pieces visible and frees the slots that stage s - 1 read, and the pieces of weight
// stage s + 1 and feature stage s + 2 are issued into them.  After the K loop the hidden activations alias the rings.
//
// Fmt, the precision's policy (defined next to its kernel), carries what differs:
//   A_ROW_B, A_PIECES, W_STAGE, ROW_HBM_B (bytes of a feature row in HBM), NA (A fragments of a lane per stage);
//   swz(row): the row's slot permutation;  a_unit(q, c): the unit of the lane's c-th A fragment;
//   its accumulators, compute(wt, at, a_off, nh): the stage's MFMAs from weight stage wt (+ 16 lane) and feature stage at, and
//   hidden(t, reg): the pre-bias fc1 sum for sv_fc_tail.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int SV_FCP_WAVES = 12, SV_FCP_MT = SV_FC_PERCU_CELLS / 16, SV_FCP_NSTAGE = FEAT / 64;

template <class Fmt>
__device__ __forceinline__ void sv_fc_head_percu(Fmt &f, const void *feat, long B, long per, const uint4 *w1img, const float *b1, const float *w2,
                                                 const float *b2, float *logits, u8 *digits, float *conf)
{
    // one LDS object: [2 weight stages][3 feature stages] (the hidden activations alias them after the K loop) [w2][logits]
    constexpr int CELLS = SV_FC_PERCU_CELLS, W_STAGE = Fmt::W_STAGE, W_PIECES = W_STAGE / 8 / 1024, A_ROW_B = Fmt::A_ROW_B, A_UNITS = A_ROW_B / 16;
    constexpr int A_STAGE = CELLS * A_ROW_B, OFF_A = 2 * W_STAGE, RINGS = OFF_A + 3 * A_STAGE, HS_B = CELLS * SV_FC_HS_LD * 4;
    constexpr int OFF_W2 = RINGS > HS_B ? RINGS : HS_B, OFF_LG = OFF_W2 + 10 * 128 * 4, LDS_B = OFF_LG + SV_FCP_MT * 16 * 12 * 4;
    static_assert(SV_FCP_WAVES == 2 * SV_FCP_MT && W_PIECES * 8 * 1024 == W_STAGE, "waves 0-7 load a weight stage in whole pieces");
    static_assert(Fmt::A_PIECES * SV_FCP_WAVES * 1024 == A_STAGE && Fmt::NA * 4 == A_UNITS, "every wave loads A_PIECES pieces of a feature stage");
    static_assert(OFF_W2 % 16 == 0 && LDS_B <= 160 * 1024, "the rings, or the hidden activations over them, and the fc2 tail fit the CU's LDS");
    __shared__ __attribute__((aligned(16))) unsigned char lds[LDS_B];
    float(*hs)[SV_FC_HS_LD] = (float(*)[SV_FC_HS_LD])lds;                              // [96][129] floats = 49.5 KB
    float(*w2s)[128] = (float(*)[128])(lds + OFF_W2);
    float(*lg)[16][12] = (float(*)[16][12])(lds + OFF_LG);
    const unsigned lds_base = (unsigned)(unsigned long long)(__attribute__((address_space(3))) unsigned char *)lds;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int mt = wave % SV_FCP_MT, nh = wave / SV_FCP_MT;                            // M tile, N half (hidden units 64 nh ..)
    const bool loader = wave < 8;
    sv_fc2_stage<64 * SV_FCP_WAVES>(w2s, w2, tid);

    // this lane's A fragments in a feature stage: row 16 mt + r, fragment c = unit a_unit(q, c), in slot unit ^ swz(row)
    unsigned a_off[Fmt::NA];
#pragma unroll
    for (int c = 0; c < Fmt::NA; c++) a_off[c] = OFF_A + (16 * mt + r) * A_ROW_B + (Fmt::a_unit(q, c) ^ Fmt::swz(r)) * 16;

    const long base = (long)blockIdx.x * per, c_end = base + per < B ? base + per : B;     // per <= 96: one pass (sv_fc_percu_share)
    const long cell0 = base + 16 * mt;
    const bool tile_live = cell0 < c_end;                                              // (wave-uniform) an M tile with no cell does no arithmetic
    // this lane's share of the wave's feature pieces: piece i = rows (A_PIECES wave + i) (1024 / A_ROW_B) .. of the pass, this lane's row
    // of it lane / A_UNITS, slot lane % A_UNITS -> unit slot ^ swz(row)
    const unsigned char *asrc[Fmt::A_PIECES];
#pragma unroll
    for (int i = 0; i < Fmt::A_PIECES; i++) {
        const int rl = (Fmt::A_PIECES * wave + i) * (1024 / A_ROW_B) + lane / A_UNITS;
        long row = base + rl;
        if (row >= c_end) row = c_end - 1;                                             // rows past the end: a valid address, results dropped
        asrc[i] = (const unsigned char *)feat + row * Fmt::ROW_HBM_B + (((unsigned)(lane % A_UNITS)) ^ Fmt::swz(rl)) * 16;
    }
    const uint4 *wp = w1img + (wave & 7) * W_PIECES * 64 + lane;                        // this wave's pieces of a weight stage
    auto issue_w = [&](int st) {
        if (loader) {
            const unsigned dst = lds_base + (st & 1) * W_STAGE + (wave & 7) * W_PIECES * 1024;
#pragma unroll
            for (int j = 0; j < W_PIECES; j++) sv_glds16(wp + (long)st * (W_STAGE / 16) + 64 * j, dst + 1024 * j);
        }
    };
    auto issue_a = [&](int st) {
        const unsigned dst = lds_base + OFF_A + (st % 3) * A_STAGE + Fmt::A_PIECES * wave * 1024;
#pragma unroll
        for (int i = 0; i < Fmt::A_PIECES; i++) sv_glds16(asrc[i] + A_ROW_B * st, dst + 1024 * i);
    };
    f.zero();
    issue_w(0);
    issue_a(0);
    issue_a(1);
    for (int st = 0; st < SV_FCP_NSTAGE; st++) {
        // only this wave's feature pieces of stage st + 1 stay in flight: its weight pieces of stage st were issued before them
        if (st + 1 < SV_FCP_NSTAGE) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(Fmt::A_PIECES) : "memory"); else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        if (st + 1 < SV_FCP_NSTAGE) issue_w(st + 1);
        if (st + 2 < SV_FCP_NSTAGE) issue_a(st + 2);
        if (tile_live) f.compute(lds + (st & 1) * W_STAGE + lane * 16, lds + (st % 3) * A_STAGE, a_off, nh);
    }
    __syncthreads();                                                                    // everybody is done reading the rings: hs may overwrite them

    sv_fc_tail<4>(hs + 16 * mt, 64 * nh, [=](int t, int reg) { return f.hidden(t, reg); }, b1, w2s, b2, lg[mt], cell0, c_end, nh == 0, logits, digits, conf);
}

}  // namespace
