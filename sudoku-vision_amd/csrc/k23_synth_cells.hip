// K23 -- ml/generate_synthetic_v2.py's digit cells on MI355X: one launch, one 256-thread workgroup per output cell.
//
//   k_synth_cells, phase A: every thread computes its pixels of the base image from the output's cell record (background, paper grain,
//   grid-line artefacts, smudge, glyph blend: sv_syn_base_pixel in sv_synth_host.h, the text a host compiler also compiles) straight into
//   an LDS plane.  A pixel depends on no other, so the phase has no barrier of its own.  Phase B runs the output's step program on that
//   plane, ping-ponging between two LDS planes as K22 does: K22's eleven step bodies (sv_augment_dev.h, the one text both kernels
//   include) and the generator's own ops -- the two warps with a constant border, the scale with a pad value, the Q8.8 Gaussian blur
//   and the 2 x 2 erode / dilate.  The cell is stored once; nothing but the cell and step records, the glyph atlas (a few KiB, in L2
//   after the first workgroups) and that store touches HBM.  include/sudoku_vision_hip.h states the arithmetic; the file is compiled
//   with -ffp-contract=off, and the double arithmetic of the backgrounds and the warp coordinates is part of the result.
//
//   LDS (dynamic, sized by the cell) as in K22: two u8 planes of size*size bytes (rounded up to 16) and, because K22's elastic step
//   stays reachable through phase B, its three f32 planes: 2*784 + 3*3136 = 10,992 bytes at 28 x 28 (14 workgroups fit the 160 KiB
//   of a CU; the 32-wave cap allows 8), 57,344 bytes at 64 x 64 (2 workgroups per CU) -- below the 64 KiB a workgroup gets without
//   opting in to more.
//
//   An atlas slot out of range draws nothing, a mask's sides are clamped to the slot, offsets, rectangles, widths, strides, taps and
//   counts are clamped or clipped, an unknown op is the identity: no record can make the kernel touch memory outside its buffers.
//   sv_synth_check_program (sv_synth_host.h) is what reports a malformed job.
#include "sv_augment_dev.h"
#include "sv_synth_host.h"

namespace {

__global__ __launch_bounds__(256) void k_synth_cells(const sv_syn_cell *__restrict__ cells, const sv_aug_step *__restrict__ steps, const int32_t *__restrict__ n_steps,
                                                     int size, const u8 *__restrict__ atlas, const int32_t *__restrict__ dims, int n_slots, uint64_t seed,
                                                     uint64_t index_base, u8 *dst, int plane_bytes)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ AugShared sh;
    __shared__ sv_syn_cell cell;
    const int tid = threadIdx.x, H = size, W = size, HW = size * size;
    const size_t o = blockIdx.x;
    u8 *plane[2] = {lds, lds + plane_bytes};
    float *fx = (float *)(lds + 2 * plane_bytes), *fy = fx + HW, *ft = fy + HW;
    const uint64_t g = index_base + o;

    u8 *d = dst + o * (size_t)HW;
    if (tid < (int)(sizeof(sv_syn_cell) / 4)) ((uint32_t *)&cell)[tid] = ((const uint32_t *)(cells + o))[tid];
    __syncthreads();
    for (int p = tid; p < HW; p += 256) {
        const int y = p / W, x = p - y * W;
        plane[0][p] = sv_syn_base_pixel(cell, size, x, y, seed, g, atlas, dims, n_slots, d);
    }

    const int ns = sv_clamp(n_steps[o], 0, SV_AUG_MAX_STEPS);
    int cur = 0;
    for (int slot = 0; slot < ns; slot++) {
        __syncthreads();                                       // the previous plane is complete; sh is free
        if (tid < (int)(sizeof(sv_aug_step) / 4)) ((uint32_t *)&sh.st)[tid] = ((const uint32_t *)(steps + o * SV_AUG_MAX_STEPS + slot))[tid];
        if (tid == 32) sh.sum = 0;
        __syncthreads();
        const sv_aug_step &st = sh.st;
        const u8 *in = plane[cur];
        u8 *out = plane[cur ^ 1];
        bool wrote = true;
        switch (st.op) {
        case SV_SYN_AFFINE_CONST: wrote = aug_run_step(sh, SV_AUG_AFFINE, sv_clamp(st.i[0], 0, 255), 128, in, out, H, W, fx, fy, ft, seed, g, slot, tid); break;
        case SV_SYN_PERSPECTIVE_CONST: wrote = aug_run_step(sh, SV_AUG_PERSPECTIVE, sv_clamp(st.i[0], 0, 255), 128, in, out, H, W, fx, fy, ft, seed, g, slot, tid); break;
        case SV_SYN_SCALE_PAD: wrote = aug_run_step(sh, SV_AUG_SCALE, -1, sv_clamp(st.i[3], 0, 255), in, out, H, W, fx, fy, ft, seed, g, slot, tid); break;
        case SV_SYN_GAUSS_BLUR: {
            const int k = st.i[0];
            if (k != 3 && k != 5) { wrote = false; break; }
            for (int p = tid; p < HW; p += 256) {
                const int y = p / W, x = p - y * W;
                out[p] = sv_syn_blur_px(in, H, W, x, y, k, st.i + 1);
            }
            break;
        }
        case SV_SYN_ERODE: case SV_SYN_DILATE:
            for (int p = tid; p < HW; p += 256) {
                const int y = p / W, x = p - y * W;
                out[p] = sv_syn_morph_px(in, H, W, x, y, st.op == SV_SYN_DILATE);
            }
            break;
        default: wrote = aug_run_step(sh, st.op, -1, 128, in, out, H, W, fx, fy, ft, seed, g, slot, tid); break;      // K22's ops; anything else: the identity
        }
        if (wrote) cur ^= 1;                                   // uniform: st is the same for every thread
    }
    __syncthreads();
    for (int p = tid; p < HW; p += 256) d[p] = plane[cur][p];
}

}  // namespace

int svk_synth_cells(sv_ctx *ctx, const sv_syn_cell *cells, const sv_aug_step *steps, const int32_t *n_steps, long n_out, int size, const u8 *atlas, const int32_t *dims,
                    int n_slots, uint64_t seed, long index_base, u8 *dst, hipStream_t s)
{
    (void)ctx;
    const int plane_bytes = (size * size + 15) & ~15;
    const size_t lds = 2 * (size_t)plane_bytes + 3 * sizeof(float) * (size_t)(size * size);
    hipLaunchKernelGGL(k_synth_cells, dim3((unsigned)n_out), dim3(256), lds, s, cells, steps, n_steps, size, atlas, dims, n_slots, seed, (uint64_t)index_base, dst,
                       plane_bytes);
    SV_LAUNCH_CHECK("k_synth_cells");
    return SV_OK;
}
