// K22 -- tools/augment_data.py's ten augmentations on MI355X: one launch, one 256-thread workgroup per output image.
//
//   k_augment: the workgroup loads its source image (u8, at most 64 x 64) into an LDS plane, runs the output's program -- up to
//   SV_AUG_MAX_STEPS step records read from device memory -- ping-ponging between two LDS planes, and stores the result once.
//   Between steps the image is u8, as each of the reference's functions returns u8.  Nothing but the first load, the step records
//   and the last store touches HBM.  include/sudoku_vision_hip.h states the arithmetic of every step; the file is compiled with
//   -ffp-contract=off, so every float and double operation below is rounded on its own.
//
//   LDS (dynamic, sized by the image): two u8 planes of H*W bytes (rounded up to 16) and three f32 planes of H*W floats for the
//   elastic step (the two displacement fields and the row pass's temporary): 2*784 + 3*3136 = 10,992 bytes at 28 x 28 (14
//   workgroups fit the 160 KiB of a CU; the 32-wave cap allows 8), 57,344 bytes at 64 x 64 (2 workgroups per CU) -- below the
//   64 KiB a workgroup gets without opting in to more.
//
//   An unknown op is the identity, the step count and the source index are clamped, a rectangle is clipped, a radius or a blur
//   size outside the contract makes its step the identity, and every tap is clamped into the plane: no program can make the kernel
//   touch memory outside its buffers.  sv_augment_check_program (sv_augment_host.h) is what reports a malformed program.
#include "sv_augment_dev.h"

namespace {

__global__ __launch_bounds__(256) void k_augment(const u8 *__restrict__ src, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride,
                                                 const sv_aug_step *__restrict__ steps, const int32_t *__restrict__ n_steps, const int32_t *__restrict__ src_index,
                                                 uint64_t seed, uint64_t index_base, u8 *__restrict__ dst, int plane_bytes)
{
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ AugShared sh;
    const int tid = threadIdx.x, HW = H * W;
    const size_t o = blockIdx.x;
    u8 *plane[2] = {lds, lds + plane_bytes};
    float *fx = (float *)(lds + 2 * plane_bytes), *fy = fx + HW, *ft = fy + HW;

    const u8 *img = src + (ptrdiff_t)sv_clamp(src_index[o], 0, n_src - 1) * img_stride;
    for (int p = tid; p < HW; p += 256) {
        const int y = p / W, x = p - y * W;
        plane[0][p] = img[(ptrdiff_t)y * pitch + x];
    }
    const int ns = sv_clamp(n_steps[o], 0, SV_AUG_MAX_STEPS);
    const uint64_t g = index_base + o;
    int cur = 0;
    for (int slot = 0; slot < ns; slot++) {
        __syncthreads();                                       // the previous step's plane is complete; sh is free
        if (tid < (int)(sizeof(sv_aug_step) / 4)) ((uint32_t *)&sh.st)[tid] = ((const uint32_t *)(steps + o * SV_AUG_MAX_STEPS + slot))[tid];
        if (tid == 32) sh.sum = 0;
        __syncthreads();
        const u8 *in = plane[cur];
        u8 *out = plane[cur ^ 1];
        if (aug_run_step(sh, sh.st.op, -1, 128, in, out, H, W, fx, fy, ft, seed, g, slot, tid)) cur ^= 1;       // uniform: st is the same for every thread
    }
    __syncthreads();
    u8 *d = dst + o * (size_t)HW;
    for (int p = tid; p < HW; p += 256) d[p] = plane[cur][p];
}

}  // namespace

int svk_augment(sv_ctx *ctx, const u8 *src, int n_src, int H, int W, ptrdiff_t pitch, ptrdiff_t img_stride, const sv_aug_step *steps, const int32_t *n_steps,
                const int32_t *src_index, long n_out, uint64_t seed, long index_base, u8 *dst, hipStream_t s)
{
    (void)ctx;
    const int plane_bytes = (H * W + 15) & ~15;
    const size_t lds = 2 * (size_t)plane_bytes + 3 * sizeof(float) * (size_t)(H * W);
    hipLaunchKernelGGL(k_augment, dim3((unsigned)n_out), dim3(256), lds, s, src, n_src, H, W, pitch, img_stride, steps, n_steps, src_index, seed, (uint64_t)index_base,
                       dst, plane_bytes);
    SV_LAUNCH_CHECK("k_augment");
    return SV_OK;
}
