// K21: model evaluation metrics (include/sudoku_vision_hip.h, sv_eval_metrics): what the reference's ml/evaluate_v2.py:67-220 and
// ml/train.py:157-190 do on the host after copying every logit there -- softmax, argmax, confusion counts, reliability bins, the list of
// misclassified cells -- in one pass over the logits.
//
//   k_eval_clear     zeroes the stats block (a launch, not a memset: DESIGN.md "Stream order and graph replay")
//   k_eval_cells     tiles of EV_TILE cells, a thread per cell; at most EV_MAX_WGS workgroups, each taking every gridDim.x-th tile: per-cell
//                    outputs, aggregates in LDS over all its tiles, then one integer atomic per non-zero aggregate and workgroup.  With a
//                    failure list: the cell's wrong flag and the tile's count of them go to the scratch.
//   k_eval_scan      one workgroup: exclusive prefix sum over the tiles' wrong counts, in place; the list's base
//   k_eval_failures  one workgroup per tile: prefix sum over its wrong flags, and the records whose place is below max_failures (the
//                    tiles past the list's end leave at once).  A record's cell is evaluated again from its ten inputs.
//
// Scratch (ctx->eval, only with a failure list): u64 list base | u32 wrong count, then offset, per tile | u8 wrong flag per cell.
//
// The softmax is k_softmax_topk's (k3_cnn.hip) restated, not shared through a header: that kernel's translation unit is left as it is.
// Same operations in the same order under the same flags (-ffp-contract=off, the same expf), so the probabilities are bit-identical;
// tests/test_gpu_eval.py asserts it.
#include "sv_internal.h"

namespace {

constexpr int EV_TILE = 256, EV_MAX_WGS = 1024;
typedef unsigned long long u64;

struct EvalEdges { double b[SV_EVAL_MAX_BINS + 1]; };

struct EvalCell {
    float p[10];        // softmax mode: expf(z - m), not yet divided; probability mode: the input
    float den;          // 1 in probability mode
    float zl;           // softmax mode: z[label] - m (0 for a bad label)
    int pred, label;    // label -1: outside 0..9
    bool finite;
};

template <bool PROB>
__device__ __forceinline__ void eval_cell(const float *__restrict__ in, const void *__restrict__ labels, bool i64, long cell, float T, EvalCell &c)
{
    float l[10];
    c.finite = true;
#pragma unroll
    for (int j = 0; j < 10; j++) { l[j] = in[cell * 10 + j]; c.finite = c.finite && isfinite(l[j]); }
    float top = l[0];
    c.pred = 0;
#pragma unroll
    for (int j = 1; j < 10; j++)
        if (l[j] > top) { top = l[j]; c.pred = j; }
    if (!c.finite) {                                        // rare: a NaN is the maximum, the first one (np.argmax, torch.argmax)
#pragma unroll
        for (int j = 9; j >= 0; j--)
            if (l[j] != l[j]) { top = l[j]; c.pred = j; }
    }
    const long label = i64 ? (long)((const long long *)labels)[cell] : (long)((const int *)labels)[cell];
    c.label = label >= 0 && label < 10 ? (int)label : -1;
    c.zl = 0.f;
    if (PROB) {
#pragma unroll
        for (int j = 0; j < 10; j++) c.p[j] = l[j];
        c.den = 1.f;
        c.finite = c.finite && top >= 0.f && top <= 1.f;
        return;
    }
    float best = -INFINITY;
#pragma unroll
    for (int j = 0; j < 10; j++) { c.p[j] = T == 1.f ? l[j] : l[j] / T; best = fmaxf(best, c.p[j]); }
    float den = 0.f;
#pragma unroll
    for (int j = 0; j < 10; j++) {
        const float d = c.p[j] - best;
        if (j == c.label) c.zl = d;
        c.p[j] = expf(d);
        den += c.p[j];
    }
    c.den = den;
}

// p[j] without a dynamically indexed register array
__device__ __forceinline__ float pick10(const float (&p)[10], int j)
{
    float v = p[0];
#pragma unroll
    for (int i = 1; i < 10; i++) v = i == j ? p[i] : v;
    return v;
}

struct EvalLds {
    unsigned confusion[100];
    unsigned bin_count[SV_EVAL_MAX_BINS], bin_correct[SV_EVAL_MAX_BINS];
    u64 bin_conf[SV_EVAL_MAX_BINS];
    unsigned valid, correct, bad_labels, nonfinite;
    u64 conf_all, conf_correct;
    double edges[SV_EVAL_MAX_BINS + 1];
};

__device__ __forceinline__ void flush(uint64_t *dst, u64 v)
{
    if (v) atomicAdd((u64 *)dst, v);
}

__global__ __launch_bounds__(256) void k_eval_clear(uint64_t *stats)
{
    for (unsigned i = threadIdx.x; i < sizeof(sv_eval_stats) / 8; i += 256) stats[i] = 0;
}

template <bool PROB>
__global__ __launch_bounds__(EV_TILE) void k_eval_cells(const float *__restrict__ in, const void *__restrict__ labels, int i64, long B, long ntiles, float T,
                                                        EvalEdges edges, int n_bins, float *__restrict__ probs, u8 *__restrict__ pred, float *__restrict__ conf,
                                                        float *__restrict__ true_prob, float *__restrict__ nll, u8 *__restrict__ correct,
                                                        sv_eval_stats *__restrict__ stats, unsigned *__restrict__ tile_wrong, u8 *__restrict__ wrong_flag)
{
    __shared__ EvalLds s;
    const int tid = threadIdx.x;
    for (int i = tid; i < 100; i += EV_TILE) s.confusion[i] = 0;
    if (tid < SV_EVAL_MAX_BINS) { s.bin_count[tid] = 0; s.bin_correct[tid] = 0; s.bin_conf[tid] = 0; }
    if (tid <= n_bins) s.edges[tid] = edges.b[tid];
    if (tid == 0) { s.valid = s.correct = s.bad_labels = s.nonfinite = 0; s.conf_all = s.conf_correct = 0; }
    __syncthreads();

    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {          // uniform over the workgroup
        const long cell = tile * EV_TILE + tid;
        bool wrong = false;
        if (cell < B) {
            EvalCell c;
            eval_cell<PROB>(in, labels, i64 != 0, cell, T, c);
            const float cf = pick10(c.p, c.pred) / c.den;
            const bool valid = c.finite && c.label >= 0, ok = valid && c.pred == c.label;
            wrong = valid && !ok;
            if (probs) {
#pragma unroll
                for (int j = 0; j < 10; j++) probs[cell * 10 + j] = c.p[j] / c.den;
            }
            if (pred) pred[cell] = (u8)c.pred;
            if (conf) conf[cell] = cf;
            if (true_prob || nll) {
                const float tp = c.label >= 0 ? pick10(c.p, c.label) / c.den : NAN;
                if (true_prob) true_prob[cell] = tp;
                if (nll) nll[cell] = c.label < 0 ? NAN : PROB ? -logf(tp) : logf(c.den) - c.zl;
            }
            if (correct) correct[cell] = (u8)ok;
            if (wrong_flag) wrong_flag[cell] = (u8)wrong;
            if (!c.finite) atomicAdd(&s.nonfinite, 1u);
            else if (c.label < 0) atomicAdd(&s.bad_labels, 1u);
            else {
                const u64 fx = (u64)(cf * 1073741824.f);
                atomicAdd(&s.confusion[c.label * 10 + c.pred], 1u);
                atomicAdd(&s.valid, 1u);
                atomicAdd(&s.conf_all, fx);
                if (ok) { atomicAdd(&s.correct, 1u); atomicAdd(&s.conf_correct, fx); }
                // the first edge that is >= conf: edges[k - 1] < conf <= edges[k], bin k - 1 when there is one (ml/evaluate_v2.py:163)
                const double cd = (double)cf;
                int lo = 0, hi = n_bins + 1;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (s.edges[mid] >= cd) hi = mid; else lo = mid + 1;
                }
                if (lo >= 1 && lo <= n_bins) {
                    atomicAdd(&s.bin_count[lo - 1], 1u);
                    atomicAdd(&s.bin_conf[lo - 1], fx);
                    if (ok) atomicAdd(&s.bin_correct[lo - 1], 1u);
                }
            }
        }
        if (tile_wrong) {                                                      // uniform: every thread of the workgroup is here
            const int n = __syncthreads_count(wrong);
            if (tid == 0) tile_wrong[tile] = (unsigned)n;
        }
    }
    __syncthreads();

    for (int i = tid; i < 100; i += EV_TILE) flush(&stats->confusion[i / 10][i % 10], s.confusion[i]);
    if (tid < n_bins) {
        flush(&stats->bin_count[tid], s.bin_count[tid]);
        flush(&stats->bin_correct[tid], s.bin_correct[tid]);
        flush(&stats->bin_conf[tid], s.bin_conf[tid]);
    }
    if (tid == EV_TILE - 1) {
        const u64 n = s.valid, good = s.correct, bad = n - good;
        flush(&stats->n, n);
        flush(&stats->n_correct, good);
        flush(&stats->n_wrong, bad);
        flush(&stats->bad_labels, s.bad_labels);
        flush(&stats->nonfinite, s.nonfinite);
        flush(&stats->tot_count[0], n);
        flush(&stats->tot_count[1], good);
        flush(&stats->tot_count[2], bad);
        flush(&stats->tot_correct[0], good);
        flush(&stats->tot_correct[1], good);
        flush(&stats->tot_conf[0], s.conf_all);
        flush(&stats->tot_conf[1], s.conf_correct);
        flush(&stats->tot_conf[2], s.conf_all - s.conf_correct);
    }
}

// exclusive prefix sum of v over the 256 threads of the workgroup (sh: 256 entries); total: the sum over all of them
__device__ __forceinline__ unsigned scan256(unsigned v, unsigned *sh, unsigned &total)
{
    const int tid = threadIdx.x;
    sh[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const unsigned add = tid >= d ? sh[tid - d] : 0;
        __syncthreads();
        sh[tid] += add;
        __syncthreads();
    }
    const unsigned incl = sh[tid];
    total = sh[255];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(256) void k_eval_scan(unsigned *__restrict__ tile_wrong, long ntiles, const sv_eval_stats *__restrict__ stats, u64 *__restrict__ list_base)
{
    __shared__ unsigned sh[256];
    unsigned running = 0;                                   // the wrong cells of one call: at most B < 2^32
    for (long at = 0; at < ntiles; at += 256) {
        const long i = at + threadIdx.x;
        const unsigned v = i < ntiles ? tile_wrong[i] : 0;
        unsigned total;
        const unsigned excl = scan256(v, sh, total);
        if (i < ntiles) tile_wrong[i] = running + excl;
        running += total;
    }
    // k_eval_cells has added this call's wrong cells to n_wrong already: the list goes on where the calls before it stopped
    if (threadIdx.x == 0) *list_base = stats->n_wrong - running;
}

template <bool PROB>
__global__ __launch_bounds__(EV_TILE) void k_eval_failures(const float *__restrict__ in, const void *__restrict__ labels, int i64, long B, long index_base, float T,
                                                           const unsigned *__restrict__ tile_offset, const u8 *__restrict__ wrong_flag,
                                                           const u64 *__restrict__ list_base, sv_eval_failure *__restrict__ failures, long max_failures)
{
    __shared__ unsigned sh[256];
    const u64 base = *list_base + tile_offset[blockIdx.x];
    if (base >= (u64)max_failures) return;                  // uniform over the workgroup: before any barrier
    const long cell = (long)blockIdx.x * EV_TILE + threadIdx.x;
    const bool wrong = cell < B && wrong_flag[cell];
    unsigned total;
    const u64 place = base + scan256(wrong ? 1u : 0u, sh, total);
    if (!wrong || place >= (u64)max_failures) return;
    EvalCell c;
    eval_cell<PROB>(in, labels, i64 != 0, cell, T, c);    // a wrong cell is valid: its label is 0..9
    sv_eval_failure f;
    f.index = index_base + cell;
    f.label = c.label;
    f.pred = c.pred;
    f.conf = pick10(c.p, c.pred) / c.den;
    f.true_prob = pick10(c.p, c.label) / c.den;
    unsigned taken = 0;                                     // k_softmax_topk's selection: from the lowest untaken class, only to a strictly greater one
    for (int q = 0; q < 3; q++) {
        float top = -1.f;
        int arg = -1;
#pragma unroll
        for (int j = 0; j < 10; j++)
            if (!(taken >> j & 1) && (arg < 0 || c.p[j] > top)) { top = c.p[j]; arg = j; }
        taken |= 1u << arg;
        f.top3_index[q] = arg;
        f.top3_prob[q] = top / c.den;
    }
    failures[place] = f;
}

size_t scratch_bytes(long B, long ntiles) { return 8 + ((size_t)ntiles * 4 + 7) / 8 * 8 + (size_t)B; }

}  // namespace

int svk_eval_metrics(sv_ctx *ctx, const float *input, bool prob, const void *labels, bool i64, long B, long index_base, float T, const double *bin_edges, int n_bins,
                     bool accumulate, float *probs, u8 *pred, float *conf, float *true_prob, float *nll, u8 *correct, sv_eval_stats *stats,
                     sv_eval_failure *failures, long max_failures, hipStream_t s)
{
    if (!accumulate) {
        hipLaunchKernelGGL(k_eval_clear, dim3(1), dim3(256), 0, s, (uint64_t *)stats);
        SV_LAUNCH_CHECK("k_eval_clear");
    }
    if (B == 0) return SV_OK;
    EvalEdges edges = {};
    for (int i = 0; i <= n_bins; i++) edges.b[i] = bin_edges[i];
    const long ntiles = (B + EV_TILE - 1) / EV_TILE;
    const unsigned grid = (unsigned)(ntiles < EV_MAX_WGS ? ntiles : EV_MAX_WGS);
    u64 *list_base = nullptr;
    unsigned *tile_wrong = nullptr;
    u8 *wrong_flag = nullptr;
    if (max_failures > 0) {
        const int rc = ctx->eval.grow(ctx, scratch_bytes(B, ntiles));
        if (rc) return rc;
        list_base = ctx->eval.as<u64>();
        tile_wrong = (unsigned *)(list_base + 1);
        wrong_flag = ctx->eval.as<u8>() + scratch_bytes(0, ntiles);
    }
    if (prob)
        hipLaunchKernelGGL(k_eval_cells<true>, dim3(grid), dim3(EV_TILE), 0, s, input, labels, (int)i64, B, ntiles, T, edges, n_bins, probs, pred, conf, true_prob, nll,
                           correct, stats, tile_wrong, wrong_flag);
    else
        hipLaunchKernelGGL(k_eval_cells<false>, dim3(grid), dim3(EV_TILE), 0, s, input, labels, (int)i64, B, ntiles, T, edges, n_bins, probs, pred, conf, true_prob, nll,
                           correct, stats, tile_wrong, wrong_flag);
    SV_LAUNCH_CHECK("k_eval_cells");
    if (max_failures > 0) {
        hipLaunchKernelGGL(k_eval_scan, dim3(1), dim3(256), 0, s, tile_wrong, ntiles, (const sv_eval_stats *)stats, list_base);
        SV_LAUNCH_CHECK("k_eval_scan");
        if (prob)
            hipLaunchKernelGGL(k_eval_failures<true>, dim3((unsigned)ntiles), dim3(EV_TILE), 0, s, input, labels, (int)i64, B, index_base, T,
                               (const unsigned *)tile_wrong, (const u8 *)wrong_flag, (const u64 *)list_base, failures, max_failures);
        else
            hipLaunchKernelGGL(k_eval_failures<false>, dim3((unsigned)ntiles), dim3(EV_TILE), 0, s, input, labels, (int)i64, B, index_base, T,
                               (const unsigned *)tile_wrong, (const u8 *)wrong_flag, (const u64 *)list_base, failures, max_failures);
        SV_LAUNCH_CHECK("k_eval_failures");
    }
    return SV_OK;
}
