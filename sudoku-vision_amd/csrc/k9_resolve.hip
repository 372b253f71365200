// K9 -- run_v2's validation and correction stage (pipeline/run_v2.py:344-371: validate_predictions, pipeline/validator.py:69-159, then
// resolve_conflicts, pipeline/conflict_resolver.py:58-286) for n frames in one launch, exact to the bit (DESIGN.md "K9").
//
//   k_resolve : one wave (a 64-thread workgroup) per frame.
//     phase 1   the frame's top-k goes to LDS once; the wave validates it (below).  A valid frame writes its outputs and leaves.
//     phase 2   beam search.  A path is the frame in LDS plus a Path record: its corrections and the full new state of the <= 3 cells
//               they touched.  Per depth, for every path of the beam the wave validates it and ranks its correction candidates;
//               then lane 10 p + c applies candidate c to path p, which changes one cell, so it re-validates from the path's
//               per-(unit, digit) counts with six LDS reads and scores in f64; then the winner or the next beam is selected.
//
// Validation, spread over the lanes: a lane owns cells `lane` and `lane + 64`.  For each digit d = 1..9 two ballots give the 81-bit
// mask of the cells showing d; a unit's count of d is one AND and a popcount against the unit's mask, so lanes 0..26 (one unit each)
// count the conflicts, and a lane whose cell shows d reads off how many of its three units repeat it and which conflict names the
// cell first.  No array is indexed by a run-time value in registers; everything that is lives in LDS.
//
// accept != 0 applies run_v2's acceptance rule (pipeline/run_v2.py:365) before the outputs are written.
//
// Order rules (all from the reference): candidates by (conflicts of the cell descending, its confidence ascending,
// the alternative's confidence descending, the order validate_predictions first names the cell, the alternative's slot), first 10;
// paths are evaluated in (beam, candidate) order = lane order; the first valid path of the strictly lowest score wins; the next beam
// is what heapq.nsmallest returns for objects that compare by score alone, which one lane replays (next_beam).
#include "sv_device.h"
#include "sv_internal.h"
#include "sv_m81.h"

namespace {

constexpr int RB = 6;            // paths in a beam, at most
constexpr int RC = 10;           // candidates kept per path
constexpr int RM = 3;            // corrections of a path, at most
constexpr int RENT = 81 * 3;     // candidates of a path before the cut, at most
constexpr uint32_t RNONE = 255;  // an alternative slot that holds nothing

__device__ __forceinline__ float sel4(float4 v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
__device__ __forceinline__ uint32_t byte_of(uint32_t w, int j) { return (w >> (8 * j)) & 255u; }

struct Path {
    uint32_t ncorr, nov;         // corrections made; cells they touched
    uint32_t corr[RM];           // cell | old digit << 8 | new digit << 16
    float corr_old[RM], corr_new[RM];
    uint32_t ov_cell[RM];
    uint32_t ov_dg[RM];          // the touched cell's digit and alternatives, a byte each (RNONE: nothing)
    float4 ov_pr[RM];            // and their probabilities
};

constexpr int P_RESULT = 2 * RB, P_START = 2 * RB + 1;

struct Smem {
    float4 pr[81];               // the frame as read: probabilities
    uint32_t dg[81];             //                   digit and alternatives, a byte each
    Path path[2 * RB + 2];       // two beams, the winner, the uncorrected frame
    uint64_t ent[RENT][2];       // a path's candidates as sort keys
    double psum[RB];             // per beam path: sum of the confidences of its filled cells
    double sc[64];               // scores of a depth's invalid paths, in evaluation order
    int pfill[RB], pnconf[RB], ncand[RB];
    int heap[RB], nsel;
    uint16_t cand[RB][RC];       // cell | slot << 7
    u8 cnt[RB][27][12];          // [path][unit][digit]: cells of the unit showing the digit
};

__device__ __forceinline__ void cell_state(const Smem &S, const Path &P, int x, uint32_t &dg, float4 &pr)
{
    dg = S.dg[x];
    pr = S.pr[x];
#pragma unroll
    for (int i = 0; i < RM; i++)
        if (i < (int)P.nov && (int)P.ov_cell[i] == x) { dg = P.ov_dg[i]; pr = P.ov_pr[i]; }
}

// what validation tells a lane about one of its cells: how many conflicts name it, and a key that orders cells as
// validate_predictions first names them (unit, then the first cell of the unit showing the digit, then the cell)
__device__ __forceinline__ void cell_conflicts(m81 m, int x, int &cc, uint32_t &fn)
{
    const int r = x / 9, c = x % 9, b = box_of(x);
    const m81 mr = m & row_mask(r), mc = m & col_mask(c), mb = m & box_mask(b);
    const bool inr = pop(mr) >= 2, inc = pop(mc) >= 2, inb = pop(mb) >= 2;
    cc = inr + inc + inb;
    const int unit = inr ? r : inc ? 9 + c : 18 + b;
    const int head = inr ? first(mr) : inc ? first(mc) : first(mb);
    fn = (uint32_t)((unit * 81 + head) * 81 + x);
}

struct Analysis {
    uint32_t dg[2];      // the lane's two cells (the second only for lane < 17)
    float4 pr[2];
    int cc[2];
    uint32_t fn[2];
    int nconf, nfill;    // uniform
    double sum;          // uniform
};

// The whole wave validates path P.  cnt: where to leave the per-(unit, digit) counts, or nullptr.
__device__ __forceinline__ void analyse(const Smem &S, const Path &P, int lane, u8 (*cnt)[12], Analysis &A)
{
    const bool has1 = lane < 81 - 64;
    cell_state(S, P, lane, A.dg[0], A.pr[0]);
    cell_state(S, P, has1 ? lane + 64 : 80, A.dg[1], A.pr[1]);
    const int d0 = A.dg[0] & 255, d1 = has1 ? (int)(A.dg[1] & 255) : 0;
    const m81 unit = unit_mask(min(lane, 26));
    A.cc[0] = A.cc[1] = 0;
    A.fn[0] = A.fn[1] = 0;
    A.nconf = 0;
#pragma unroll
    for (int d = 1; d <= 9; d++) {
        const m81 m = {__ballot(d0 == d), __ballot(d1 == d)};
        const int c = pop(m & unit);
        if (cnt && lane < 27) cnt[lane][d] = (u8)c;
        A.nconf += __popcll(__ballot(lane < 27 && c >= 2));
        if (d0 == d) cell_conflicts(m, lane, A.cc[0], A.fn[0]);
        if (d1 == d) cell_conflicts(m, lane + 64, A.cc[1], A.fn[1]);
    }
    A.nfill = __popcll(__ballot(d0 > 0)) + __popcll(__ballot(d1 > 0));
    // every confidence is an f32 and the sum of 81 of them is exact in a double whenever none is below 2^-18: any order will do
    double s = (d0 > 0 ? (double)A.pr[0].x : 0.0) + (d1 > 0 ? (double)A.pr[1].x : 0.0);
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    A.sum = s;
}

// _score_path: single IEEE double operations (this file is built with -ffp-contract=off)
__device__ __forceinline__ double path_score(int nconf, double sum, int nfill)
{
    const double avg = nfill > 0 ? sum / (double)nfill : 0.0;
    return (double)(nconf * 100) + (1.0 - avg) * 10.0;
}

// dst = src with alternative `slot` (1..3) of cell x installed; dg, pr: x's state in src.  One lane.
__device__ __forceinline__ void make_child(Path &dst, const Path &src, int x, int slot, uint32_t dg, float4 pr)
{
    dst.ncorr = src.ncorr;
    dst.nov = src.nov;
#pragma unroll
    for (int i = 0; i < RM; i++) {
        dst.corr[i] = src.corr[i]; dst.corr_old[i] = src.corr_old[i]; dst.corr_new[i] = src.corr_new[i];
        dst.ov_cell[i] = src.ov_cell[i]; dst.ov_dg[i] = src.ov_dg[i]; dst.ov_pr[i] = src.ov_pr[i];
    }
    const uint32_t a = dg & 255, b = byte_of(dg, slot);
    const float ca = pr.x, cb = sel4(pr, slot);
    const int i = min((int)src.ncorr, RM - 1);
    dst.corr[i] = (uint32_t)x | a << 8 | b << 16;
    dst.corr_old[i] = ca;
    dst.corr_new[i] = cb;
    dst.ncorr = i + 1;
    int o = min((int)src.nov, RM - 1);
    bool fresh = true;
#pragma unroll
    for (int j = RM - 1; j >= 0; j--)
        if (j < (int)src.nov && (int)src.ov_cell[j] == x) { o = j; fresh = false; }
    if (fresh) dst.nov = o + 1;
    dst.ov_cell[o] = x;
    // [(old digit, old confidence)] + [every alternative that does not name the new digit]
    u8 *db = reinterpret_cast<u8 *>(&dst.ov_dg[o]);
    float *pb = reinterpret_cast<float *>(&dst.ov_pr[o]);
    db[0] = (u8)b; pb[0] = cb;
    db[1] = (u8)a; pb[1] = ca;
    int n = 2;
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const uint32_t ad = byte_of(dg, j);
        if (ad != RNONE && ad != b && n < 4) { db[n] = (u8)ad; pb[n] = sel4(pr, j); n++; }
    }
    for (; n < 4; n++) { db[n] = (u8)RNONE; pb[n] = 0.f; }
}

// heapq.nsmallest(bw, paths) for m paths that compare by score alone (S.sc, evaluation order): leaves the chosen paths' numbers in
// S.heap in beam order and returns how many.  m <= bw: a stable sort.  Otherwise CPython's own procedure, because it is not the
// first bw of a stable sort: a max-heap of bw paths (heapify, then every later path that is strictly better than the root replaces
// it and sifts), and at the end the heap's array is sorted stably by score.  One lane.
__device__ void next_beam(Smem &S, int m, int bw)
{
    int *heap = S.heap;
    const double *sc = S.sc;
    const int n = min(m, bw);
    for (int i = 0; i < n; i++) heap[i] = i;
    if (m > bw) {
        auto settle = [&](int pos) {      // heapq._siftup_max: the larger child (the right one when equal) moves up to a leaf ...
            const int start = pos, item = heap[pos];
            int child = 2 * pos + 1;
            while (child < n) {
                if (child + 1 < n && !(sc[heap[child + 1]] < sc[heap[child]])) child++;
                heap[pos] = heap[child];
                pos = child;
                child = 2 * pos + 1;
            }
            while (pos > start && sc[heap[(pos - 1) >> 1]] < sc[item]) {   // ... then the item climbs while its parent is smaller
                heap[pos] = heap[(pos - 1) >> 1];
                pos = (pos - 1) >> 1;
            }
            heap[pos] = item;
        };
        for (int pos = n / 2 - 1; pos >= 0; pos--) settle(pos);
        for (int i = n; i < m; i++)
            if (sc[i] < sc[heap[0]]) { heap[0] = i; settle(0); }
    }
    for (int i = 1; i < n; i++) {         // stable
        const int v = heap[i];
        int j = i;
        while (j > 0 && sc[v] < sc[heap[j - 1]]) { heap[j] = heap[j - 1]; j--; }
        heap[j] = v;
    }
    S.nsel = n;
}

struct ResolveOut {
    u8 *digits; float *conf; u8 *index; float *prob; u8 *success; int *before; int *after; u8 *conflict_count; u8 *ncorr; u8 *corr_cells;
    float *corr_conf; int *explored; double *score;
};

__global__ __launch_bounds__(64) void k_resolve(const u8 *index, const float *prob, int k, int bw, int maxc, double min_alt, int accept, ResolveOut out)
{
    __shared__ Smem S;
    const int lane = threadIdx.x;
    const long f = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1;

    // ---- phase 1: the frame, once ----------------------------------------------------------------------------------------------------
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int x = lane + 64 * s;
        if (x < 81) {
            uint32_t dg = 0;
            float p[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t d = RNONE;
                if (j < k) {
                    d = index[(f * 81 + x) * k + j];
                    p[j] = prob[(f * 81 + x) * k + j];
                    if (d > 9) d = j ? RNONE : 0;        // not a class: an empty cell, or no alternative
                }
                dg |= d << (8 * j);
            }
            S.dg[x] = dg;
            S.pr[x] = make_float4(p[0], p[1], p[2], p[3]);
        }
    }
    if (lane == 0) S.path[P_START].ncorr = S.path[P_START].nov = S.path[0].ncorr = S.path[0].nov = 0;
    __syncthreads();

    Analysis A;
    analyse(S, S.path[P_START], lane, S.cnt[0], A);
    const int before = A.nconf;
    int result = P_START, success = 1, explored = 1;
    double score = 0.0;

    // ---- phase 2: beam search --------------------------------------------------------------------------------------------------------
    if (before > 0) {
        success = 0;
        int cur = 0, nbeam = 1;
        result = -1;
        for (int depth = 0; depth < maxc && result < 0; depth++) {
            for (int p = 0; p < nbeam; p++) {
                const Path &P = S.path[cur * RB + p];
                analyse(S, P, lane, S.cnt[p], A);
                if (lane == 0) { S.psum[p] = A.sum; S.pfill[p] = A.nfill; S.pnconf[p] = A.nconf; }
                // _get_correction_candidates: every alternative of a conflicted cell that names another digit with enough confidence
                int total = 0;
#pragma unroll
                for (int s = 0; s < 2; s++) {
                    const uint32_t digit = A.dg[s] & 255;
                    const int x = lane + 64 * s;
#pragma unroll
                    for (int j = 1; j < 4; j++) {
                        const uint32_t ad = byte_of(A.dg[s], j);
                        const float ap = sel4(A.pr[s], j);
                        const bool ok = x < 81 && A.cc[s] > 0 && ad != RNONE && ad != digit && (double)ap >= min_alt;
                        const uint64_t votes = __ballot(ok);
                        if (ok) {
                            const int e = total + __popcll(votes & below);
                            S.ent[e][0] = (uint64_t)(3 - A.cc[s]) << 32 | __float_as_uint(A.pr[s].x);
                            S.ent[e][1] = (uint64_t)(~__float_as_uint(ap)) << 32 | (A.fn[s] << 9 | (uint32_t)(j - 1) << 7 | (uint32_t)x);
                        }
                        total += __popcll(votes);
                    }
                }
                __syncthreads();
                for (int e = lane; e < total; e += 64) {     // the keys are distinct: a candidate's rank is how many sort before it
                    const uint64_t k0 = S.ent[e][0], k1 = S.ent[e][1];
                    int rank = 0;
                    for (int i = 0; i < total; i++) {
                        const uint64_t o0 = S.ent[i][0], o1 = S.ent[i][1];
                        rank += o0 < k0 || (o0 == k0 && o1 < k1);
                    }
                    if (rank < RC) S.cand[p][rank] = (uint16_t)(k1 & 0x1FF);
                }
                if (lane == 0) S.ncand[p] = min(total, RC);
                __syncthreads();
            }

            // lane 10 p + c: candidate c of path p
            const int p = lane / RC, c = lane - p * RC;
            const bool active = p < nbeam && c < S.ncand[min(p, RB - 1)];
            int x = 0, slot = 1, nconf = 1;
            uint32_t dg = 0;
            float4 pr = make_float4(0.f, 0.f, 0.f, 0.f);
            double sc = 0.0;
            if (active) {
                const Path &P = S.path[cur * RB + p];
                const uint32_t cd = S.cand[p][c];
                x = cd & 127;
                slot = 1 + (cd >> 7);
                cell_state(S, P, x, dg, pr);
                const uint32_t a = dg & 255, b = byte_of(dg, slot);
                const int units[3] = {x / 9, 9 + x % 9, 18 + box_of(x)};
                nconf = S.pnconf[p];
                int nfill = S.pfill[p];
                double sum = S.psum[p];
#pragma unroll
                for (int u = 0; u < 3; u++) {
                    if (a > 0 && S.cnt[p][units[u]][a] == 2) nconf--;     // the old digit's conflict in this unit had two cells
                    if (b > 0 && S.cnt[p][units[u]][b] == 1) nconf++;     // the new digit meets its first peer
                }
                if (a > 0) { sum -= (double)pr.x; nfill--; }              // exact, as the sum itself
                if (b > 0) { sum += (double)sel4(pr, slot); nfill++; }
                sc = path_score(nconf, sum, nfill);
            }
            const uint64_t evaluated = __ballot(active), valid = __ballot(active && nconf == 0);
            if (valid) {
                // the first valid path of the strictly lowest score, and the counter as it stood when that path was evaluated
                double best = active && nconf == 0 ? sc : __longlong_as_double(0x7FF0000000000000ll);
                for (int o = 32; o > 0; o >>= 1) best = fmin(best, __shfl_xor(best, o));
                const int win = __ffsll((long long)__ballot(active && nconf == 0 && sc == best)) - 1;
                if (lane == win) make_child(S.path[P_RESULT], S.path[cur * RB + p], x, slot, dg, pr);
                explored += __popcll(evaluated & ((2ull << win) - 1));
                score = best;
                success = 1;
                result = P_RESULT;
            } else if (!evaluated) {
                result = P_START;                                          // nothing left to try: the uncorrected frame
            } else {
                const int m = __popcll(evaluated), mine = __popcll(evaluated & below);
                explored += m;
                if (active) S.sc[mine] = sc;
                __syncthreads();
                if (lane == 0) next_beam(S, m, bw);
                __syncthreads();
                const int nsel = S.nsel;
                for (int r = 0; r < nsel; r++)
                    if (active && S.heap[r] == mine) make_child(S.path[(cur ^ 1) * RB + r], S.path[cur * RB + p], x, slot, dg, pr);
                nbeam = nsel;
                cur ^= 1;
            }
            __syncthreads();
        }
        if (result < 0) result = cur * RB;                                 // no valid path: the best of the last beam
    }

    // ---- outputs: the chosen path, validated once more for its conflicts ---------------------------------------------------------------
    int after = 0;
    if (result != P_START || before > 0) {
        analyse(S, S.path[result], lane, nullptr, A);
        after = A.nconf;
        // run_v2's acceptance rule (pipeline/run_v2.py:365), when asked for: a repair that neither succeeded nor left fewer conflicts
        // is dropped and the outputs describe the frame as it came
        if (accept && !success && after >= before && result != P_START) {
            result = P_START;
            analyse(S, S.path[result], lane, nullptr, A);
            after = A.nconf;
        }
    }
    const Path &R = S.path[result];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const int x = lane + 64 * s;
        if (x < 81) {
            const long o = f * 81 + x;
            if (out.digits) out.digits[o] = (u8)(A.dg[s] & 255);
            if (out.conf) out.conf[o] = A.pr[s].x;
            if (out.conflict_count) out.conflict_count[o] = (u8)A.cc[s];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (j < k) {
                    if (out.index) out.index[o * k + j] = (u8)byte_of(A.dg[s], j);
                    if (out.prob) out.prob[o * k + j] = sel4(A.pr[s], j);
                }
            }
        }
    }
    if (lane == 0) {
        if (out.success) out.success[f] = (u8)success;
        if (out.before) out.before[f] = before;
        if (out.after) out.after[f] = after;
        if (out.ncorr) out.ncorr[f] = (u8)R.ncorr;
        if (out.explored) out.explored[f] = explored;
        if (out.score) out.score[f] = score;
    }
    if (lane < RM) {
        const bool made = lane < (int)R.ncorr;
        const uint32_t cd = made ? R.corr[lane] : 0;
        if (out.corr_cells) {
            u8 *q = out.corr_cells + (f * RM + lane) * 3;
            q[0] = (u8)(cd & 255); q[1] = (u8)byte_of(cd, 1); q[2] = (u8)byte_of(cd, 2);
        }
        if (out.corr_conf) {
            out.corr_conf[(f * RM + lane) * 2] = made ? R.corr_old[lane] : 0.f;
            out.corr_conf[(f * RM + lane) * 2 + 1] = made ? R.corr_new[lane] : 0.f;
        }
    }
}

}  // namespace

int svk_resolve_conflicts(const u8 *index, const float *prob, long n, int k, int beam_width, int max_corrections, double min_alt_conf, int accept, u8 *digits,
                          float *conf, u8 *index_out, float *prob_out, u8 *success, int *before, int *after, u8 *conflict_count, u8 *ncorr,
                          u8 *corr_cells, float *corr_conf, int *explored, double *score, hipStream_t s)
{
    const ResolveOut out = {digits, conf, index_out, prob_out, success, before, after, conflict_count, ncorr, corr_cells, corr_conf, explored, score};
    hipLaunchKernelGGL(k_resolve, dim3((unsigned)n), dim3(64), 0, s, index, prob, k, beam_width, max_corrections, min_alt_conf, accept, out);
    SV_LAUNCH_CHECK("k_resolve");
    return SV_OK;
}
