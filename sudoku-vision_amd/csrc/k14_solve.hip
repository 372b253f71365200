// K14 -- run_v2's last stage, run_solver (pipeline/run_v2.py:393-407), for n grids in one launch: solver/src/sudoku.c with the decision
// order of host_solver.cpp, so every result, solution and node count equals sv_solve_sudoku_batch_host's (DESIGN.md "K14").
//
//   k_solve : one wave (a 64-thread workgroup) per grid.  A lane owns cells `lane` and `lane + 64`: their values and their candidates
//   (a mask, bit d = d possible, 0 for a filled cell) stay in its registers.  Everything the wave decides on is uniform: it comes out of
//   a ballot, a shuffle from a uniform lane, or LDS.
//     validate   validate_grid (sudoku.c:413-467): a byte above 9, or per digit a unit (lanes 0..26, one each) showing it twice
//     init       init_candidates (:226-247): an empty cell loses every digit one of its peers shows
//     propagate  (:287-401) the reference's sweeps in the reference's order.  Naked singles: the first empty cell at or after a cursor
//                with at most one candidate is what the row-major scan acts on next (nothing changes before it is reached): none left
//                is the contradiction, one is placed and the cursor moves past the cell.  Hidden singles: the same with a cursor over
//                (unit, digit), rows, columns, boxes, digits ascending: lane u sees for each digit whether unit u lacks it and has at
//                most one place for it; the first such entry at or after the cursor is the one the reference's loops act on next.
//                Each placement is followed by a fresh look, so a later entry is always judged on the state the reference judges it on.
//     search     solve_with_candidates (:6-59) without recursion: a level of the stack is the state after its node's propagate (81 x
//                u16: candidates | value << 10) plus the branch cell and the digits of it not yet tried.  A node is one propagate.
//   No array is indexed by a run-time value in registers (k10_propagate.hip says why); the stack is LDS.
//
// Every loop is bounded: nodes by max_nodes, sweeps of a node by 82 (each but the last places a cell), the scans of a sweep by 82 (81
// placements and the look that finds nothing), the unwinding of the stack by its 81 levels, digits by 9.  Nothing waits on memory
// another workgroup writes.
#include "sv_device.h"
#include "sv_internal.h"
#include "sv_m81.h"

namespace {

constexpr int LEVELS = 81;            // a level per empty cell at most: every level below the top has placed its branch cell
constexpr int SCANS = 82;             // looks of one scan: 81 placements and the one that finds nothing
constexpr uint32_t ALL = 0x3FE;       // candidates 1..9
constexpr int NOCELL = 15;            // the value of the second cell of lanes 17..63, which does not exist: never empty, never a digit

struct Stack {
    uint16_t st[LEVELS][81];          // per level and cell: candidates | value << 10
    uint32_t pend[LEVELS];            // per level: branch cell << 16 | candidates of it still to be tried
};

struct Cells {
    uint32_t v[2], c[2];              // the lane's two cells: value, candidates
    m81 peers[2];                     // the 20 peers of each (none for a cell that does not exist)
};

// the wave puts d into cell x (both uniform): the cell is filled and its peers lose the digit (eliminate_from_peers, sudoku.c:251-283)
__device__ __forceinline__ void place(Cells &C, int lane, int x, int d)
{
    const int l = x & 63;
    const uint32_t keep = ~(1u << d);
    if (x < 64) {
        if (C.peers[0].lo >> l & 1) C.c[0] &= keep;
        if (C.peers[1].lo >> l & 1) C.c[1] &= keep;
        if (lane == l) { C.v[0] = d; C.c[0] = 0; }
    } else {
        if (C.peers[0].hi >> l & 1) C.c[0] &= keep;
        if (C.peers[1].hi >> l & 1) C.c[1] &= keep;
        if (lane == l) { C.v[1] = d; C.c[1] = 0; }
    }
}

// candidates of cell x (uniform), uniform
__device__ __forceinline__ uint32_t cand_of(const Cells &C, int x)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)(x < 64 ? C.c[0] : C.c[1]), x & 63);
}

// propagate(), sudoku.c:287-401 -> false on a contradiction
__device__ bool propagate(Cells &C, int lane, m81 unit)
{
    for (int sweep = 0; sweep < 82; sweep++) {
        bool progress = false;
        // naked singles, row-major, each placed before the next cell is looked at
        int cursor = 0;
        for (int look = 0; look < SCANS; look++) {
            const m81 due = {__ballot(C.v[0] == 0 && __popc(C.c[0]) <= 1 && lane >= cursor),
                             __ballot(C.v[1] == 0 && __popc(C.c[1]) <= 1 && lane + 64 >= cursor)};
            if (!any(due)) break;
            const int x = first(due);
            const uint32_t c = cand_of(C, x);
            if (c == 0) return false;
            place(C, lane, x, __ffs((int)c) - 1);
            cursor = x + 1;
            progress = true;
        }
        // hidden singles: units in order, digits ascending; the cursor is unit << 4 | digit
        int at = 1;
        for (int look = 0; look < SCANS; look++) {
            uint32_t due = 0;
#pragma unroll
            for (int d = 1; d <= 9; d++) {
                const m81 shown = {__ballot(C.v[0] == (uint32_t)d), __ballot(C.v[1] == (uint32_t)d)};
                const m81 open = {__ballot(C.c[0] >> d & 1), __ballot(C.c[1] >> d & 1)};      // a filled cell has no candidates
                if (!any(shown & unit) && pop(open & unit) <= 1) due |= 1u << d;
            }
            const int u0 = at >> 4;
            if (lane > 26 || lane < u0) due = 0;
            if (lane == u0) due &= ~((1u << (at & 15)) - 1);
            const uint64_t units = __ballot(due != 0);
            if (!units) break;
            const int u = __ffsll((long long)units) - 1;
            const int d = __ffs(__builtin_amdgcn_readlane((int)due, u)) - 1;
            const m81 spots = m81{__ballot(C.c[0] >> d & 1), __ballot(C.c[1] >> d & 1)} & unit_mask(u);
            if (!any(spots)) return false;
            place(C, lane, first(spots), d);
            at = u << 4 | (d + 1);
            progress = true;
        }
        if (!progress) break;
    }
    return true;
}

__global__ __launch_bounds__(64) void k_solve(const u8 *grid, const u8 *active, int max_nodes, u8 *solution, int8_t *result, int *nodes_out)
{
    __shared__ Stack S;
    const int lane = threadIdx.x;
    const long f = blockIdx.x;
    const bool has1 = lane < 81 - 64;

    const uint32_t g0 = grid[f * 81 + lane], g1 = has1 ? grid[f * 81 + 64 + lane] : NOCELL;
    Cells C;
    C.v[0] = g0;
    C.v[1] = g1;
    C.c[0] = C.c[1] = 0;
    const m81 unit = unit_mask(min(lane, 26));

    int res = SV_SOLVE_SKIPPED, nodes = 0;
    if (!active || active[f]) {
        // ---- validate_grid ----------------------------------------------------------------------------------------------------------
        bool twice = false;
#pragma unroll
        for (int d = 1; d <= 9; d++) {
            const m81 shown = {__ballot(g0 == (uint32_t)d), __ballot(g1 == (uint32_t)d)};
            twice |= pop(shown & unit) > 1;
        }
        if (__ballot(g0 > 9 || (has1 && g1 > 9) || (lane < 27 && twice))) {
            res = -1;
        } else {
            // ---- init_candidates ----------------------------------------------------------------------------------------------------
#pragma unroll
            for (int s = 0; s < 2; s++) {
                const int x = lane + 64 * s;
                const int y = min(x, 80);
                const m81 all = row_mask(y / 9) | col_mask(y % 9) | box_mask(box_of(y));
                C.peers[s] = x < 81 ? all & ~shl({1, 0}, y) : m81{0, 0};
                C.c[s] = C.v[s] ? 0 : ALL;
            }
#pragma unroll
            for (int d = 1; d <= 9; d++) {
                const m81 shown = {__ballot(g0 == (uint32_t)d), __ballot(g1 == (uint32_t)d)};
#pragma unroll
                for (int s = 0; s < 2; s++)
                    if (any(shown & C.peers[s])) C.c[s] &= ~(1u << d);
            }

            // ---- solve_with_candidates ----------------------------------------------------------------------------------------------
            int depth = 0;
            res = SV_SOLVE_BUDGET;
            for (int entry = 0; entry <= max_nodes; entry++) {
                if (nodes == max_nodes) break;                        // a node is due and the budget is spent
                nodes++;
                int pushed = -1;
                if (propagate(C, lane, unit)) {
                    // the first empty cell with the fewest candidates
                    int best = -1;
                    for (int k = 0; k <= 9 && best < 0; k++) {
                        const m81 m = {__ballot(C.v[0] == 0 && __popc(C.c[0]) == k), __ballot(C.v[1] == 0 && __popc(C.c[1]) == k)};
                        if (any(m)) best = first(m);
                    }
                    if (best < 0) { res = 1; break; }                 // no empty cell left: solved
                    const uint32_t todo = cand_of(C, best);
                    pushed = min(depth, LEVELS - 1);
                    S.st[pushed][lane] = (uint16_t)(C.c[0] | C.v[0] << 10);
                    if (has1) S.st[pushed][lane + 64] = (uint16_t)(C.c[1] | C.v[1] << 10);
                    if (lane == 0) S.pend[pushed] = (uint32_t)best << 16 | todo;
                    depth = pushed + 1;
                    __syncthreads();
                }
                // the deepest level that has a digit left to try
                uint32_t p = 0;
                for (int k = 0; k <= LEVELS; k++) {
                    if (depth == 0) break;
                    p = __builtin_amdgcn_readfirstlane(S.pend[depth - 1]);
                    if (p & ALL) break;
                    depth--;
                }
                if (depth == 0) { res = 0; break; }
                const int d = __ffs((int)(p & ALL)) - 1;
                __syncthreads();
                if (lane == 0) S.pend[depth - 1] = p & ~(1u << d);
                if (depth - 1 != pushed) {                            // an older level: its state comes back from the stack
                    const uint32_t a = S.st[depth - 1][lane], b = has1 ? S.st[depth - 1][lane + 64] : (uint32_t)NOCELL << 10;
                    C.c[0] = a & 0x3FF; C.v[0] = a >> 10;
                    C.c[1] = b & 0x3FF; C.v[1] = b >> 10;
                }
                place(C, lane, (int)(p >> 16) & 127, d);
                __syncthreads();
            }
            if (res != 1) { C.v[0] = g0; C.v[1] = g1; }             // the solution is the grid unless solved
        }
    }

    if (solution) {
        solution[f * 81 + lane] = (u8)C.v[0];
        if (has1) solution[f * 81 + 64 + lane] = (u8)C.v[1];
    }
    if (lane == 0) {
        if (result) result[f] = (int8_t)res;
        if (nodes_out) nodes_out[f] = res == -1 ? 0 : nodes;
    }
}

}  // namespace

int svk_solve_sudoku_batch(const u8 *grid, const u8 *active, int n, int max_nodes, u8 *solution, int8_t *result, int *nodes, hipStream_t s)
{
    hipLaunchKernelGGL(k_solve, dim3((unsigned)n), dim3(64), 0, s, grid, active, max_nodes, solution, result, nodes);
    SV_LAUNCH_CHECK("k_solve");
    return SV_OK;
}
