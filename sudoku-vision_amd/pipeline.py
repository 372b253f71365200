"""End-to-end frame -> digits pipeline with the host corner search in the loop -- the build's counterpart
of the hot section of pipeline/run.py:244-312 (call order, glue, output conventions), batched and
software-pipelined for a resident pool of frames:

    GPU  K1 (binary) -> despeckle  --D2H, pinned-->  CPU contour corner search (threads)  --Minv, H2D-->  GPU  K2 -> K3

Chunks of frames are double-buffered: while the host searches chunk i, the GPU thresholds chunk i+1 and
classifies chunk i-1.  `glue` selects what sits between extract_cells and the model (see include/sudoku_vision_hip.h sv_glue).
A frame whose grid is not found gets found=False and digits 0 (the reference
returns "Grid detection failed" for it, pipeline/run.py:268-272); so does a frame whose four corners do not define a
homography (order_points, cv/grid.py:79-91, returns one point twice for a quad rotated near 45 degrees; the reference
warps garbage for that image) -- one such frame never affects the others of its batch."""
import os
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field

import numpy as np
import torch

from . import host
from .runtime import Context


def host_cpu_budget():
    """CPUs this process may actually use: the cgroup CPU quota when there is one (a box gives each GPU job 16 of the host's
    256 logical CPUs through cpu.max; running more runnable threads than the quota gets the whole group throttled for the rest
    of the period -- 30 ms stalls in the corner search), else the affinity mask."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: t.split()),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", lambda t: [t.strip(), open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().strip()])):
        try:
            quota, period = parse(open(path).read())
            if quota not in ("max", "-1"):
                n = min(n, max(1, int(quota) // int(period)))
            break
        except (OSError, ValueError):
            continue
    return n


def _parse_cpulist(text):
    cpus = set()
    for part in text.strip().split(","):
        if part:
            lo, _, hi = part.partition("-")
            cpus.update(range(int(lo), int(hi or lo) + 1))
    return cpus


def gpu_local_cpus(device):
    """CPUs of the NUMA node the GPU hangs off (sysfs local_cpulist of its PCI function) that this process may run on, or None when
    the platform does not say.  The pipeline's pinned buffers are first touched, hence placed, there; host threads that wander to the
    other socket of a two-socket box run the search 10-20 % slower and with 40-ms outliers (tools/dev/e2e_stall_trace.py)."""
    try:
        p = torch.cuda.get_device_properties(device)
        path = f"/sys/bus/pci/devices/{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0/local_cpulist"
        cpus = _parse_cpulist(open(path).read())
    except (OSError, ValueError, AttributeError, RuntimeError):
        return None
    if hasattr(os, "sched_getaffinity"):
        cpus &= os.sched_getaffinity(0)
    return cpus or None


class FramePipeline:
    def __init__(self, ctx: Context, H: int, W: int, chunk: int = 32, host_threads=None, min_area_ratio=0.1, glue=0, despeckle=True, sparse=True, depth=5, cpu_affinity="auto", bits_direct=True,
                 quality=False, resolve=False, propagate=False, solve=False, solve_max_nodes=4096):
        self.ctx, self.H, self.W, self.chunk = ctx, H, W, chunk
        # chunks in flight.  A chunk's chain is K1 -> D2H -> search -> K2/K3, and chunk i's K1 is only issued once chunk i-depth+1's search has
        # returned: with too few in flight the period is (K1 + D2H + search) / (depth - 1), not the slowest stage
        self.depth = depth = max(2, int(depth))
        self.host_threads = host_threads or max(1, host_cpu_budget() - 2)   # two CPUs left for this thread and the runtime's own
        self.min_area_ratio = min_area_ratio
        # the speck filter is exact only while nothing it can erase (bounding box <= 62x62 px, area <= 61*61) reaches the
        # search's area floor (include/sudoku_vision_hip.h, sv_despeckle_u8): small frames go through unfiltered
        self.despeckle = bool(despeckle) and min_area_ratio * H * W > 61 * 61
        self.glue = glue            # Context.GLUE_NORMALIZE, or GLUE_RUNPY for run.py's preprocess_cell (CLAHE + threshold)
        dev = ctx.device
        self.s_pre = torch.cuda.Stream(dev)       # K1 (+ despeckle)
        self.s_d2h = torch.cuda.Stream(dev)       # the D2H copy on its own stream: in s_pre it would hold back the next chunk's K1 for 0.3 ms
        self.s_cls = torch.cuda.Stream(dev)       # H2D + K2 + K3
        # D2H payload: with despeckle on and W % 32 == 0 the binary crosses PCIe as 1 bit per pixel (W/32 words per row)
        self.packed = self.despeckle and W % 32 == 0
        self.bits_direct = bool(bits_direct)        # K1 emits the bit image itself (sv_preprocess_bits_u8); False: byte image + packing despeckle
        # sparse=True (default): ... as sparse records (row masks + the non-zero words) with room for half of the words; a frame that does not
        # fit is fetched dense (sv_pack_sparse_bits).  2-3x fewer PCIe bytes on the synthetic feed for one small kernel; PCIe itself is not the
        # bound (the dense copy runs at 55 GB/s on its own stream) but the host side is: the search threads then read 138 KB of records per
        # frame instead of 259 KB of freshly DMA-written memory, and with K1 writing bits the pipeline is balanced enough for that to show
        # (128-frame chunks: 132 k frames/s sparse, 113 k dense; tools/e2e_breakdown.py)
        self.sparse = self.packed and bool(sparse) and H * ((W // 32 + 63) // 64) <= 16000
        if self.packed:
            self.dev_bits = [torch.empty((chunk, H, W // 32), dtype=torch.int32, device=dev) for _ in range(depth)]
        if self.sparse:
            # room for a third of the words (a synthetic 1080p frame keeps 13-15 k of its 64.8 k after the filter); an int: capacity in words
            # (tests force the fallback with it).  Smaller records = fewer D2H bytes: 192 k frames/s against 187 k with room for half (tools/dev/e2e_knobs.py)
            cap = H * (W // 32) // 3 if sparse is True else int(sparse)
            self.rec_bytes = host.sparse_bits_record_bytes(H, W, cap)
            self.pinned = [torch.empty((chunk, self.rec_bytes), dtype=torch.uint8).pin_memory() for _ in range(depth)]
            self.dev_rec = [torch.empty((chunk, self.rec_bytes), dtype=torch.uint8, device=dev) for _ in range(depth)]
            self.s_side = torch.cuda.Stream(dev)
        elif self.packed:
            self.pinned = [torch.empty((chunk, H, W // 32), dtype=torch.int32).pin_memory() for _ in range(depth)]
        else:
            self.pinned = [torch.empty((chunk, H, W), dtype=torch.uint8).pin_memory() for _ in range(depth)]
        self.dev_bin = None                       # byte images, only when K1 cannot write bits directly (allocated on first use)
        self.minv_pin = [torch.empty((chunk, 9), dtype=torch.float64).pin_memory() for _ in range(depth)]
        self.minv_dev = [torch.empty((chunk, 9), dtype=torch.float64, device=dev) for _ in range(depth)]
        # host threads next to the GPU: "auto" = the GPU's NUMA node, None = leave them alone, or an explicit set of CPUs.  Applies to the
        # search thread and the library's workers, not to the caller's thread
        self.cpus = gpu_local_cpus(dev) if cpu_affinity == "auto" else (set(cpu_affinity) if cpu_affinity else None)
        if self.cpus:
            host.set_pool_affinity(self.cpus)
        self.pool = ThreadPoolExecutor(1, initializer=(lambda: os.sched_setaffinity(0, self.cpus)) if self.cpus and hasattr(os, "sched_setaffinity") else None)
        self.dense_fallbacks = 0
        # quality=True: run() also returns run_v2's quality scores (cv/grid_quality.py): the frame statistics on s_pre, and the grid line
        # coverage on s_cls once the corners are known, from a per-slot copy of K1's output taken before the speck filter erases digits
        self.quality = bool(quality)
        if self.quality:
            self.q_bin = [None] * depth           # shaped on first use like K1's output (bit or byte image)
        # resolve=True: run() also returns run_v2's validation and correction stage (pipeline/run_v2.py:344-371): top-3 and the beam
        # search (csrc/k9_resolve.hip) on s_cls after K3, with run_v2's acceptance rule (:365) applied on the device
        self.resolve = bool(resolve)
        # propagate=True: run() also returns run_v2's constraint propagation (pipeline/run_v2.py:373-391, csrc/k10_propagate.hip), one more
        # launch per chunk on s_cls: on the repaired digits when resolve=True, else on the recognised ones
        self.propagate = bool(propagate)
        # solve=True: run() also returns run_v2's last stage, the solver (pipeline/run_v2.py:393-407, csrc/k14_solve.hip), one more launch per
        # chunk on s_cls, on the grid the stages before it end with, for the frames run_v2 would hand to it.  A frame that spends
        # solve_max_nodes search nodes is reported as such (Context.SOLVE_BUDGET), not finished on the host
        self.solve, self.solve_max_nodes = bool(solve), int(solve_max_nodes)
        ctx.reserve(chunk * 81)

    def _search(self, slot, m, ev):
        ev.synchronize()
        if self.sparse:
            corners, found = host.find_grid_corners_sparse_batch(self.pinned[slot][:m].numpy(), self.H, self.W, self.min_area_ratio, 0.02, self.host_threads)
            over = np.nonzero(found == 2)[0]
            if over.size:                       # records that overflowed: fetch those frames dense (the slot's bit image is still there)
                with torch.cuda.stream(self.s_side):
                    dense = self.dev_bits[slot][torch.from_numpy(over).to(self.ctx.device)].cpu().numpy()
                c2, f2 = host.find_grid_corners_bits_batch(dense, self.H, self.W, self.min_area_ratio, 0.02, self.host_threads)
                corners[over], found[over] = c2, f2
                self.dense_fallbacks += int(over.size)
            found = found.astype(bool)
        elif self.packed:
            corners, found = host.find_grid_corners_bits_batch(self.pinned[slot][:m].numpy(), self.H, self.W, self.min_area_ratio, 0.02, self.host_threads)
        else:
            corners, found = host.find_grid_corners_batch(self.pinned[slot][:m].numpy(), self.min_area_ratio, 0.02, self.host_threads)
        minv, ok = Context.corners_to_minv_batch(corners.astype(np.float32))    # not-found frames hold zeros: degenerate, identity, masked
        self.minv_pin[slot][:m] = torch.from_numpy(minv.reshape(m, 9))
        return corners, found & ok

    def describe(self):
        d2h = (f"pinned D2H of sparse records of the bit-packed binary (row masks + non-zero words, {self.rec_bytes // 1000} KB/frame over PCIe, "
               f"dense fallback {self.H * self.W // 8 // 1000} KB)" if self.sparse
               else f"pinned D2H of the bit-packed binary ({self.H * self.W // 8 // 1000} KB/frame over PCIe)" if self.packed
               else f"pinned D2H of the binary ({self.H * self.W // 1000} KB/frame over PCIe)")
        k1 = ("K1 (bit image) -> despeckle in place (exact speck filter) -> " if self.packed and self.bits_direct
              else f"K1 -> {'despeckle (exact speck filter) -> ' if self.despeckle else ''}")
        return (f"{k1}{d2h} -> C++ contour corner search on "
                f"{self.host_threads} host threads -> K2 -> K3, {self.chunk}-frame chunks, {self.depth} in flight"
                + (f", host threads on the GPU's NUMA node ({len(self.cpus)} CPUs)" if self.cpus else "")
                + (", then top-3 -> K9 (validation + beam-search conflict repair) per chunk" if self.resolve else "")
                + (", then K10 (constraint propagation) per chunk" if self.propagate else "")
                + (f", then K14 (solver, {self.solve_max_nodes} search nodes per frame at most) per chunk" if self.solve else ""))

    def run(self, frames, out=None, repeat=1, total=None):
        """frames u8 [n,H,W,3] on the context's device -> dict(digits u8[n,81], logits f32[n,81,10], conf f32[n,81],
        corners int32[n,4,2] (host), found bool[n] (host)); with quality=True also quality f32[n,6] (host: overall, sharpness, contrast,
        completeness, geometry, size -- cv/grid_quality.py's scores of each frame, NaN in the corner-dependent columns where found is False); with
        resolve=True also resolved_digits u8[n,81] (the digits after run_v2's conflict repair where run_v2 would take them, else the most
        probable class of `logits`), resolve_success bool[n] (the frame is valid: it was, or the repair made it so), num_conflicts i32[n]
        (conflicts left in resolved_digits) and n_corrections u8[n] (corrections taken), all on the device; all zero / False for a
        frame whose grid was not found; with propagate=True also propagated_digits u8[n,81] (the grid after run_v2's constraint propagation
        of resolved_digits, or of digits without resolve=True), propagate_valid bool[n] (False: run_v2 reports the frame `invalid`),
        contradiction_cell u8[n] (9 * row + col, 255 = none) and n_propagated u8[n] (cells the propagation filled), on the device; zeros,
        False and 255 for a frame whose grid was not found; with solve=True also solution u8[n,81], solve_result int8[n] and solve_nodes
        int32[n] (Context.solve_sudoku of propagated_digits, else resolved_digits, else digits, for the frames with propagate_valid, or
        without propagate=True those whose grid was found; the others are Context.SOLVE_SKIPPED), on the device.  repeat > 1 streams the pool that many times through the
        pipeline without draining it in between (steady-state throughput measurement); total = k streams exactly k frames,
        cycling the pool (the k-th frame is pool frame k mod n: BASELINE configs[3]'s shard of 100,000 frames); both need chunk | n."""
        n = frames.shape[0]
        if (repeat > 1 or total is not None) and n % self.chunk:
            raise ValueError("repeat / total need the chunk size to divide the number of frames")
        dev = self.ctx.device
        if out is None:
            out = {"logits": torch.empty((n, 81, 10), dtype=torch.float32, device=dev),
                   "digits": torch.empty((n, 81), dtype=torch.uint8, device=dev),
                   "conf": torch.empty((n, 81), dtype=torch.float32, device=dev)}
        corners_all = np.zeros((n, 4, 2), np.int32)
        found_all = np.zeros(n, bool)
        cur = torch.cuda.current_stream(dev)
        self.s_pre.wait_stream(cur)
        self.s_d2h.wait_stream(cur)
        self.s_cls.wait_stream(cur)
        # sv_preprocess_bits_u8's layout requirements (otherwise K1 writes bytes and the despeckle packs them)
        bits_direct = (self.packed and self.bits_direct and frames.is_contiguous() and frames.data_ptr() % 4 == 0 and (3 * self.W) % 4 == 0
                       and self.H >= 16 and self.W >= 16)
        if not bits_direct and self.dev_bin is None:
            self.dev_bin = [torch.empty((self.chunk, self.H, self.W), dtype=torch.uint8, device=dev) for _ in range(self.depth)]
        if self.quality:
            qshape, qtype = ((self.chunk, self.H, self.W // 32), torch.int32) if bits_direct else ((self.chunk, self.H, self.W), torch.uint8)
            if self.q_bin[0] is None or tuple(self.q_bin[0].shape) != qshape or self.q_bin[0].dtype != qtype:
                self.q_bin = [torch.empty(qshape, dtype=qtype, device=dev) for _ in range(self.depth)]
            q_s1 = torch.empty((n,), dtype=torch.int64, device=dev)
            q_s2 = torch.empty((n,), dtype=torch.int64, device=dev)
            q_hist = torch.empty((n, 256), dtype=torch.int32, device=dev)
            q_cnt = torch.zeros((n, 20), dtype=torch.int32, device=dev)
        if self.resolve:
            resolve_ok = torch.empty((n,), dtype=torch.uint8, device=dev)
            out.update(resolved_digits=torch.empty((n, 81), dtype=torch.uint8, device=dev), resolve_success=resolve_ok.view(torch.bool),
                       num_conflicts=torch.empty((n,), dtype=torch.int32, device=dev), n_corrections=torch.empty((n,), dtype=torch.uint8, device=dev))
        if self.propagate:
            propagate_ok = torch.empty((n,), dtype=torch.uint8, device=dev)
            out.update(propagated_digits=torch.empty((n, 81), dtype=torch.uint8, device=dev), propagate_valid=propagate_ok.view(torch.bool),
                       contradiction_cell=torch.empty((n,), dtype=torch.uint8, device=dev), n_propagated=torch.empty((n,), dtype=torch.uint8, device=dev))
        if self.solve:
            solve_in = out["propagated_digits" if self.propagate else "resolved_digits" if self.resolve else "digits"]
            out.update(solution=torch.empty((n, 81), dtype=torch.uint8, device=dev), solve_result=torch.empty((n,), dtype=torch.int8, device=dev),
                       solve_nodes=torch.empty((n,), dtype=torch.int32, device=dev))
        if total is None:
            starts = [(s0, min(self.chunk, n - s0)) for _ in range(repeat) for s0 in range(0, n, self.chunk)]
        else:
            starts = [((k * self.chunk) % n, min(self.chunk, total - k * self.chunk)) for k in range((total + self.chunk - 1) // self.chunk)]
        pending = []                                  # (future, slot, start, m)
        free_ev = [None] * self.depth                 # classification done with slot's buffers

        def classify(item):
            fut, slot, s, m = item
            corners, found = fut.result()
            corners_all[s:s + m], found_all[s:s + m] = corners, found
            with torch.cuda.stream(self.s_cls):
                self.minv_dev[slot][:m].copy_(self.minv_pin[slot][:m], non_blocking=True)
                sub = {k: out[k][s:s + m] for k in ("logits", "digits", "conf")}
                self.ctx.frames_to_digits(frames[s:s + m], self.minv_dev[slot][:m], out=sub, glue=self.glue)
                if self.quality:
                    self.ctx.grid_line_coverage(self.q_bin[slot][:m], self.minv_dev[slot][:m], out=q_cnt[s:s + m])
                if self.resolve:
                    # two launches per chunk: top-3, then K9 with run_v2's acceptance rule (pipeline/run_v2.py:365) applied in the kernel,
                    # writing straight into run()'s outputs
                    idx, prob = self.ctx.softmax_topk(sub["logits"], 3)
                    self.ctx.resolve_conflicts(idx.view(m, 81, 3), prob.view(m, 81, 3), acceptance_rule=True,
                                               out={"digits": out["resolved_digits"][s:s + m], "success": resolve_ok[s:s + m],
                                                    "num_conflicts_after": out["num_conflicts"][s:s + m], "n_corrections": out["n_corrections"][s:s + m]})
                if self.propagate:
                    self.ctx.propagate_constraints(out["resolved_digits" if self.resolve else "digits"][s:s + m],
                                                   out={"grid": out["propagated_digits"][s:s + m], "is_valid": propagate_ok[s:s + m],
                                                        "contradiction_cell": out["contradiction_cell"][s:s + m], "n_resolved": out["n_propagated"][s:s + m]})
                lost = None
                if not found.all():
                    lost = torch.from_numpy(~found).to(dev)
                    out["digits"][s:s + m][lost] = 0
                    if self.propagate:            # no grid, nothing to propagate
                        out["propagated_digits"][s:s + m][lost] = 0
                        out["n_propagated"][s:s + m][lost] = 0
                        out["contradiction_cell"][s:s + m][lost] = 255
                        propagate_ok[s:s + m][lost] = 0
                    if self.resolve:              # no grid, no cells: nothing was validated
                        for key in ("resolved_digits", "num_conflicts", "n_corrections"):
                            out[key][s:s + m][lost] = 0
                        resolve_ok[s:s + m][lost] = 0
                if self.solve:                    # after the lost frames were cleared: their grids are empty and they are not active
                    self.ctx.solve_sudoku(solve_in[s:s + m], propagate_ok[s:s + m] if self.propagate else None if lost is None else ~lost,
                                          max_nodes=self.solve_max_nodes,
                                          out={"solution": out["solution"][s:s + m], "result": out["solve_result"][s:s + m], "nodes": out["solve_nodes"][s:s + m]})
                ev = torch.cuda.Event(blocking=True)      # the waiting thread sleeps instead of spinning: the box's CPU quota is for the search
                ev.record(self.s_cls)
                free_ev[slot] = ev

        for i, (s, m) in enumerate(starts):
            slot = i % self.depth
            if free_ev[slot] is not None:
                free_ev[slot].synchronize()
            with torch.cuda.stream(self.s_pre):
                # every buffer of a chunk belongs to its slot: an allocation in here (a 130-MB hipMalloc while the caching allocator's pool
                # grows) stalls the whole pipeline for tens of milliseconds
                if bits_direct:
                    # K1 writes the bit image itself and the speck filter works on it in place: no byte image at all
                    b = self.ctx.preprocess_bits(frames[s:s + m], out=self.dev_bits[slot][:m])
                    if self.quality:
                        self.q_bin[slot][:m].copy_(b)
                    b = self.ctx.despeckle_bits(b)
                else:
                    b = self.ctx.preprocess(frames[s:s + m], out=self.dev_bin[slot][:m])
                    if self.quality:
                        self.q_bin[slot][:m].copy_(b)
                # exact accelerator for the host search: erase the specks that cannot matter (csrc/k4_despeckle.hip), in place
                if self.packed:
                    if not bits_direct:
                        b = self.ctx.despeckle(b, out=b, packed=self.dev_bits[slot][:m])
                    if self.sparse:
                        b = self.ctx.pack_sparse_bits(b, self.dev_rec[slot])
                elif self.despeckle:
                    b = self.ctx.despeckle(b, out=b)
                ready = torch.cuda.Event()
                ready.record(self.s_pre)
                if self.quality:                  # after `ready`: the D2H copy does not wait for it
                    self.ctx.frame_quality_stats(frames[s:s + m], out=(q_s1[s:s + m], q_s2[s:s + m], q_hist[s:s + m]))
            with torch.cuda.stream(self.s_d2h):
                self.s_d2h.wait_event(ready)
                self.pinned[slot][:m].copy_(b, non_blocking=True)
                ev = torch.cuda.Event(blocking=True)      # the waiting thread sleeps instead of spinning: the box's CPU quota is for the search
                ev.record(self.s_d2h)
            pending.append((self.pool.submit(self._search, slot, m, ev), slot, s, m))
            if len(pending) > self.depth - 2:
                classify(pending.pop(0))
        while pending:
            classify(pending.pop(0))
        cur.wait_stream(self.s_cls)
        out["corners"], out["found"] = corners_all, found_all
        if self.quality:
            from .cv.grid_quality import scores_from_stats
            cur.wait_stream(self.s_pre)
            s1, s2, hist, cnt = (t.cpu().numpy() for t in (q_s1, q_s2, q_hist, q_cnt))
            out["quality"] = scores_from_stats(s1, s2, hist, cnt, corners_all, found_all, self.H * self.W).astype(np.float32)
        return out


def _corners_behind_filters(ctx, frames, binary_dev=None, min_area_ratio=0.1):
    """The corner search of one frame behind the exact filters K4 (csrc/k4_despeckle.hip) and K11 (csrc/k11_components.hip): same corners
    as host.find_grid_corners of the unfiltered binary, with one or two borders left for the host to follow instead of thousands.
    frames u8 [1,H,W,3]; binary_dev: the binary to search (u8 [H,W] on the device) when it is not K1's.  Where W % 32 == 0 the binary
    crosses to the host as H*W/8 bytes and the bit scanner reads it; otherwise as bytes.  K4 runs only where its precondition holds."""
    H, W = frames.shape[1], frames.shape[2]
    k4 = min_area_ratio * H * W > 61 * 61
    if W % 32 == 0 and H >= 16:
        if binary_dev is None:
            bits = ctx.preprocess_bits(frames)
            if k4:
                ctx.despeckle_bits(bits)
        else:
            bits = torch.empty((1, H, W // 32), dtype=torch.int32, device=ctx.device)
            if k4:
                ctx.despeckle(binary_dev[None], packed=bits)
            else:
                ctx.component_filter(binary_dev[None], 0.0, packed=bits)           # ratio 0 erases nothing: a plain pack
        ctx.component_filter_bits(bits, min_area_ratio)
        corners, found = host.find_grid_corners_bits_batch(bits.cpu().numpy(), H, W, min_area_ratio, threads=1)
        return corners[0] if found[0] else None
    b = (ctx.preprocess(frames) if binary_dev is None else binary_dev[None].contiguous())
    if k4:
        b = ctx.despeckle(b)
    b = ctx.component_filter(b, min_area_ratio, out=b if k4 or binary_dev is None else None)
    return host.find_grid_corners(b[0].cpu().numpy(), min_area_ratio)


def recognize_image(image, model_state_dict=None, ctx=None, glue=Context.GLUE_RUNPY, top_k=0, quality=False, preprocess="v1", model="v1", resolve=False, propagate=False, component_filter=False, grid="v1", solve=False, overlay=False):
    """One BGR image (numpy uint8 [H,W,3], or a CUDA uint8 tensor of that shape) -> dict(grid 9x9 list, digits, confidences, corners) or None when no
    grid is found -- the call order of pipeline/run.py:261-312, preprocess_cell (:73-95) included by default.
    top_k > 1 adds run_v2's per-cell `alternatives` (pipeline/run_v2.py:165-178): 81 lists of (digit, prob), best excluded.
    quality=True adds run_v2's quality check (pipeline/run_v2.py:299-311): `quality` (a cv.grid_quality.QualityScore) and
    `quality_feedback` (get_user_feedback); comparing quality.overall with a minimum is left to the caller, as run_v2 does.
    preprocess="v2": the binary the corner search reads is run_v2's (pipeline/run_v2.py:278-280),
    cv.preprocess_v2.preprocess_multi_strategy(image).binary, and the result carries what run_v2 prints of it (:283-284):
    `preprocess_method`, `has_shadow`, `has_glare`.  It runs on the default context of the current device.
    model="v3": the model run_v2 loads (pipeline/run_v2.py:95-128), DigitCNNv3; model_state_dict is then its state_dict and the same
    call order runs with the v3 forward.  `confidence` is softmax(logits / temperature) at the digit; the top_k alternatives come from
    softmax(logits), without the temperature, as at run_v2.py:166-180.
    model="v3_light": the same with DigitCNNv3Light (ml/model_v3.py:232-282), the reference's lighter model; model_state_dict is its state_dict.
    resolve=True (implies top_k=3 unless more are asked for; at most 4): run_v2's validation and correction stage (pipeline/run_v2.py:344-371)
    on the device: `validation` (is_valid, num_conflicts, cells_in_conflict of the cells run_v2 goes on with), `corrections` (the
    (row, col, old digit, new digit, old confidence, new confidence) taken: those of a repair that succeeded or left fewer conflicts,
    :365), `resolved_grid` and `paths_explored`.  `grid` and `digits` stay the uncorrected recognition.
    propagate=True: run_v2's constraint propagation (pipeline/run_v2.py:373-391) on the device, of `resolved_grid` when resolve=True and of
    `grid` otherwise, with the cells' confidences: `propagation` (is_valid, iterations, contradiction_cell as (row, col) or None,
    cells_resolved as (row, col, digit) in the reference's order) and `propagated_grid` (what run_v2 hands to the solver).  With
    resolve=True the confidences are run_v2's own (:374): softmax(logits) without the temperature, the repaired cells carrying their
    alternative's.  Without it -- a path run_v2 does not have -- they are `confidence`, softmax(logits / temperature) for the v3 models.
    They decide is_fixed only (confidence > 0.9), which no entry of the result shows.
    solve=True: run_v2's solver stage (pipeline/run_v2.py:393-407) on the device (Context.solve_sudoku), of `propagated_grid` when
    propagate=True (and only if the propagation was valid, as in run_v2), else of `resolved_grid`, else of `grid`: `solve_result` (1 solved,
    0 no solution, -1 invalid, 3 not attempted), `solution` (9x9; the input grid unless solved) and `solve_nodes`.  A frame that spends the
    device's node budget is finished by the unbounded host solver, so 2 is never reported.
    component_filter=True (opt-in; for photos, where the host corner search is what takes the time): the binary goes to the host behind
    the exact filters K4 and K11 (_corners_behind_filters), as a bit image where W % 32 == 0.  Same result, keys and values.
    grid="v2": the corners come from run_v2's detection (pipeline/run_v2.py:287), cv.grid_v2.detect_grid(binary, gray), which falls back
    to Hough lines, a de-rotated contour search and Harris corners + RANSAC where the contour search alone finds nothing; the result
    carries `detection_method`, `detection_confidence` and `rotation_angle`, and `corners` are the ordered float32 corners.
    component_filter does not apply to it.
    overlay=True (needs solve=True, else ValueError): `overlay`, a uint8 tensor [H,W,3] on the device: the image with the cells the
    solver filled in drawn at `corners` (Context.render_overlay with resolve/overlay.py's overlay_cells of the solver's input and
    `solution`) when solve_result is 1, otherwise an unchanged copy of the image."""
    from .runtime import default_context
    if overlay and not solve:
        raise ValueError("overlay=True needs solve=True: there is nothing to draw without a solution")
    if grid not in ("v1", "v2"):
        raise ValueError(f"grid must be 'v1' or 'v2', got {grid!r}")
    if preprocess not in ("v1", "v2"):
        raise ValueError(f"preprocess must be 'v1' or 'v2', got {preprocess!r}")
    if model not in ("v1", "v3", "v3_light"):
        raise ValueError(f"model must be 'v1', 'v3' or 'v3_light', got {model!r}")
    ctx = ctx or default_context()
    load, forward = {"v1": (ctx.load_state_dict, ctx.frames_to_digits), "v3": (ctx.load_state_dict_v3, ctx.frames_to_digits_v3),
                     "v3_light": (ctx.load_state_dict_v3_light, ctx.frames_to_digits_v3_light)}[model]
    if model_state_dict is not None:
        load(model_state_dict)
    if isinstance(image, torch.Tensor):             # already in HBM (imgcodecs.imread(..., device=True))
        frames = image.contiguous()[None]
    else:
        frames = torch.from_numpy(np.ascontiguousarray(image)).to(ctx.device)[None]
    pre = None
    if preprocess == "v2":
        from .cv import preprocess_v2
        pre = preprocess_v2.preprocess_multi_strategy(frames[0])
        binary_dev = pre.binary
    else:
        binary_dev = None if component_filter and grid == "v1" else ctx.preprocess(frames)[0]
    detection = None
    if grid == "v2":
        from .cv import grid_v2
        detection = grid_v2.detect_grid(binary_dev, ctx.gray(frames)[0])
        corners = detection.corners
    elif component_filter:
        corners = _corners_behind_filters(ctx, frames, binary_dev)
    else:
        binary = binary_dev.cpu().numpy()
        corners = host.find_grid_corners(binary)
    if corners is None:
        return None
    minv = ctx.minv_to_device(Context.corners_to_minv(corners[None].astype(np.float32)))
    out = forward(frames, minv, glue=glue)
    digits = out["digits"][0].cpu().numpy()
    res = {"grid": [[int(digits[r * 9 + c]) for c in range(9)] for r in range(9)], "digits": digits,
           "confidence": out["conf"][0].cpu().numpy(), "logits": out["logits"][0].cpu().numpy(), "corners": corners}
    if resolve:
        top_k = max(top_k, 3)
    if top_k > 1:
        idx, prob = ctx.softmax_topk(out["logits"][0], top_k)
        if resolve:
            res.update(_validate_and_resolve(ctx, idx[None], prob[None]))
            resolved = res.pop("_cells")
        idx, prob = idx.cpu().numpy(), prob.cpu().numpy()
        res["alternatives"] = [[(int(idx[i, j]), float(prob[i, j])) for j in range(1, top_k)] for i in range(81)]
    if propagate:
        cells, conf = resolved if resolve else (out["digits"], out["conf"])
        prop_dev = ctx.propagate_constraints(cells, conf)
        state = {k: v[0].cpu().numpy() for k, v in prop_dev.items()}
        bad, g = int(state["contradiction_cell"]), state["grid"]
        res["propagation"] = {"is_valid": bool(state["is_valid"]), "iterations": int(state["iterations"]),
                              "contradiction_cell": None if bad == 255 else (bad // 9, bad % 9),
                              "cells_resolved": [(int(x) // 9, int(x) % 9, int(v)) for x, v in state["resolved"][:int(state["n_resolved"])]]}
        res["propagated_grid"] = [[int(g[r * 9 + c]) for c in range(9)] for r in range(9)]
    if solve:
        if propagate:
            given, active = prop_dev["grid"], prop_dev["is_valid"]
        else:
            given, active = (resolved[0] if resolve else out["digits"]), None
        solved = ctx.solve_sudoku(given, active)
        code, sol, nodes = (solved[k][0].cpu().numpy() for k in ("result", "solution", "nodes"))
        if int(code) == Context.SOLVE_BUDGET:                 # the device's budget is spent: the host finishes the frame, without one
            codes, sols, counts = host.solve_sudoku_batch(given.cpu().numpy(), threads=1)
            code, sol, nodes = codes[0], sols[0].reshape(81), counts[0]
        res["solve_result"], res["solve_nodes"] = int(code), int(nodes)
        res["solution"] = [[int(sol[r * 9 + c]) for c in range(9)] for r in range(9)]
        if overlay:
            res["overlay"] = _draw_solution(ctx, frames, corners, given[0].cpu().numpy(), sol, int(code) == 1)[0]
    if quality:
        from .cv import grid_quality
        if binary_dev is None:                                # component_filter=True never made the byte image
            binary_dev = ctx.preprocess(frames)[0]
        q = grid_quality.assess_grid_quality(frames[0], binary_dev, corners, ctx=ctx)
        res["quality"], res["quality_feedback"] = q, grid_quality.get_user_feedback(q)
    if pre is not None:
        res["preprocess_method"], res["has_shadow"], res["has_glare"] = pre.method_used, pre.has_shadow, pre.has_glare
    if detection is not None:
        res["detection_method"], res["detection_confidence"], res["rotation_angle"] = detection.method, detection.confidence, detection.rotation_angle
    return res


def _encode_frame_out(ctx, res, encode):
    """recognize_stream's encode: True -> res["jpeg"], "png" -> res["png"]"""
    if encode == "png":
        res["png"] = ctx.imencode_png(res["frame_out"])
    else:
        res["jpeg"] = ctx.imencode(res["frame_out"])


def recognize_stream(frames, model_state_dict=None, ctx=None, glue=Context.GLUE_RUNPY, preprocess="v1", grid="v1", stabilizer=None, motion_detector=None, overlay=False, solve_max_nodes=4096, encode=False):
    """A camera feed: the loop of cv/stabilizer.py:308-335 followed by this library's recognition.  frames: an iterable of BGR frames
    (numpy uint8 [H,W,3] or CUDA uint8 tensors).  A generator; per frame it yields a dict:
        motion        the motion gate's verdict (cv.stabilizer.MotionDetector.update); True: the frame is skipped, every other entry
                      but `motion` is None / False, and the stabiliser does not see it
        detected      a grid was found in this frame
        stabilized    the StabilizedResult of cv.stabilizer.GridStabilizer.update(corners or None)
        corners_used  the stabilised corners K2 warped with, float32 [4,2]; None when there are none or they define no homography
        digits, confidence   the 81 digits and their confidences read at corners_used, else None
    overlay=True adds three entries: the recognised digits go to the solver (Context.solve_sudoku with solve_max_nodes; the host
    finishes a frame that spends the budget, as in recognize_image), and
        solution, solve_result   the 81 solved digits (the recognised ones unless solve_result is 1) and the solver's verdict, else None
        frame_out     a uint8 tensor [H,W,3] on the device: the frame with the cells the solver filled in drawn at corners_used
                      (Context.render_overlay) where solve_result is 1; the input frame itself for a skipped or unsolved frame
    encode=True (needs overlay=True, else ValueError) adds
        jpeg          the bytes of frame_out as a JPEG file (Context.imencode: quality 95, 4:2:0, cv2.imwrite's defaults)
    encode="png" (needs overlay=True too) adds instead
        png           the bytes of frame_out as a PNG file (Context.imencode_png: Sub filter, Z_RLE, cv2.imwrite's defaults)
    preprocess, grid: "v1" | "v2" as in recognize_image (grid="v1": K1's binary and the host contour search; "v2":
    cv.grid_v2.detect_grid).  stabilizer, motion_detector: the GridStabilizer / MotionDetector to use (default: new ones with the
    reference's defaults).  With the default use_kalman=True the stabilised corners of the first min_detections - 1 detections are
    exact zeros (cv/stabilizer.py), which define no homography: those frames yield digits=None.  FramePipeline is the tool for independent
    frames; this is for one feed, frame by frame."""
    from .runtime import default_context
    from .cv import stabilizer as stab
    if grid not in ("v1", "v2"):
        raise ValueError(f"grid must be 'v1' or 'v2', got {grid!r}")
    if preprocess not in ("v1", "v2"):
        raise ValueError(f"preprocess must be 'v1' or 'v2', got {preprocess!r}")
    if encode and not overlay:
        raise ValueError("encode=True needs overlay=True: frame_out is what gets encoded")
    ctx = ctx or default_context()
    if model_state_dict is not None:
        ctx.load_state_dict(model_state_dict)
    stabilizer = stabilizer or stab.GridStabilizer()
    motion_detector = motion_detector or stab.MotionDetector()
    if motion_detector.ctx is None:
        motion_detector.ctx = ctx
    for image in frames:
        if isinstance(image, torch.Tensor):
            frame = image.contiguous()[None]
        else:
            frame = torch.from_numpy(np.ascontiguousarray(image)).to(ctx.device)[None]
        res = {"motion": motion_detector.update(frame[0]), "detected": False, "stabilized": None, "corners_used": None, "digits": None,
               "confidence": None}
        if overlay:
            res.update(solution=None, solve_result=None, frame_out=frame[0])
        if res["motion"]:
            if encode:
                _encode_frame_out(ctx, res, encode)
            yield res
            continue
        if preprocess == "v2":
            from .cv import preprocess_v2
            binary_dev = preprocess_v2.preprocess_multi_strategy(frame[0]).binary
        else:
            binary_dev = ctx.preprocess(frame)[0]
        if grid == "v2":
            from .cv import grid_v2
            corners = grid_v2.detect_grid(binary_dev, ctx.gray(frame)[0]).corners
        else:
            corners = host.find_grid_corners(binary_dev.cpu().numpy())
        res["detected"] = corners is not None
        res["stabilized"] = s = stabilizer.update(None if corners is None else np.asarray(corners, np.float32))
        if s.corners is not None:
            used = np.asarray(s.corners, np.float32)
            minv, ok = Context.corners_to_minv_batch(used[None])
            if ok[0]:
                out = ctx.frames_to_digits(frame, ctx.minv_to_device(minv), glue=glue)
                res["corners_used"], res["digits"], res["confidence"] = used, out["digits"][0].cpu().numpy(), out["conf"][0].cpu().numpy()
                if overlay:
                    solved = ctx.solve_sudoku(out["digits"], max_nodes=solve_max_nodes)
                    code, sol = int(solved["result"][0]), solved["solution"][0].cpu().numpy()
                    if code == Context.SOLVE_BUDGET:
                        codes, sols, _ = host.solve_sudoku_batch(res["digits"][None], threads=1)
                        code, sol = int(codes[0]), sols[0].reshape(81)
                    res["solution"], res["solve_result"] = sol, code
                    if code == 1:
                        res["frame_out"] = _draw_solution(ctx, frame, used, res["digits"], sol, True)[0]
        if encode:
            _encode_frame_out(ctx, res, encode)
        yield res


def _draw_solution(ctx, frame, corners, given, solution, solved):
    """frame u8 [1,H,W,3] on the device -> a new [1,H,W,3]: the cells of `solution` that `given` leaves empty drawn at `corners`
    (the iOS rule, resolve/overlay.py overlay_cells) when `solved`, else an unchanged copy."""
    m, ok = Context.corners_to_m_batch(np.asarray(corners, np.float32).reshape(1, 4, 2))
    given, solution = np.asarray(given, np.uint8).reshape(81), np.asarray(solution, np.uint8).reshape(81)
    digits = np.where(given != 0, 0, solution).astype(np.uint8)
    active = torch.tensor([bool(solved) and bool(ok[0])], dtype=torch.bool, device=ctx.device)
    return ctx.render_overlay(frame, ctx.minv_to_device(m), torch.from_numpy(digits[None]).to(ctx.device), active=active)


def _validate_and_resolve(ctx, idx, prob):
    """pipeline/run_v2.py:347-371 on one frame's top-k (device tensors [1,81,k]): validate; if invalid, search; take the search's cells
    if it succeeded or left fewer conflicts -- one launch, with the acceptance rule applied in the kernel."""
    dev = ctx.resolve_conflicts(idx, prob, acceptance_rule=True)
    state = {k: v[0].cpu().numpy() for k, v in dev.items()}
    corrections = [(int(x) // 9, int(x) % 9, int(old), int(new), float(c0), float(c1))
                   for (x, old, new), (c0, c1) in zip(state["corr_cells"][:int(state["n_corrections"])], state["corr_conf"])]
    digits, count = state["digits"], state["conflict_count"]
    return {"validation": {"is_valid": int(state["num_conflicts_after"]) == 0, "num_conflicts": int(state["num_conflicts_after"]),
                           "cells_in_conflict": [(x // 9, x % 9) for x in range(81) if count[x]]},
            "corrections": corrections, "resolved_grid": [[int(digits[r * 9 + c]) for c in range(9)] for r in range(9)],
            "paths_explored": int(state["paths_explored"]), "_cells": (dev["digits"], dev["conf"])}


def run_solver(grid):
    """The reference's run_solver (pipeline/run.py:163-202) without the subprocess: -> (success, solution) with
    solution == grid when the puzzle is invalid or has no solution."""
    code, sol = host.solve_sudoku(grid)
    g = [[int(v) for v in row] for row in np.asarray(grid).reshape(9, 9)]
    return (True, [[int(v) for v in row] for row in sol]) if code == 1 else (False, g)


# ---- the harness's own entry point (pipeline/run.py:36-70, 205-241, 244-355), same result fields and error strings ------------------
@dataclass
class CellPrediction:
    """pipeline/run.py:36-43"""
    row: int
    col: int
    digit: int                      # 0 = empty, 1-9 = digit
    confidence: float
    is_original: bool = True        # True if read from the image, False if filled in by the solver


@dataclass
class PipelineResult:
    """pipeline/run.py:46-66 (same fields; times in seconds)"""
    success: bool
    error: str = None
    time_cv: float = 0.0
    time_ml: float = 0.0
    time_solver: float = 0.0
    time_total: float = 0.0
    original_image: np.ndarray = None
    warped_grid: np.ndarray = None
    cells: list = field(default_factory=list)
    predictions: list = field(default_factory=list)
    recognized_grid: list = field(default_factory=list)
    solution: list = field(default_factory=list)
    low_confidence_cells: list = field(default_factory=list)
    constraint_violations: list = field(default_factory=list)


def check_constraints(grid):
    """The messages of pipeline/run.py:205-241 for a 9x9 grid: one entry per repeated value in a row, a column or a box
    (0 = empty is ignored); a value seen three times in a unit yields two entries, each naming the previous occurrence."""
    out = []
    units = [("row", r, [(r, c) for c in range(9)]) for r in range(9)]
    units += [("col", c, [(r, c) for r in range(9)]) for c in range(9)]
    units += [("box", b, [(3 * (b // 3) + i, 3 * (b % 3) + j) for i in range(3) for j in range(3)]) for b in range(9)]
    for kind, idx, members in units:
        last = {}
        for r, c in members:
            v = grid[r][c]
            if v <= 0:
                continue
            if v in last:
                pr, pc = last[v]
                if kind == "row":
                    out.append(f"Row {idx + 1}: duplicate {v} at columns {pc + 1} and {c + 1}")
                elif kind == "col":
                    out.append(f"Column {idx + 1}: duplicate {v} at rows {pr + 1} and {r + 1}")
                else:
                    out.append(f"Box ({idx // 3 + 1},{idx % 3 + 1}): duplicate {v}")
            last[v] = (r, c)
    return out


def run_pipeline(image_path, state_dict=None, ctx=None, debug=False, low_confidence=0.7, component_filter=False, reduce=1, grid="v1", output=None):
    """run_pipeline(image_path) of pipeline/run.py:244-355 on the MI355X path: JPEG -> frame in HBM (imgcodecs) -> K1 -> host
    corner search -> K2 (warped 450x450 grid kept, as the reference keeps it) -> preprocess_cell + DigitCNN (K3) -> constraint
    check -> in-process solver.  Same PipelineResult fields, same error strings, same partial results on failure.
    component_filter=True: the corner search reads the binary behind the exact filters K4 and K11 (recognize_image); same result.
    reduce = 2, 4 or 8: the JPEG is decoded at 1/reduce of its size (cv2.IMREAD_REDUCED_COLOR_*) and everything downstream runs on that frame.
    grid="v2": the corners come from cv.grid_v2.detect_grid (recognize_image); the result then has the attributes detection_method,
    detection_confidence and rotation_angle (run_v2's PipelineResult fields).
    output: a .jpg path; when the puzzle is solved, the frame with the solution drawn in (Context.render_overlay) is written there by
    imgcodecs.imwrite, as run.py's --output does (pipeline/run.py:419-432); the result then has the attribute output_written.  Like every
    other stage, writing reports and does not raise: a path that is not a .jpg, or one that cannot be written, leaves output_written False and
    "Output failed: ..." in error, with the solved result otherwise intact."""
    from . import imgcodecs
    from .runtime import default_context
    if grid not in ("v1", "v2"):
        raise ValueError(f"grid must be 'v1' or 'v2', got {grid!r}")
    res = PipelineResult(success=False)
    t_total = time.time()
    ctx = ctx or default_context()
    if state_dict is not None:
        ctx.load_state_dict(state_dict)
    frame = imgcodecs.imread(image_path, device=True, ctx=ctx, reduce=reduce)
    if frame is None:
        res.error = f"Failed to load image: {image_path}"
        return res
    res.original_image = frame.cpu().numpy()

    t_cv = time.time()
    try:
        if component_filter and grid == "v1":
            filtered = _corners_behind_filters(ctx, frame[None])
        else:
            binary = ctx.preprocess(frame[None])[0].cpu().numpy()
    except Exception as e:                                   # noqa: BLE001 -- the reference reports, it does not raise
        res.error = f"Preprocessing failed: {e}"
        return res
    try:
        if grid == "v2":
            from .cv import grid_v2
            detection = grid_v2.detect_grid(binary, ctx.gray(frame[None])[0])
            corners = detection.corners
            res.detection_method, res.detection_confidence, res.rotation_angle = detection.method, detection.confidence, detection.rotation_angle
        else:
            corners = filtered if component_filter else host.find_grid_corners(binary)
        if corners is None:
            res.error = "Grid detection failed: no quadrilateral found"
            return res
    except Exception as e:                                   # noqa: BLE001
        res.error = f"Grid detection failed: {e}"
        return res
    try:
        minv = ctx.minv_to_device(Context.corners_to_minv(corners[None].astype(np.float32)))
        warped = ctx.warp_perspective(frame, minv[0], 450)
        res.warped_grid = warped.cpu().numpy()
    except Exception as e:                                   # noqa: BLE001
        res.error = f"Perspective warp failed: {e}"
        return res
    try:
        cells = ctx.extract_cells(warped, 28, 5, 5)          # cv/extract.py:13-56 defaults: 50-px cells, 10 % margin
        res.cells = list(cells.cpu().numpy())
        if len(res.cells) != 81:
            res.error = f"Cell extraction failed: expected 81 cells, got {len(res.cells)}"
            return res
    except Exception as e:                                   # noqa: BLE001
        res.error = f"Cell extraction failed: {e}"
        return res
    res.time_cv = time.time() - t_cv

    t_ml = time.time()
    try:
        logits, digits, conf = ctx.cnn_forward(cells, want_digits=True, glue=Context.GLUE_RUNPY)
        digits, conf = digits.cpu().numpy(), conf.cpu().numpy()
        res.predictions = [CellPrediction(row=i // 9, col=i % 9, digit=int(digits[i]), confidence=float(conf[i])) for i in range(81)]
        grid = [[int(digits[r * 9 + c]) for c in range(9)] for r in range(9)]
        res.recognized_grid = grid
        res.low_confidence_cells = [(p.row, p.col, p.confidence) for p in res.predictions if p.digit > 0 and p.confidence < low_confidence]
    except Exception as e:                                   # noqa: BLE001
        res.error = f"ML inference failed: {e}"
        return res
    res.time_ml = time.time() - t_ml

    res.constraint_violations = check_constraints(grid)
    if res.constraint_violations and debug:
        print(f"Warning: {len(res.constraint_violations)} constraint violations detected")
        for v in res.constraint_violations[:5]:
            print(f"  - {v}")

    t_solver = time.time()
    try:
        ok, solution = run_solver(grid)
        if ok:
            res.solution = solution
            for p in res.predictions:
                if p.digit == 0:
                    p.digit = solution[p.row][p.col]
                    p.is_original = False
        else:
            res.error = "Solver failed: puzzle may be invalid or have recognition errors"
            res.solution = grid                              # the reference still returns the partial result
    except Exception as e:                                   # noqa: BLE001
        res.error = f"Solver error: {e}"
        return res
    res.time_solver = time.time() - t_solver
    if ok and output is not None:
        try:
            drawn = _draw_solution(ctx, frame[None], corners, digits, np.asarray(solution, np.uint8).reshape(81), True)[0]
            res.output_written = imgcodecs.imwrite(output, drawn, ctx=ctx)
            if not res.output_written:
                res.error = f"Output failed: cannot write {output}"
        except Exception as e:                               # noqa: BLE001
            res.output_written = False
            res.error = f"Output failed: {e}"
    res.time_total = time.time() - t_total
    res.success = ok
    return res
