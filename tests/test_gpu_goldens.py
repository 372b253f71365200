"""GPU (-m gpu): the HIP path against COMMITTED golden values (tests/golden/cv_goldens.json, photo_goldens.npz) -- not only
against the live oracle --, all five data/test_images photos end to end, BASELINE configs[2] (hipGraph capture / replay) and the
multi-rank bench entry rehearsed on one GPU.  Same parity caveat as tests/test_cv_goldens.py: the CV goldens come from a
restatement of OpenCV (cv2 is not in the image)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import cnn_oracle
import sv_oracle as o

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
G = json.load(open(os.path.join(GOLDEN, "cv_goldens.json")))
LOGIT_TOL = 1e-4


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _trained(golden_dir):
    g2 = np.load(os.path.join(golden_dir, "cnn_coreml_fp16.npz"))
    return {k: torch.from_numpy(g2[k.replace(".", "_")].astype(np.float32)) for k in cnn_oracle.KEYS}


@pytest.mark.parametrize("rec", G["synthetic"], ids=lambda r: f"{r['H']}x{r['W']}-s{r['seed']}-{r['index']}")
def test_synthetic_goldens(ctx, rec):
    """K1 binary, homography bytes and K2 cells of seeded frames: SHA-256 equal to the committed values."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import synth_frames
    frames, corners, _ = synth_frames(rec["n"], rec["H"], rec["W"], seed=rec["seed"], noise="int")      # on the CPU: bit-stable
    i = rec["index"]
    assert sha(frames[i].numpy()) == rec["frame_sha256"]
    d = frames[i:i + 1].cuda()
    binary = ctx.preprocess(d)[0].cpu().numpy()
    assert sha(binary) == rec["binary_sha256"]
    minv = sva.Context.corners_to_minv(corners[i:i + 1])
    assert sha(minv[0]) == rec["minv_sha256"]
    cells = ctx.warp_cells(d, ctx.minv_to_device(minv))[0].cpu().numpy()
    assert sha(cells) == rec["cells_sha256"]
    got = sva.host.find_grid_corners(binary)
    assert (None if got is None else got.tolist()) == rec["found_corners"]


@pytest.mark.parametrize("rec", G["photos"], ids=lambda r: r["file"])
def test_all_reference_photos_end_to_end(ctx, golden_dir, rec):
    """data/test_images/sample_{1..5}.jpg (north_star: "bit-exact digit-index parity on data/test_images"; the reference's note
    "CV success rate on test images: 4/5", tests/test_integration.py:261).  Per photo, everything on the product path:
    GPU JPEG decode (= the PIL-decoded frame the goldens were made from), K1 binary SHA-256, host corner search, K2 cells,
    run.py glue + DigitCNN with the trained weights: digits equal, logits <= 1e-4.  The photo without a grid goes through the
    `None` path: find_grid_contour -> None, run_pipeline -> "Grid detection failed: no quadrilateral found" (cv/grid.py:51-52,71;
    pipeline/run.py:268-272)."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import imgcodecs
    from sudoku_vision_amd.pipeline import recognize_image, run_pipeline
    path = os.path.join(golden_dir, rec["file"])
    sd = _trained(golden_dir)
    ctx.load_state_dict(sd)
    frame = imgcodecs.imread(path, device=True, ctx=ctx)
    assert list(frame.shape) == rec["shape"] and sha(frame.cpu().numpy()) == rec["frame_sha256"]
    binary = ctx.preprocess(frame[None])[0].cpu().numpy()
    assert sha(binary) == rec["binary_sha256"]
    corners = sva.host.find_grid_corners(binary)
    assert (None if corners is None else corners.tolist()) == rec["corners"]
    res = run_pipeline(path, ctx=ctx)
    if rec["corners"] is None:
        assert recognize_image(frame, ctx=ctx) is None
        assert not res.success and res.error == "Grid detection failed: no quadrilateral found"
        assert res.warped_grid is None and res.cells == [] and res.predictions == []
        return
    P = np.load(os.path.join(golden_dir, "photo_goldens.npz"))
    key = rec["file"].split(".")[0]
    minv = sva.Context.corners_to_minv(corners[None].astype(np.float32))
    assert sha(minv[0]) == rec["minv_sha256"]
    cells = ctx.warp_cells(frame[None], ctx.minv_to_device(minv))[0].cpu().numpy()
    assert sha(cells) == rec["cells_sha256"] and (cells == P[key + "_cells"]).all()
    out = recognize_image(frame, ctx=ctx)                                  # run.py order incl. preprocess_cell
    assert (out["digits"] == P[key + "_digits"]).all()
    assert np.abs(out["logits"] - P[key + "_logits"]).max() <= LOGIT_TOL
    assert (np.stack(res.cells) == P[key + "_cells"]).all()                # run_pipeline: warp 450x450 then extract_cells = the fused K2
    assert [p.digit if p.is_original else 0 for p in res.predictions] == P[key + "_digits"].tolist()
    assert res.recognized_grid == [[int(P[key + "_digits"][r * 9 + c]) for c in range(9)] for r in range(9)]
    # the batched pipeline on the same photo (portrait photos are 2736 wide: not a multiple of 32, so the byte image + byte search path;
    # landscape ones take the bit-image path): same corners, same digits
    from sudoku_vision_amd.pipeline import FramePipeline
    H, W = frame.shape[0], frame.shape[1]
    pipe = FramePipeline(ctx, H, W, chunk=1, host_threads=2, glue=ctx.GLUE_RUNPY)
    assert pipe.packed == (W % 32 == 0)
    pres = pipe.run(frame[None].contiguous())
    torch.cuda.synchronize()
    assert pres["found"].tolist() == [True] and (pres["corners"][0] == corners).all()
    assert (pres["digits"][0].cpu().numpy() == P[key + "_digits"]).all()


def test_hipgraph_capture_replay_configs2(ctx, golden_dir):
    """BASELINE configs[2]: the per-frame path with its two device segments captured in hipGraphs exactly as bench_latency.py
    does (segment 1: K1 -> despeckle -> bit-packed binary; segment 2: K2 -> K3), call order of pipeline/run.py:261-302.
    Replayed on four different frames: K1 binary and cells bit-exact, logits <= 1e-4, digits equal to the oracle's; the host search
    on the despeckled bits finds what the oracle's search finds on the raw binary.  Capture itself proves the library makes no
    hipMalloc / synchronising call once sv_ctx_reserve has sized the scratch (either would abort the capture); device memory in
    use does not change across replays."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import synth_frames
    H, W = 1080, 1920
    pool, _, _ = synth_frames(4, H, W, seed=77, device="cuda")
    pool[3] = 200                                                          # a frame without a grid
    host_pool = [pool[i].cpu().pin_memory() for i in range(4)]
    sd = _trained(golden_dir)
    ctx.load_state_dict(sd)
    ctx.reserve(81)
    frame_d = torch.empty((1, H, W, 3), dtype=torch.uint8, device="cuda")
    k1_d = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
    scratch_d = torch.empty((1, H, W), dtype=torch.uint8, device="cuda")
    bits_d = torch.empty((1, H, W // 32), dtype=torch.int32, device="cuda")
    bits_h = torch.empty((1, H, W // 32), dtype=torch.int32).pin_memory()
    minv_h = torch.empty((1, 9), dtype=torch.float64).pin_memory()
    minv_d = torch.zeros((1, 9), dtype=torch.float64, device="cuda")
    minv_d[0, 0] = minv_d[0, 4] = minv_d[0, 8] = 1
    out = {"logits": torch.empty((1, 81, 10), device="cuda"), "digits": torch.empty((1, 81), dtype=torch.uint8, device="cuda"),
           "conf": torch.empty((1, 81), device="cuda"), "cells": torch.empty((1, 81, 28, 28), dtype=torch.uint8, device="cuda")}
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        frame_d[0].copy_(host_pool[0], non_blocking=True)
        ctx.despeckle(ctx.preprocess(frame_d, out=k1_d), out=scratch_d, packed=bits_d)       # warm-up outside capture
        ctx.frames_to_digits(frame_d, minv_d, out=out, glue=ctx.GLUE_RUNPY)
        stream.synchronize()
        g1 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, stream=stream):
            ctx.despeckle(ctx.preprocess(frame_d, out=k1_d), out=scratch_d, packed=bits_d)
        g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g2, stream=stream):
            ctx.frames_to_digits(frame_d, minv_d, out=out, glue=ctx.GLUE_RUNPY)
        # segment 1 as bench_latency.py runs it since round 2: K1 writes the bit image, the speck filter works on it in place
        bits2_d, bits2_h = torch.empty_like(bits_d), torch.empty_like(bits_h).pin_memory()
        ctx.despeckle_bits(ctx.preprocess_bits(frame_d, out=bits2_d))
        stream.synchronize()
        g1b = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1b, stream=stream):
            ctx.despeckle_bits(ctx.preprocess_bits(frame_d, out=bits2_d))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    found = 0
    for i in (0, 1, 2, 3, 1):
        with torch.cuda.stream(stream):
            frame_d[0].copy_(host_pool[i], non_blocking=True)
            g1.replay()
            g1b.replay()
            bits_h.copy_(bits_d, non_blocking=True)
            bits2_h.copy_(bits2_d, non_blocking=True)
            stream.synchronize()
            assert np.array_equal(bits2_h.numpy(), bits_h.numpy())
            cc, ff = sva.host.find_grid_corners_bits_batch(bits_h.numpy(), H, W, threads=1)
            img = host_pool[i].numpy()
            binary = o.preprocess_for_grid_detection(img)
            assert (k1_d[0].cpu().numpy() == binary).all()
            want = o.find_grid_contour(binary)
            assert bool(ff[0]) == (want is not None)
            if want is None:
                continue
            assert (cc[0] == np.asarray(want).reshape(4, 2)).all()
            found += 1
            minv_h.copy_(torch.from_numpy(sva.Context.corners_to_minv(cc[:1].astype(np.float32)).reshape(1, 9)))
            minv_d.copy_(minv_h, non_blocking=True)
            g2.replay()
            stream.synchronize()
        cells = o.warp_cells(img, cc[0].astype(np.float32))
        assert (out["cells"][0].cpu().numpy() == cells).all()
        el, ed, _ = cnn_oracle.predict(sd, o.cells_to_input(o.preprocess_cells(cells))[:, None])
        assert np.abs(out["logits"][0].cpu().numpy() - el.numpy()).max() <= LOGIT_TOL
        assert (out["digits"][0].cpu().numpy() == ed.numpy()).all()
    assert found == 4
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] == free0                           # replays allocate nothing (library scratch included)


def _adversarial_binaries(H, W):
    """{0,255} images built to break a component filter: a ring (area above the floor) with an island in its hole, a spiral inside one tile, a
    spiral across many tiles, a large square touching the frame edges, a thin diagonal whose bounding box is above the area floor but whose
    area is far below it, a quadrilateral just above the floor next to one just below it, everything buried in speck noise."""
    rs = np.random.RandomState(H + W)
    out = []
    noise = (rs.uniform(size=(H, W)) < 0.004)
    base = np.zeros((H, W), bool)
    yy, xx = np.mgrid[:H, :W]
    a = base.copy()                                                         # ring + island
    a[H // 8:H - H // 8, W // 8:W - W // 8] = True
    a[H // 8 + 6:H - H // 8 - 6, W // 8 + 6:W - W // 8 - 6] = False
    a[H // 2 - 20:H // 2 + 20, W // 2 - 20:W // 2 + 20] = True
    out.append(a | noise)
    b = base.copy()                                                         # small spiral inside one 64x64 tile + a long spiral across tiles
    for k in range(1, 14):
        b[70 + 2 * k, 70 + 2 * k:130 - 2 * k] = True
        b[70 + 2 * k:130 - 2 * k, 129 - 2 * k] = True
    for k in range(0, min(H, W) // 2 - 40, 12):
        b[20 + k, 150 + k:W - 20 - k] = True
        b[20 + k:H - 20 - k, W - 21 - k] = True
        b[H - 21 - k, 150 + k + 12:W - 20 - k] = True
        b[20 + k + 12:H - 20 - k, 150 + k + 12] = True
    out.append(b | noise)
    c = base.copy()                                                         # a block touching the top and left frame edges, a second one the bottom right corner
    c[0:H // 2, 0:W // 2] = True
    c[H - H // 3:, W - W // 3:] = True
    out.append(c | noise)
    d = base.copy()                                                         # 3-px diagonal: bounding box ~ the whole frame, area tiny; plus a real quad
    d[(abs(yy * W - xx * H) < 2 * max(H, W))] = True
    d[H // 3:H // 3 + H // 3, W // 2 + 10:W // 2 + 10 + W // 3] = True
    d[H // 3 + 4:H // 3 + H // 3 - 4, W // 2 + 14:W // 2 + 6 + W // 3] = False
    out.append(d | noise)
    e = base.copy()                                                         # two squares whose areas straddle 2 % of the frame
    s_hi, s_lo = int(np.sqrt(0.02 * H * W)) + 3, int(np.sqrt(0.02 * H * W)) - 3
    e[40:40 + s_hi, 40:40 + s_hi] = True
    e[40 + 3:40 + s_hi - 3, 40 + 3:40 + s_hi - 3] = False
    e[H - 40 - s_lo:H - 40, W - 40 - s_lo:W - 40] = True
    out.append(e | noise)
    out.append(noise | (rs.uniform(size=(H, W)) < 0.02))                    # no grid at all
    return [(x * 255).astype(np.uint8) for x in out]


@pytest.mark.parametrize("H,W", [(1080, 1920), (540, 960)])
def test_filtered_search_equals_unfiltered(ctx, H, W):
    """the corner search behind the GPU component filter (sv_despeckle_bits, in every hand-over form: byte image, bit image,
    sparse records) returns exactly what the unfiltered search (cv/grid.py:37-71 on the raw binary) returns -- the same corners or None --
    on adversarial images and on the synthetic golden frames, for min_area_ratio 0.1 (the reference's default) and 0.02.  The filter's
    precondition (include/sudoku_vision_hip.h, sv_despeckle_u8): min_area_ratio * H * W > 61 * 61; both shapes and ratios satisfy it."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import synth_frames
    imgs = _adversarial_binaries(H, W)
    frames = synth_frames(3, H, W, seed=9, noise="int")[0].cuda()
    imgs += list(ctx.preprocess(frames).cpu().numpy())
    d = torch.from_numpy(np.stack(imgs)).cuda()
    n = len(imgs)
    filt = ctx.despeckle(d)
    bits = torch.empty((n, H, W // 32), dtype=torch.int32, device="cuda")
    ctx.despeckle(d, out=torch.empty_like(d), packed=bits)
    cap = H * (W // 32) // 2
    stride = sva.host.sparse_bits_record_bytes(H, W, cap)
    recs = ctx.pack_sparse_bits(bits, torch.empty((n, stride), dtype=torch.uint8, device="cuda")).cpu().numpy()
    fnp, bnp = filt.cpu().numpy(), bits.cpu().numpy()
    some_found = 0
    for ratio in (0.1, 0.02):
        assert ratio * H * W > 61 * 61
        cb, fb = sva.host.find_grid_corners_bits_batch(bnp, H, W, ratio, 0.02, 2)
        cs, fs = sva.host.find_grid_corners_sparse_batch(recs, H, W, ratio, 0.02, 2)
        for i in range(n):
            want = sva.host.find_grid_corners(imgs[i], ratio)                # the unfiltered search on the raw binary
            got_bytes = sva.host.find_grid_corners(fnp[i], ratio)
            assert (want is None) == (got_bytes is None) and (want is None or (want == got_bytes).all()), (i, ratio)
            assert bool(fb[i]) == (want is not None) and (want is None or (cb[i] == want).all()), (i, ratio)
            assert fs[i] in (0, 1) and bool(fs[i]) == (want is not None) and (want is None or (cs[i] == want).all()), (i, ratio)
            some_found += want is not None
    assert some_found >= 8                                                   # the cases are not all trivially "None"


def _bench(args, env=None, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=dict(os.environ, **(env or {})),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_bench_starts_its_own_ranks(ctx):
    """`python bench.py --gpus 2` with no outer launcher: two ranks (both on cuda:0 under SV_BENCH_REHEARSE=1), n_gpus = 2 in
    the line, weak scaling counts both ranks' frames, `ranks` names each rank's GPU; configs[3]'s round-robin workload at a small total."""
    res = _bench(["--full", "--gpus", "2", "--frames", "32", "--steps", "3", "--warmup", "1", "--no-e2e", "--no-cpu-baseline"],
                 env={"SV_BENCH_REHEARSE": "1"})
    assert res["n_gpus"] == 2 and res["steps"] == 3 and res["scaling"] == "weak" and res["value_kind"] == "device_only"
    assert res["config"]["frames_per_step"] == 64
    assert abs(res["value"] - 64 * 3 / (res["ms_per_step"] * 3e-3)) <= 1e-6 * res["value"]
    assert 0 < res["roofline"]["frac"] <= 1.0
    assert [r["rank"] for r in res["ranks"]] == [0, 1] and len({r["pid"] for r in res["ranks"]}) == 2
    assert all(r["pci_bus_id"] and r["device"] for r in res["ranks"])
    res3 = _bench(["--full", "--gpus", "2", "--workload", "configs3", "--total-frames", "301", "--frames", "32", "--steps", "2", "--warmup", "1"],
                  env={"SV_BENCH_REHEARSE": "1"})
    assert res3["n_gpus"] == 2 and res3["scaling"] == "strong" and res3["config"]["frames_per_step"] == 301
    assert res3["config"]["frames_per_gpu"] == 151                        # rank 0 owns frames 0, 2, ..., 300
    assert res3["kernels"]["k_preprocess"]["launches"] == 2 * 5           # 151 = 4 x 32 + 23: five launches per step
    assert res3["value_kind"] == "end_to_end" and res3["end_to_end_with_host_corner_search"]["grids_found"] == 32


def test_bench_single_gpu_line_is_honest(ctx):
    """--gpus 1 line: value = the end-to-end figure BASELINE's metric names, value_device_only beside it; roofline.frac <= 1 and
    reproducible from its own fields; the traffic constant says where it comes from."""
    res = _bench(["--full", "--frames", "64", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    rf = res["roofline"]
    e2e = res["end_to_end_with_host_corner_search"]
    assert res["n_gpus"] == 1 and res["value_kind"] == "end_to_end" and res["metric"].startswith("end-to-end")
    assert res["value"] == res["value_end_to_end"] == e2e["value"] < res["value_device_only"]
    assert abs(res["value"] - 64 * 3 / (res["ms_per_step"] * 3e-3)) <= 1e-6 * res["value"]
    assert sorted(e2e["regions"])[1] == e2e["value"] and e2e["grids_found"] == e2e["of"] == 64
    assert 0 < rf["frac"] <= 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    assert len(res["ranks"]) == 1 and res["ranks"][0]["rank"] == 0 and res["ranks"][0]["pci_bus_id"]
    if rf["kernel"] == "k_conv_features":
        k = res["kernels"]["k_conv_features"]
        assert abs(rf["achieved"] * 1e12 - rf["issued_flop_per_cell"] * 81 * 64 / (k["avg_ms"] * 1e-3)) <= 1e-6 * rf["achieved"] * 1e12


def test_bench_plain_line_and_dumped_outputs(ctx, tmp_path):
    """A plain run (no --full) times exactly `steps` steps of the end-to-end path in one region and measures nothing beside it;
    --dump-outputs writes what that path returned for its last step, the same on a second run, and equal to the device path run
    in-process on the same seeded frames with the corners the host search found."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.synth import random_state_dict, synth_frames
    dumps = []
    for i in range(2):
        d = tmp_path / f"run{i}"
        res = _bench(["--frames", "32", "--steps", "3", "--warmup", "1", "--dump-outputs", str(d)])
        assert res["full"] is False and res["steps"] == 3 and res["value_kind"] == "end_to_end" and res["metric"].startswith("end-to-end")
        assert res["unit"] == "frames/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
        assert abs(res["value"] - 32 * 3 / (res["ms_per_step"] * 3e-3)) <= 1e-6 * res["value"]
        e2e = res["end_to_end_with_host_corner_search"]
        assert len(e2e["regions"]) == 1 and e2e["value"] == res["value"] and e2e["grids_found"] == 32
        assert not {"value_device_only", "kernels", "roofline", "cpu_baseline", "cpu_baseline_test_image"} & set(res)
        arrays = {k: np.load(d / f"{k}.npy") for k in ("logits", "digits", "conf", "corners", "found")}
        assert sorted(p.name for p in d.iterdir()) == sorted(f"{k}.npy" for k in arrays)
        assert all(v.dtype == np.float32 for v in arrays.values())
        assert [arrays[k].shape for k in ("logits", "digits", "conf", "corners", "found")] == [(32, 81, 10), (32, 81), (32, 81), (32, 4, 2), (32,)]
        dumps.append(arrays)
    for k in dumps[0]:
        assert (dumps[0][k] == dumps[1][k]).all(), k
    got = dumps[0]
    assert (got["found"] == 1).all()
    frames, _, _ = synth_frames(32, 1080, 1920, seed=1234, device="cuda")
    ctx.load_state_dict(random_state_dict(1234))
    want = ctx.frames_to_digits(frames, ctx.minv_to_device(sva.Context.corners_to_minv(got["corners"])))
    assert (want["digits"].cpu().numpy() == got["digits"]).all()
    assert np.abs(want["logits"].cpu().numpy() - got["logits"]).max() <= 1e-6
    assert np.abs(want["conf"].cpu().numpy() - got["conf"]).max() <= 1e-6


def test_bench_configs3_full_size(ctx):
    """BASELINE configs[3] at its stated size on one GPU: 100,000 frames through the 256-frame pool in one step.  Every kernel is
    launched ceil(100000/256) times, the step covers 100,000 frames, and the per-GPU device-only rate is that of configs[1]."""
    res = _bench(["--full", "--workload", "configs3", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"], timeout=900)
    assert res["scaling"] == "strong" and res["config"]["frames_per_step"] == 100000 and res["config"]["frames_per_gpu"] == 100000
    launches = -(-100000 // 256)
    for k in ("k_preprocess", "k_warp_cells", "k_conv_features", "k_fc_head"):
        assert res["kernels"][k]["launches"] == launches, k
    assert res["value_kind"] == "end_to_end" and res["end_to_end_with_host_corner_search"]["grids_found"] == 256
    ref = _bench(["--steps", "40", "--warmup", "10", "--no-e2e", "--no-cpu-baseline"])
    # (two separate runs: the same binary measures up to 5 % apart minutes apart on one box -- K1 0.594 vs 0.625 ms in profiles/r03_i -- so the bound
    # is 10 %; it is there to catch a workload that is not the one it says it is)
    assert abs(res["per_gpu_value_device_only"] / ref["value"] - 1) <= 0.10, (res["per_gpu_value_device_only"], ref["value"])


def test_degenerate_quad_does_not_abort_the_batch(ctx, golden_dir, monkeypatch):
    """A quad for which order_points (cv/grid.py:79-91) returns a point twice -- here a diamond, TR == BR -- makes the 8x8
    system singular.  In a batch that frame alone is reported not found (digits 0); the others are unaffected."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.pipeline import FramePipeline
    bad = np.array([[100, 0], [210, 100], [100, 200], [0, 95]], np.float32)
    with pytest.raises(sva._native.NativeError, match="SV_ERR_DEGENERATE"):
        sva.Context.corners_to_minv(bad[None])
    minv, ok = sva.Context.corners_to_minv_batch(np.stack([bad, bad + 7, np.array([[10, 10], [300, 12], [305, 290], [8, 300]], np.float32)]))
    assert ok.tolist() == [False, False, True] and (minv[0] == np.eye(3)).all()
    # in the pipeline: the search's answer for frame 2 replaced by that quad (a rasterised diamond rarely ties exactly)
    ctx.load_state_dict(_trained(golden_dir))
    frames, corners, _ = _frames_cuda(4, 540, 960, 8)
    real = sva.host.find_grid_corners_sparse_batch

    def search(*a, **k):
        c, f = real(*a, **k)
        c[2] = bad.astype(np.int32)
        return c, f

    monkeypatch.setattr(sva.host, "find_grid_corners_sparse_batch", search)
    pipe = FramePipeline(ctx, 540, 960, chunk=4, host_threads=2)
    assert pipe.packed and pipe.sparse
    res = pipe.run(frames)
    assert res["found"].tolist() == [True, True, False, True]
    assert (res["digits"][2] == 0).all()
    good = [0, 1, 3]
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(res["corners"][good].astype(np.float32)))
    assert torch.equal(res["digits"][good], ctx.frames_to_digits(frames[good].contiguous(), minv)["digits"])


def _frames_cuda(n, H, W, seed):
    from sudoku_vision_amd.synth import synth_frames
    return synth_frames(n, H, W, seed=seed, device="cuda")


def test_small_frames_skip_the_speck_filter(ctx, golden_dir):
    """sv_despeckle_u8 is exact only while min_area_ratio*H*W > 61*61: on a 150x150 frame (floor 2250 px) a grid that fits
    a 64x64 tile would be erased.  FramePipeline sends such frames through unfiltered and finds what the plain search finds."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd.pipeline import FramePipeline
    ctx.load_state_dict(_trained(golden_dir))
    H = W = 150
    frames = torch.full((2, H, W, 3), 215, dtype=torch.uint8, device="cuda")
    frames[0, 50:110, 48:108] = 25                                         # a 60x60 dark square: area 3481 > 0.1*150*150
    pipe = FramePipeline(ctx, H, W, chunk=2, host_threads=1)
    assert not pipe.despeckle and not pipe.packed
    res = pipe.run(frames)
    b = ctx.preprocess(frames).cpu().numpy()
    want = [sva.host.find_grid_corners(b[i]) for i in range(2)]
    assert want[0] is not None and want[1] is None
    assert res["found"].tolist() == [True, False] and (res["corners"][0] == want[0]).all()
    # the filter itself, applied regardless, would have lost it: the guard is what keeps the pipeline equal to the reference
    f = ctx.despeckle(ctx.preprocess(frames)).cpu().numpy()
    assert sva.host.find_grid_corners(f[0]) is None or (sva.host.find_grid_corners(f[0]) == want[0]).all()
    big = FramePipeline(ctx, 1080, 1920, chunk=2, host_threads=1)
    assert big.despeckle and big.packed


@pytest.mark.gpu
def test_copy_to_pinned_host(ctx):
    """sv_copy_to_pinned_host (the shader D2H copy of the end-to-end path): byte-exact for sizes with and without a 16-byte tail, ordered on
    the stream, and a pageable destination is refused."""
    g = torch.Generator().manual_seed(5)
    for nbytes in (16, 48 + 7, 1 << 20, (1 << 20) + 3, 259200 * 3):
        src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g)
        dev = src.to(ctx.device)
        dst = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
        ctx.copy_to_pinned(dev, dst)
        torch.cuda.synchronize()
        assert torch.equal(dst, src)
    with pytest.raises(TypeError):
        ctx.copy_to_pinned(dev, torch.zeros(nbytes, dtype=torch.uint8))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1080, 1920), (270, 480), (96, 3648), (50, 4128), (1300, 64), (700, 2112)])
def test_sparse_bit_records_kernel(ctx, H, W):
    """sv_pack_sparse_bits against the numpy statement of the record format (tests/test_host_contours.py), empty to dense frames, with and
    without overflow, one and two mask groups per row, frames whose row groups fit the kernel's register-resident form (<= 1152) and
    frames that do not (1300 x 64, 700 x 2112); and the records expand back to the dense image on the host."""
    import sudoku_vision_amd as sva
    from test_host_contours import _pack_sparse_np
    rng = np.random.RandomState(H)
    wpr = W // 32
    imgs = np.stack([np.packbits(rng.rand(H, W) < d, axis=1, bitorder="little").view(np.uint32) for d in (0.0, 0.001, 0.01, 0.2, 1.0)])
    imgs[4] = 0xFFFFFFFF
    gpr = (wpr + 63) // 64
    for cap in (H * wpr, H * wpr // 4, 4):
        stride = sva.host.sparse_bits_record_bytes(H, W, cap)
        rec = torch.full((len(imgs) + 1, stride), 0xEE, dtype=torch.uint8, device=ctx.device)
        got = ctx.pack_sparse_bits(torch.from_numpy(imgs.view(np.int32)).to(ctx.device), rec).cpu().numpy()
        assert (rec[len(imgs)].cpu().numpy() == 0xEE).all()                       # nothing written past the last record
        for k in range(len(imgs)):
            want = _pack_sparse_np(sva.host, imgs[k], cap)
            nvals, cap_eff = (int(v) for v in want[:8].view(np.uint32))
            used = 8 + 8 * H * gpr + 4 * min(nvals, cap_eff)
            assert np.array_equal(got[k][:used], want[:used]), (H, W, cap, k)
            assert (got[k][used:] == 0xEE).all()                                  # nor past a record's own values
            if nvals <= cap_eff:
                assert np.array_equal(sva.host.sparse_bits_expand(got[k], H, W), imgs[k])


@pytest.mark.gpu
def test_pipeline_sparse_handover_equals_dense(ctx):
    """The end-to-end pipeline with the binary handed to the host search as sparse records, as the dense bit image, and with every record
    forced to overflow (dense fallback per frame): identical corners, found flags and digits."""
    from sudoku_vision_amd import synth
    from sudoku_vision_amd.pipeline import FramePipeline
    ctx.load_state_dict(synth.random_state_dict(1234))
    frames = synth.synth_frames(6, 540, 960, seed=77, device=ctx.device)[0]
    frames[2] = 90                                                               # no grid in this one
    res = {}
    for name, sparse in (("sparse", True), ("dense", False), ("overflow", 16)):
        pipe = FramePipeline(ctx, 540, 960, chunk=4, host_threads=2, sparse=sparse)
        assert pipe.sparse == (name != "dense")
        out = pipe.run(frames)
        torch.cuda.synchronize()
        res[name] = (out["corners"].copy(), out["found"].copy(), out["digits"].cpu().numpy())
        if name == "overflow":
            assert pipe.dense_fallbacks == 5                                  # every frame but the flat one (no set pixels, nothing to overflow)
    assert res["dense"][1].tolist() == [True, True, False, True, True, True]
    for name in ("sparse", "overflow"):
        for a, b in zip(res[name], res["dense"]):
            assert np.array_equal(a, b), name


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", [(1080, 1920), (540, 960), (33, 64), (200, 2752), (16, 32)])
def test_bit_image_k1_and_despeckle(ctx, H, W):
    """sv_preprocess_bits_u8 = the bits of sv_preprocess_u8's binary, and sv_despeckle_bits (in place) = sv_despeckle_u8's packed output, on a
    synthetic frame, a noise frame and a flat one; the byte kernels are themselves bit-exact against the oracle elsewhere in this suite."""
    from sudoku_vision_amd import synth
    g = torch.Generator().manual_seed(H * W)
    frames = torch.randint(0, 256, (3, H, W, 3), dtype=torch.uint8, generator=g)
    if H >= 200:
        frames[0] = torch.from_numpy(np.asarray(synth.synth_frames(1, H, W, seed=H, noise="int")[0][0]))
    frames[2] = 77
    frames = frames.to(ctx.device)
    binary = ctx.preprocess(frames)
    bits = ctx.preprocess_bits(frames)
    want = np.packbits(binary.cpu().numpy() > 0, axis=2, bitorder="little").view(np.uint32).reshape(3, H, W // 32)
    assert np.array_equal(bits.cpu().numpy().view(np.uint32), want)
    packed = torch.empty_like(bits)
    ctx.despeckle(binary, out=torch.empty_like(binary), packed=packed)
    got = ctx.despeckle_bits(bits.clone())
    assert torch.equal(got, packed)
    assert want[2].sum() == 0                                                   # a flat frame thresholds to nothing


@pytest.mark.gpu
def test_pipeline_bit_image_path_equals_byte_path(ctx):
    """FramePipeline with K1 writing the bit image directly (default) and with the byte image + packing despeckle: same corners, digits."""
    from sudoku_vision_amd import synth
    from sudoku_vision_amd.pipeline import FramePipeline
    ctx.load_state_dict(synth.random_state_dict(1234))
    frames = synth.synth_frames(6, 540, 960, seed=78, device=ctx.device)[0]
    frames[4] = 30
    res = []
    for direct in (True, False):
        pipe = FramePipeline(ctx, 540, 960, chunk=4, host_threads=2, bits_direct=direct)
        assert ("bit image" in pipe.describe()) == direct
        out = pipe.run(frames)
        torch.cuda.synchronize()
        res.append((out["corners"].copy(), out["found"].copy(), out["digits"].cpu().numpy()))
    assert res[0][1].tolist() == [True, True, True, True, False, True]
    for a, b in zip(*res):
        assert np.array_equal(a, b)
    # a view with padded rows is not contiguous: the pipeline falls back to the byte path by itself
    wide = torch.zeros((6, 540, 992, 3), dtype=torch.uint8, device=ctx.device)
    wide[:, :, :960] = frames
    pipe = FramePipeline(ctx, 540, 960, chunk=4, host_threads=2)
    out = pipe.run(wide[:, :, :960])
    torch.cuda.synchronize()
    assert pipe.dev_bin is not None and np.array_equal(out["corners"], res[0][0]) and np.array_equal(out["digits"].cpu().numpy(), res[0][2])


@pytest.mark.gpu
@pytest.mark.parametrize("n,H,W", [(9, 540, 960), (3, 1080, 1920), (1, 64, 96)])
def test_fused_threshold_warp_launch(ctx, n, H, W):
    """BASELINE configs[4]'s fused threshold + warp (sv_preprocess_warp_cells_u8: K1 and K2 of the same frames in one launch, frame-to-XCD
    affinity) gives exactly what the two separate launches give; frame counts that do not fill the 8-XCD layout included."""
    import sudoku_vision_amd as sva
    from sudoku_vision_amd import synth
    frames, corners, _ = synth.synth_frames(n, H, W, seed=n + H, device=ctx.device)
    minv = ctx.minv_to_device(sva.Context.corners_to_minv(corners).reshape(n, 9))
    binary, cells = ctx.preprocess_and_warp_cells(frames, minv)
    assert torch.equal(binary, ctx.preprocess(frames))
    assert torch.equal(cells, ctx.warp_cells(frames, minv))
    host = frames[0].cpu().numpy()
    assert (binary[0].cpu().numpy() == o.preprocess_for_grid_detection(host)).all()
    assert (cells[0].cpu().numpy() == o.warp_cells(host, corners[0])).all()


@pytest.mark.gpu
def test_bench_latency_script_runs():
    """bench_latency.py (BASELINE configs[2]) end to end on a short back-to-back feed: one JSON line, every grid found, sub-5-ms frames."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench_latency.py"), "--frames", "24", "--fps", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["frames"] == 24 and d["grids_found"] == 24 and d["unit"] == "ms"
    assert 0 < d["frame_to_digits"]["p50"] < 5.0
