"""CPU: the encoder's host half through the C ABI (csrc/host_jpeg.cpp: sv_jpeg_encode_plan, sv_jpeg_entropy_encode, _batch), fed the sparse records of
tests/jpeg_encode_ref.py, writes that restatement's bytes -- which tests/test_jpeg_encode_ref.py pins to Pillow's.  Threads do not change the bytes;
bad arguments come back as SV_ERR_BAD_ARG, a small buffer as SV_ERR_BUFFER."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_encode_ref as R

SAMPLING_CODE = {"gray": 0, "444": 0, "422": 1, "420": 2}
BAD_ARG, BUFFER = -1, -6


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    import sudoku_vision_amd as sva
    if not os.path.exists(sva._native.LIB_PATH):
        g.build()
    return sva._native.lib()


def make_plan(lib, W, H, sampling, quality, restart):
    from sudoku_vision_amd._native import JpegEnc
    plan = JpegEnc()
    rc = lib.sv_jpeg_encode_plan(W, H, 1 if sampling == "gray" else 3, SAMPLING_CODE[sampling], quality, restart, C.byref(plan))
    assert rc == 0, lib.sv_last_error()
    return plan


def host_encode(lib, plan, masks, offsets, values, threads=1, cap=None):
    masks, offsets = np.ascontiguousarray(masks, np.uint64), np.ascontiguousarray(offsets, np.uint32)
    vals = np.ascontiguousarray(np.concatenate([values, np.zeros(1, np.int16)]), np.int16)         # never an empty buffer
    cap = lib.sv_jpeg_encode_bound(C.byref(plan), int(values.size)) if cap is None else cap
    out = np.zeros(max(cap, 1), np.uint8)
    size = C.c_size_t()
    rc = lib.sv_jpeg_entropy_encode(C.byref(plan), masks.ctypes.data, offsets.ctypes.data, vals.ctypes.data, int(values.size), out.ctypes.data, cap, C.byref(size), threads)
    return rc, out[:size.value].tobytes() if rc == 0 else size.value


@pytest.mark.parametrize("kind", R.CONTENTS)
@pytest.mark.parametrize("sampling", list(R.SAMPLINGS))
def test_host_encoder_writes_the_restatements_bytes(lib, sampling, kind):
    for H, W in R.SIZES:
        img = R.content(kind, H, W, sampling == "gray")
        for q in R.QUALITIES:
            geo, coef, quant = R.forward(img, q, sampling)
            records = R.sparse(coef)
            for restart in R.RESTARTS:
                plan = make_plan(lib, W, H, sampling, q, restart)
                assert plan.info.coef_count == geo.coef_count and (np.array(plan.quant).reshape(3, 64)[:geo.ncomp] == quant[:geo.ncomp]).all()
                want = R.entropy_encode(geo, coef, quant, restart)
                rc, got = host_encode(lib, plan, *records)
                assert rc == 0 and got == want, (H, W, q, restart)
                if restart:
                    rc, threaded = host_encode(lib, plan, *records, threads=4)
                    assert rc == 0 and threaded == got, (H, W, q, restart)


def test_plan_matches_the_decoders_parse(lib):
    """the plan's geometry is what sv_jpeg_parse reads back from the file"""
    from sudoku_vision_amd import host
    for sampling in R.SAMPLINGS:
        img = R.content("noise", 33, 17, sampling == "gray")
        info = host.jpeg_parse(R.encode(img, 75, sampling, 3))
        plan = make_plan(lib, 17, 33, sampling, 75, 3)
        for name in ("width", "height", "out_width", "out_height", "components", "h_samp", "v_samp", "orientation", "restart_interval", "coef_count"):
            assert getattr(plan.info, name) == getattr(info, name), (sampling, name)


def test_batch_equals_single_and_threads_do_not_matter(lib):
    H, W, n = 40, 24, 5
    plan = make_plan(lib, W, H, "420", 75, 1)
    recs, singles = [], []
    for kind in ("noise", "checker", "zeros", "ramp", "photo"):
        _, coef, _ = R.forward(R.content(kind, H, W), 75, "420")
        m, o, v = R.sparse(coef)
        recs.append((np.ascontiguousarray(m), np.ascontiguousarray(o), np.ascontiguousarray(np.concatenate([v, np.zeros(1, np.int16)])), v.size))
        singles.append(host_encode(lib, plan, m, o, v)[1])
    VP = C.c_void_p * n
    for threads in (1, 3):
        cap = int(plan.out_bound)
        outs = [np.zeros(cap, np.uint8) for _ in range(n)]
        sizes, status = (C.c_size_t * n)(), (C.c_int * n)()
        rc = lib.sv_jpeg_entropy_encode_batch(C.byref(plan), n, VP(*[r[0].ctypes.data for r in recs]), VP(*[r[1].ctypes.data for r in recs]),
                                              VP(*[r[2].ctypes.data for r in recs]), (C.c_long * n)(*[r[3] for r in recs]), VP(*[o.ctypes.data for o in outs]),
                                              (C.c_size_t * n)(*[cap] * n), sizes, threads, status)
        assert rc == 0 and list(status) == [0] * n
        assert [outs[i][:sizes[i]].tobytes() for i in range(n)] == singles


def test_argument_errors(lib):
    from sudoku_vision_amd._native import JpegEnc
    plan = JpegEnc()
    good = (16, 16, 3, 2, 75, 0)
    for i, bad in ((4, 0), (4, 101), (3, 3), (3, -1), (0, 0), (1, -5), (0, 65536), (2, 2), (5, -1), (5, 65536)):
        args = list(good)
        args[i] = bad
        assert lib.sv_jpeg_encode_plan(*args, C.byref(plan)) == BAD_ARG, args
    assert lib.sv_jpeg_encode_plan(*good, None) == BAD_ARG
    assert lib.sv_jpeg_encode_plan(16, 16, 1, 99, 75, 0, C.byref(plan)) == 0          # gray: sampling is ignored
    # host half: too small a buffer reports what is needed; NULL and malformed records are refused
    plan = make_plan(lib, 16, 16, "420", 75, 0)
    _, coef, _ = R.forward(R.content("noise", 16, 16), 75, "420")
    m, o, v = R.sparse(coef)
    rc, good_bytes = host_encode(lib, plan, m, o, v)
    assert rc == 0
    rc, need = host_encode(lib, plan, m, o, v, cap=len(good_bytes) - 1)
    assert rc == BUFFER and need == len(good_bytes) and b"bytes" in lib.sv_last_error()
    assert host_encode(lib, plan, m, o, v, cap=len(good_bytes))[0] == 0
    size = C.c_size_t()
    assert lib.sv_jpeg_entropy_encode(C.byref(plan), None, None, None, 0, None, 0, C.byref(size), 1) == BAD_ARG
    assert host_encode(lib, plan, m, o, v[:-3])[0] == BAD_ARG                          # records refer beyond values_count
    z = v.copy()
    z[5] = 0
    assert host_encode(lib, plan, m, o, z)[0] == BAD_ARG                               # a zero under a set bit
    z = v.copy()
    z[1] = 2000
    assert host_encode(lib, plan, m, o, z)[0] == BAD_ARG                               # no baseline code for the value
    assert lib.sv_jpeg_encode_bound(None, 0) == -1
    # device half: checked before anything is launched, so a NULL context is enough to see the order of the checks
    assert lib.sv_jpeg_forward_bgr_u8(None, C.byref(plan), None, 1, 48, 0, None, None, None, None, None, None) == BAD_ARG
