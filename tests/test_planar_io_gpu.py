"""GPU: planar 4:2:0 frames at the boundary (HF_FLAG_PLANAR_IN / HF_FLAG_PLANAR_OUT, include/hopperflow.h, csrc/hf_planar.hip).  Every
case runs a plain NV12 / P010 context and a planar one on the same pictures: the planar outputs must equal the plain outputs converted
(tests/planar_ref.py) over the valid columns, byte for byte, and the two contexts' flow, m_totalFrameDelta and phase planes must be
equal.  The planar inputs carry garbage in their padding columns (never read) and the plain twin gets exactly what the device makes of
them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import planar_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIN, POUT = 0x8000, 0x10000


def _cls(hdr):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR


def _pictures(H, W, S, hdr, n, seed=9, wrap=False, cut_at=None):
    """(planar frames of stride S, their NV12 / P010 twins) -- n pictures of a moving synthetic scene (a hard cut at cut_at)."""
    from hopperrender_amd import synth
    a, b = synth.Scene(H, W, hdr, seed), synth.Scene(H, W, hdr, seed + 999)
    rng = np.random.default_rng(seed)
    planar, twin = [], []
    for k in range(n):
        nv = (b if cut_at is not None and k >= cut_at else a).frame(k)
        p = planar_ref.semiplanar_to_planar(nv, H, W, W, hdr)
        y, u, v = planar_ref.planar_planes(p, H, W, W)
        dt = np.uint16 if hdr else np.uint8
        q = rng.integers(0, 65536 if hdr else 256, H * S * 3 // 2).astype(dt)    # padding garbage
        qy, qu, qv = planar_ref.planar_planes(q, H, W, S)
        qy[:], qu[:], qv[:] = y, u, v
        if wrap:   # LSB-aligned values above 1023 lose their top bits on the way in
            qy[::7, ::3] |= 0xA800
            qu[::3, ::5] |= 0x4400
            qv[1::4, ::2] |= 0xFC00
        planar.append(q)
        twin.append(planar_ref.planar_to_semiplanar(q, H, W, S, hdr))
    return planar, twin


def _same_output(planar_side_out, plain_out, H, W, S, hdr, planar):
    a = planar_ref.valid_planes_of_output(planar_side_out, H, W, S, hdr, planar)
    b = planar_ref.valid_planes_of_output(plain_out, H, W, S, hdr, False)
    for x, y, name in zip(a, b, "YUV"):
        assert x.shape == y.shape and (x == y).all(), f"plane {name} differs"


def _same_state(A, B, slots=(0, 1, 2)):
    assert A.m_totalFrameDelta == B.m_totalFrameDelta
    for i in (0, 1):
        assert (A.readBlurredFlow(i) == B.readBlurredFlow(i)).all()
    for s in slots:
        pa, ca = A.readPhasePlane(s)
        pb, cb = B.readPhasePlane(s)
        assert ca == cb and (pa == pb).all()


CASES = [  # H, W, S_in, S_out, hdr, flags, R
    (180, 320, 320, 320, 0, PIN | POUT, 8),
    (180, 320, 320, 320, 1, PIN | POUT, 8),
    (180, 320, 336, 330, 0, PIN, 8),
    (180, 320, 330, 336, 1, POUT, 8),
    (722, 1282, 1300, 1288, 0, PIN | POUT, 16),
    (722, 1282, 1290, 1296, 1, PIN | POUT, 16),
    (1080, 1920, 1920, 1920, 0, PIN | POUT, 16),
    (1080, 1920, 1920, 1920, 1, PIN | POUT, 16),
    (2160, 3840, 3840, 3840, 1, PIN | POUT, 16),
]


@pytest.mark.parametrize("H,W,Si,So,hdr,flags,R", CASES)
def test_blocking_calls_all_modes(native_lib, H, W, Si, So, hdr, flags, R):
    """hf_update_frame / hf_download_frame: output modes 0-6 and copyFrame, flow, delta and phase planes vs the plain context."""
    planar, twin = _pictures(H, W, Si, hdr, 4)
    A = _cls(hdr)(H, W, Si, So, search_radius=R)
    B = _cls(hdr)(H, W, Si, So, search_radius=R, flags=flags)
    for k in range(4):
        A.updateFrame(twin[k])
        B.updateFrame(planar[k] if flags & PIN else twin[k])
        if k >= 2:
            A.calculateOpticalFlow(); B.calculateOpticalFlow()
            _same_state(A, B)
    for mode in range(7):
        A.warpFrames(0.4, mode); B.warpFrames(0.4, mode)
        _same_output(B.downloadFrame(), A.downloadFrame(), H, W, So, hdr, bool(flags & POUT))
    A.copyFrame(); B.copyFrame()
    _same_output(B.downloadFrame(), A.downloadFrame(), H, W, So, hdr, bool(flags & POUT))
    A.close(); B.close()


@pytest.mark.parametrize("H,W", [(180, 320), (722, 1282)])
def test_hdr_values_above_1023_wrap(native_lib, H, W):
    hdr = 1
    planar, twin = _pictures(H, W, W, hdr, 4, wrap=True)
    A, B = _cls(hdr)(H, W, search_radius=8), _cls(hdr)(H, W, search_radius=8, flags=PIN | POUT)
    for k in range(4):
        A.updateFrame(twin[k]); B.updateFrame(planar[k])
    A.calculateOpticalFlow(); B.calculateOpticalFlow()
    _same_state(A, B)
    A.warpFrames(0.5, 2); B.warpFrames(0.5, 2)
    _same_output(B.downloadFrame(), A.downloadFrame(), H, W, W, hdr, True)
    A.close(); B.close()


@pytest.mark.parametrize("H,W,Si,So,hdr", [(180, 320, 320, 320, 0), (722, 1282, 1300, 1288, 1), (1080, 1920, 1920, 1920, 0)])
def test_device_entry_points(native_lib, H, W, Si, So, hdr):
    """hf_update_frame_device, hf_update_frame_device_ref (one buffer overwritten after every call: the planar context keeps no
    reference), hf_download_frame_device, hf_set_output_buffer's rejection."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer
    planar, twin = _pictures(H, W, Si, hdr, 5)
    A = _cls(hdr)(H, W, Si, So, search_radius=16)
    B = _cls(hdr)(H, W, Si, So, search_radius=16, flags=PIN | POUT)
    Cc = _cls(hdr)(H, W, Si, So, search_radius=16, flags=PIN | POUT)
    dev = DeviceBuffer(planar[0].nbytes)
    out_a, out_b = DeviceBuffer(A.output_frame_bytes), DeviceBuffer(A.output_frame_bytes)
    dt = np.uint16 if hdr else np.uint8
    for k in range(5):
        A.updateFrame(twin[k])
        dev.upload(planar[k])
        B.updateFrameDevice(dev.ptr)
        Cc.updateFrameDeviceRef(dev.ptr)
        if k >= 2:
            for m in (A, B, Cc):
                m.calculateOpticalFlow()
            _same_state(A, B); _same_state(A, Cc)
    for m in (A, B, Cc):
        m.warpFrames(0.3, 2)
    A.downloadFrameDevice(out_a.ptr)
    B.downloadFrameDevice(out_b.ptr)
    _same_output(out_b.download(dt), out_a.download(dt), H, W, So, hdr, True)
    _same_output(Cc.downloadFrame(), A.downloadFrame(), H, W, So, hdr, True)
    with pytest.raises(capi.HopperFlowError) as e:
        B.setOutputBuffer(out_b.ptr)
    assert e.value.code == capi.HF_ERR_STATE
    B.setOutputBuffer(None)   # restoring the internal buffer stays allowed
    for m in (A, B, Cc):
        m.close()


@pytest.mark.parametrize("hdr,flags", [(0, PIN | POUT), (1, PIN | POUT), (0, POUT), (1, PIN)])
def test_interpolate_period_five_outputs(native_lib, hdr, flags):
    """hf_interpolate_period: device_frame planar, 5 device outputs planar (fused period warp into stages, then converted)."""
    from hopperrender_amd.calc import DeviceBuffer
    H, W = 1080, 1920
    planar, twin = _pictures(H, W, W, hdr, 5)
    A = _cls(hdr)(H, W, search_radius=16, flags=0x1)
    B = _cls(hdr)(H, W, search_radius=16, flags=0x1 | flags)
    ts = [0.2, 0.4, 0.6, 0.8, 1.0]
    dev_a = [DeviceBuffer(f.nbytes) for f in twin]
    dev_b = [DeviceBuffer(f.nbytes) for f in planar]
    outs_a = [DeviceBuffer(A.output_frame_bytes) for _ in ts]
    outs_b = [DeviceBuffer(A.output_frame_bytes) for _ in ts]
    dt = np.uint16 if hdr else np.uint8
    for k in range(5):
        dev_a[k].upload(twin[k]); dev_b[k].upload(planar[k] if flags & PIN else twin[k])
        A.interpolatePeriod(dev_a[k].ptr, ts, [o.ptr for o in outs_a])
        B.interpolatePeriod(dev_b[k].ptr, ts, [o.ptr for o in outs_b])
        A.sync(); B.sync()
        if k >= 2:
            _same_state(A, B)
            for oa, ob in zip(outs_a, outs_b):
                _same_output(ob.download(dt), oa.download(dt), H, W, W, hdr, bool(flags & POUT))
    A.close(); B.close()


@pytest.mark.parametrize("hdr", [0, 1])
def test_async_dual_stream_longer_than_the_output_ring(native_lib, hdr):
    """hf_update_frame_async / hf_download_frame_async on an HF_FLAG_DUAL_STREAM context, 2 outputs per period over 10 periods (the
    3-slot output ring and its stages are reused many times) vs the blocking plain context."""
    from hopperrender_amd.calc import PinnedArray
    H, W, n = 360, 640, 10
    planar, twin = _pictures(H, W, W, hdr, n)
    A = _cls(hdr)(H, W, search_radius=8)
    B = _cls(hdr)(H, W, search_radius=8, flags=0x1 | 0x40 | PIN | POUT)
    dt = np.uint16 if hdr else np.uint8
    pins_in = [PinnedArray(planar[0].size, dt) for _ in range(n)]
    pins_out = [PinnedArray(planar[0].size, dt) for _ in range(2 * n)]
    want = []
    j = 0
    for k in range(n):
        pins_in[k].array[:] = planar[k]
        A.updateFrame(twin[k]); B.updateFrameAsync(pins_in[k])
        if k >= 2:
            A.calculateOpticalFlow(); B.calculateOpticalFlow()
        for t in (0.25, 0.75):
            if k >= 3:
                A.warpFrames(t, 2); B.warpFrames(t, 2)
            else:
                A.copyFrame(); B.copyFrame()
            want.append(A.downloadFrame().copy())
            B.downloadFrameAsync(pins_out[j]); j += 1
    B.sync()
    _same_state(A, B)
    for w, p in zip(want, pins_out):
        _same_output(p.array, w, H, W, W, hdr, True)
    A.close(); B.close()
    for p in pins_in + pins_out:
        p.free()


@pytest.mark.parametrize("hdr,native", [(0, False), (1, False), (0, True), (1, True)])
def test_filter_protocol(native_lib, hdr, native):
    """FilterReplay.deliver (the calculator's blocking calls) and NativeFilter.deliver (hf_filter_deliver) with planar frames."""
    from hopperrender_amd.protocol import SOURCE_24, TARGET_60, FilterReplay, NativeFilter
    H, W, n = 180, 320, 12
    planar, twin = _pictures(H, W, W, hdr, n, cut_at=7)
    A = _cls(hdr)(H, W, search_radius=8)
    B = _cls(hdr)(H, W, search_radius=8, flags=PIN | POUT)
    if native:
        fa, fb = NativeFilter(SOURCE_24, TARGET_60, scene_change_threshold=150), NativeFilter(SOURCE_24, TARGET_60, scene_change_threshold=150)
        for k in range(n):
            oa, ka = fa.deliver(A, twin[k])
            ob, kb = fb.deliver(B, planar[k])
            assert ka == kb and len(oa) == len(ob)
            for x, y in zip(ob, oa):
                _same_output(x, y, H, W, W, hdr, True)
        fa.close(); fb.close()
    else:
        ra, rb = FilterReplay(A, SOURCE_24, TARGET_60, scene_change_threshold=150), FilterReplay(B, SOURCE_24, TARGET_60, scene_change_threshold=150)
        for k in range(n):
            oa, ob = ra.deliver(twin[k]), rb.deliver(planar[k])
            assert len(oa) == len(ob)
            for x, y in zip(ob, oa):
                _same_output(x, y, H, W, W, hdr, True)
        assert ra.log == rb.log
    _same_state(A, B)
    A.close(); B.close()


@pytest.mark.parametrize("hdr", [0, 1])
def test_hostio_chunk_with_a_hard_cut(native_lib, hdr):
    """A HostIoRunner chunk (hf_hostio: pinned rings, async I/O, dual stream) with planar fill / sink vs its NV12 twin."""
    from hopperrender_amd import batch
    from hopperrender_amd.hostio import HostIoRunner
    from hopperrender_amd.protocol import SOURCE_24, TARGET_120
    H, W, n = 180, 320, 40
    planar, twin = _pictures(H, W, W, hdr, n, cut_at=27)
    chunk = batch.shard_timeline(n, 2, 1, SOURCE_24, TARGET_120)
    res = {}
    for name, flags, src in (("nv12", 0, twin), ("planar", PIN | POUT, planar)):
        r = HostIoRunner(hdr, H, W, search_radius=8, out_ring=4, flags=flags)
        outs = []

        def fill(k, arr, src=src):
            arr[:] = src[k]

        def sink(i, arr, kind, outs=outs):
            outs.append(arr.copy())

        kinds = r.run(chunk, fill, sink, 2, 150, SOURCE_24, TARGET_120)
        r.close()
        res[name] = (kinds, outs)
    assert res["nv12"][0] == res["planar"][0]
    assert len(res["nv12"][1]) == len(res["planar"][1]) > 0
    for x, y in zip(res["planar"][1], res["nv12"][1]):
        _same_output(x, y, H, W, W, hdr, True)


def test_planar_convert_device_alignments(native_lib):
    """The re-layout kernels alone (hf_planar_convert_device) on buffers at every 2-byte misalignment (the element-wise path) and
    aligned (the wide path), both directions, against the reference."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer
    lib = capi.load()
    for H, W, S, hdr in ((180, 320, 320, 1), (722, 1282, 1290, 0), (34, 66, 70, 1), (10, 20, 22, 0)):
        c = _cls(hdr)(H, W, S, S, flags=PIN | POUT)
        dt = np.uint16 if hdr else np.uint8
        n = H * S * 3 // 2
        rng = np.random.default_rng(H)
        p = rng.integers(0, 65536 if hdr else 256, n).astype(dt)
        for off in (0, 2, 4, 6, 8):
            src, dst = DeviceBuffer(p.nbytes + 64), DeviceBuffer(p.nbytes + 64)
            host = np.zeros(p.nbytes + 64, np.uint8)
            host[off:off + p.nbytes] = p.view(np.uint8)
            src.upload(host)
            dst.upload(np.zeros_like(host))
            capi.check(lib.hf_planar_convert_device(c._ctx, 0, C.c_void_p(src.ptr + off), C.c_void_p(dst.ptr + off)), c._ctx)
            got = dst.download(np.uint8)
            assert (got[:off] == 0).all() and (got[off + p.nbytes:] == 0).all(), "wrote outside the frame"
            semi = got[off:off + p.nbytes].view(dt)
            want = planar_ref.planar_to_semiplanar(p, H, S, S, hdr)   # whole rows: the padding is converted like the rest
            assert (semi == want).all()
            capi.check(lib.hf_planar_convert_device(c._ctx, 1, C.c_void_p(dst.ptr + off), C.c_void_p(src.ptr + off)), c._ctx)
            back = src.download(np.uint8)[off:off + p.nbytes].view(dt)
            assert (back == planar_ref.semiplanar_to_planar(want, H, S, S, hdr)).all()
            src.free(); dst.free()
        c.close()


def test_rejections(native_lib):
    from hopperrender_amd import capi
    from hopperrender_amd.calc import FlowBatch, OpticalFlowCalcSDR
    for kw in (dict(inputStride=323, flags=PIN), dict(outputStride=325, flags=POUT)):
        with pytest.raises(capi.HopperFlowError) as e:
            OpticalFlowCalcSDR(180, 320, **kw)
        assert e.value.code == capi.HF_ERR_INVALID_ARGUMENT and "even stride" in str(e.value)
    OpticalFlowCalcSDR(180, 320, 323, 325).close()                 # odd strides stay fine on NV12 sides
    OpticalFlowCalcSDR(180, 320, 323, 326, flags=POUT).close()     # ... and on the side that is not planar
    a = OpticalFlowCalcSDR(180, 320, flags=0x1)
    b = OpticalFlowCalcSDR(180, 320, flags=0x1 | PIN)
    with pytest.raises(capi.HopperFlowError):
        FlowBatch([a, b])
    with pytest.raises(capi.HopperFlowError):
        FlowBatch([b])
    FlowBatch([a]).close()
    a.close(); b.close()


# ---- CLI ----
def _write_y4m(path, frames_planar, H, W, hdr):
    from hopperrender_amd.y4m import Y4MWriter
    with open(path, "wb") as f:
        w = Y4MWriter(f, W, H, 24000, 1001, hdr)
        for p in frames_planar:
            w.write_planar(p)


def _rewrap_nv12_as_y4m(nv12_path, y4m_path, H, W, hdr, fps=60):
    from hopperrender_amd.y4m import Y4MWriter
    dt = np.dtype("<u2") if hdr else np.dtype(np.uint8)
    data = np.fromfile(nv12_path, dtype=dt).reshape(-1, H * W * 3 // 2)
    with open(y4m_path, "wb") as f:
        w = Y4MWriter(f, W, H, fps, 1, hdr)
        for fr in data:
            w.write(fr)


def _cli(args):
    r = subprocess.run([sys.executable, "-m", "hopperrender_amd.cli"] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]


@pytest.mark.parametrize("hdr", [0, 1])
def test_cli_y4m_and_raw_planar_equal_the_nv12_run(native_lib, tmp_path, hdr):
    H, W, n = 180, 320, 14
    planar, twin = _pictures(H, W, W, hdr, n, cut_at=9)
    nv_in = tmp_path / "in.raw"
    np.concatenate(twin).astype("<u2" if hdr else np.uint8).tofile(nv_in)
    base = ["--width", str(W), "--height", str(H), "--radius", "8", "--scene-threshold", "150"] + (["--hdr"] if hdr else [])
    _cli([str(nv_in), str(tmp_path / "ref.raw")] + base)
    _rewrap_nv12_as_y4m(tmp_path / "ref.raw", tmp_path / "ref.y4m", H, W, hdr)
    ref_y4m = (tmp_path / "ref.y4m").read_bytes()
    ref_raw_planar = b"".join(planar_ref.semiplanar_to_planar(f, H, W, W, hdr).astype("<u2" if hdr else np.uint8).tobytes()
                              for f in np.fromfile(tmp_path / "ref.raw", dtype="<u2" if hdr else np.uint8).reshape(-1, H * W * 3 // 2))
    _write_y4m(tmp_path / "in.y4m", planar, H, W, hdr)
    common = ["--radius", "8", "--scene-threshold", "150", "--target-fps", "60"]
    _cli([str(tmp_path / "in.y4m"), str(tmp_path / "out_b.y4m")] + common)
    assert (tmp_path / "out_b.y4m").read_bytes() == ref_y4m
    _cli([str(tmp_path / "in.y4m"), str(tmp_path / "out_g.y4m"), "--gpus", "2"] + common)
    assert (tmp_path / "out_g.y4m").read_bytes() == ref_y4m
    pin = tmp_path / "in.yuv"
    np.concatenate(planar).astype("<u2" if hdr else np.uint8).tofile(pin)
    fmt = ["--pix-fmt", "yuv420p10le" if hdr else "yuv420p", "--width", str(W), "--height", str(H)]
    _cli([str(pin), str(tmp_path / "out_b.yuv")] + fmt + common)
    assert (tmp_path / "out_b.yuv").read_bytes() == ref_raw_planar
    _cli([str(pin), str(tmp_path / "out_g.yuv"), "--gpus", "2"] + fmt + common)
    assert (tmp_path / "out_g.yuv").read_bytes() == ref_raw_planar


def test_cli_in_process_without_the_host_relayout(native_lib, tmp_path, monkeypatch):
    """The .y4m -> .y4m run with y4m.planar_to_semiplanar / semiplanar_to_planar made to raise: the re-layout has left the host path."""
    from hopperrender_amd import cli, y4m
    H, W, n = 180, 320, 8
    planar, twin = _pictures(H, W, W, 0, n)
    _write_y4m(tmp_path / "in.y4m", planar, H, W, False)
    nv_in = tmp_path / "in.nv12"
    np.concatenate(twin).tofile(nv_in)
    cli.main([str(nv_in), str(tmp_path / "ref.nv12"), "--width", str(W), "--height", str(H), "--radius", "8"])
    _rewrap_nv12_as_y4m(tmp_path / "ref.nv12", tmp_path / "ref.y4m", H, W, False)

    def boom(*a, **k):
        raise AssertionError("host re-layout called")

    monkeypatch.setattr(y4m, "planar_to_semiplanar", boom)
    monkeypatch.setattr(y4m, "semiplanar_to_planar", boom)
    cli.main([str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), "--radius", "8", "--target-fps", "60"])
    assert (tmp_path / "out.y4m").read_bytes() == (tmp_path / "ref.y4m").read_bytes()
