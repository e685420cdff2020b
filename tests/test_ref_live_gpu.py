"""GPU: the HIP path against THE REFERENCE ITSELF (unmodified reference host code + OpenCL kernels, oracle/_ref driven
by ref_runner), on seeds that are not in the golden set.  The reference ran each case on an MI355X and its results are
recorded bit for bit in tests/golden/ref_live.json (tests/golden/make_ref_live.py; inputs and scripts in
tests/ref_live_cases.py), so these tests need neither the reference's sources nor an OpenCL runtime."""
import numpy as np
import pytest

from ref_live_cases import HIP_CASES, HIP_TVALS, LEVELS, RANDOM_SEEDS, TINY_CASES, Recorded, hip_case, levels_case, random_case, tiny_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("hdr,H,W,si,so,R,delta,nb,seed,max_res", HIP_CASES)
def test_hip_matches_live_reference(native_lib, hdr, H, W, si, so, R, delta, nb, seed, max_res):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    case = hip_case(hdr, H, W, si, so, R, delta, nb, seed, max_res)
    ref = Recorded(case)
    f, js, tvals = case["frames"], ref.stats, HIP_TVALS

    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, si, so, delta, nb, 0.0, 255.0, max_res)
    c.m_opticalFlowSearchRadius = R
    for x in f[:3]:
        c.updateFrame(x)
    c.calculateOpticalFlow()
    assert c.m_totalFrameDelta == js[0]["total_frame_delta"]
    assert ref.same("off", c.readOffsets())
    assert ref.same("blur", c.readBlurredFlow(1))
    c.updateFrame(f[3]); c.calculateOpticalFlow()
    assert c.m_totalFrameDelta == js[1]["total_frame_delta"]
    if "off2" in ref.outputs:          # the tie cases: the second pair's offsets too
        assert ref.same("off2", c.readOffsets())
    for m in (0, 1, 2):
        for t in tvals:
            c.warpFrames(t, m)
            assert ref.same(f"w{m}_{t}", c.downloadFrame()), f"mode {m} t {t}"
    c.copyFrame()
    assert ref.same("copy", c.downloadFrame())
    # the same five outputs as ONE fused period launch (hf_interpolate_period_ex): at 2160p every thread produces all of
    # them (the launch shape bench.py times), judged here by the reference (warpFrameKernelHDR.h:116-184)
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch
    dt = np.uint16 if hdr else np.uint8
    outs = [DeviceBuffer(c.output_frame_bytes) for _ in tvals]
    zeros = np.zeros(c.output_frame_bytes, np.uint8)
    for b in outs:
        b.upload(zeros)            # the padding behind each row (output stride > width) is never written: zero as in the reference's buffer
    for m in (2, 0, 1):
        c.interpolateOnly(tvals, [b.ptr for b in outs], m)
        c.sync()
        for j, t in enumerate(tvals):
            assert ref.same(f"w{m}_{t}", outs[j].download(dt)), f"fused period, mode {m} t {t}"
    c.close()
    if H * W <= 1920 * 1080 and si == 0:
        # frames up to 1080p produce all outputs per thread only inside a batch of >= 11 members: 12 members, same frames
        n = 12
        cls = OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR
        members = [cls(H, W, si, so, delta, nb, 0.0, 255.0, max_res, search_radius=R, flags=capi.HF_FLAG_ASYNC) for _ in range(n)]
        batch = FlowBatch(members)
        dev = []
        for x in f:
            b = DeviceBuffer(x.nbytes); b.upload(x); dev.append(b)
        for k in range(4):
            batch.updateFramesDeviceRef([dev[k].ptr] * n)
            if k >= 2:
                batch.calculateOpticalFlow()
        mouts = [[DeviceBuffer(len(zeros)) for _ in tvals] for _ in range(n)]
        plans = [tvals[i % 5:] + tvals[:i % 5] for i in range(n)]
        batch.interpolatePeriod(plans, [[b.ptr for b in mo] for mo in mouts], 2)
        for i, mbr in enumerate(members):
            mbr.sync()
            assert mbr.m_totalFrameDelta == js[1]["total_frame_delta"]
            for j, t in enumerate(plans[i]):
                assert ref.same(f"w2_{t}", mouts[i][j].download(dt)), f"batched fused period, member {i} t {t}"
        batch.close()
        for mbr in members:
            mbr.close()


@pytest.mark.parametrize("hdr,H,W", TINY_CASES)
def test_tiny_frames_match_live_reference(native_lib, hdr, H, W):
    """4-row frames: the chroma plane has 2 rows and mirrorCoordinate's clamp(r, 1, dim - 2) has min > max -- OpenCL's
    min(max()) order decides.  HIP path and oracle against the reference itself."""
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    from oracle import oracle
    case = tiny_case(hdr, H, W)
    ref = Recorded(case)
    f = case["frames"]
    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, search_radius=5)
    for x in f[:3]:
        c.updateFrame(x)
    c.calculateOpticalFlow(); c.updateFrame(f[3]); c.calculateOpticalFlow()
    flow = c.readBlurredFlow(0)
    assert ref.same("flow", flow)        # from here on `flow` is the reference's blurred flow
    g = oracle.make_geom(hdr, H, W)
    for m in (0, 1, 2):
        c.warpFrames(0.43, m)
        assert ref.same(f"w{m}", c.downloadFrame()), m
        assert ref.same(f"w{m}", oracle.warp_frames(f[1], f[2], flow, g, 0.43, m)), ("oracle", m)
    c.copyFrame()
    assert ref.same("copy", c.downloadFrame())
    c.close()


@pytest.mark.parametrize("hdr", [0, 1])
def test_degenerate_levels_match_live_reference(native_lib, hdr):
    """Levels a settings UI can produce but no sane user wants: white == black, white = 0, black > white, out-of-range
    values (division by zero / negative scale inside apply_levels): blend and copy against the reference itself."""
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    from oracle import oracle
    for bk, wh in LEVELS:
        case = levels_case(hdr, bk, wh)
        ref = Recorded(case)
        f, H, W = case["frames"], case["H"], case["W"]
        g = oracle.make_geom(hdr, H, W)
        c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, 0, 0, 8, 6, bk, wh, 270, search_radius=8)
        for x in f[:3]:
            c.updateFrame(x)
        c.calculateOpticalFlow(); c.updateFrame(f[3]); c.calculateOpticalFlow()
        c.warpFrames(0.4, 2)
        assert ref.same("w2", c.downloadFrame()), (bk, wh)
        assert ref.same("w2", oracle.warp_frames(f[1], f[2], c.readBlurredFlow(0), g, 0.4, 2, bk, wh)), ("oracle", bk, wh)
        c.copyFrame()
        assert ref.same("copy", c.downloadFrame()), (bk, wh)
        assert ref.same("copy", oracle.copy_frame(f[1], g, bk, wh)), ("oracle", bk, wh)
        c.close()


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_random_configurations_match_live_reference(native_lib, seed):
    """The randomized sweep of test_random_gpu.py, but judged by the reference itself instead of the oracle: geometry,
    pitches, resolution scalar, search radius 2..16, scalars, levels, all production modes.
    The oracle is checked against the same outputs, so every seed pins it once more."""
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    from oracle import oracle
    case = random_case(seed)
    ref = Recorded(case)
    f, js, ts, cfg = case["frames"], ref.stats, case["ts"], case["cfg"]
    hdr, H, W, si, so, max_res, R, delta, nb, bk, wh = (cfg[k] for k in ("hdr", "H", "W", "si", "so", "max_res", "R", "delta", "nb", "bk", "wh"))
    g = oracle.make_geom(hdr, H, W, si, so, max_res)
    off_o, blur_o, tot_o, oob = oracle.calculate_optical_flow(f[1], f[2], g, R, 0, delta, nb, 4)
    c = (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(H, W, si, so, delta, nb, bk, wh, max_res, search_radius=R)
    for x in f[:3]:
        c.updateFrame(x)
    c.calculateOpticalFlow()
    if oob == 0:    # otherwise the reference reads outside its frame buffers (undefined)
        assert c.m_totalFrameDelta == js[0]["total_frame_delta"] == tot_o, cfg
        assert ref.same("off", c.readOffsets()) and ref.same("off", off_o), cfg
        blur = c.readBlurredFlow(1)
        assert ref.same("blur", blur) and ref.same("blur", blur_o), cfg     # from here on `blur` is the reference's blurred flow
        c.updateFrame(f[3]); c.calculateOpticalFlow()
        for m in (0, 1, 2):
            for t in ts:
                c.warpFrames(t, m)
                assert ref.same(f"w{m}_{t}", c.downloadFrame()), (cfg, m, t)
                assert ref.same(f"w{m}_{t}", oracle.warp_frames(f[1], f[2], blur, g, t, m, bk, wh)), (cfg, "oracle", m, t)
        c.copyFrame()
        assert ref.same("copy", c.downloadFrame()), cfg
    c.close()
