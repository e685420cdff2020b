"""GPU: the arithmetic every kernel that writes an output frame ends in -- the blend, the output levels, the flow views -- over its whole
input domain (tests/output_arith_model.py; tests/test_output_arith_model.py holds the model to the oracle and proves that these inputs
tell every listed flawed variant apart).

Levels are compared THROUGH THE DEVICE'S OWN RECIPROCAL: deviceRcp of every white - black and white of LEVELS (times 256 on 16-bit
frames) feeds oracle.set_flavour(1, 1, rcp=...), so arbitrary settings -- not only the spans whose v_rcp_f32 is correctly rounded -- are
held bit for bit.  With zero flow injected an output element is a pure function of one element of each source frame; the ramp frames put
every code value into luma, U and V.

  packed body      warp_finish_to inside warp_fast_kernel: 256 x 512 at rs 1, warpFrames and a fused interpolateOnly, mode 2
  scalar body      warp_element: the same frames at rs 0 (warp_kernel), with the output at base + 2 bytes, and the fast kernel's ragged
                   right edge (W = 510, where the last thread's vector crosses W)
  copy_kernel      copyFrame, aligned and with the source at base + 2 bytes
  scene_copy       a fresh batch's first period (a copy: m_frameCount < 3) through runPeriodAuto, both element types x both access widths
  flow views       modes 3 and 4 on injected flow fields that sweep direction, magnitude, both gains and the clamps

every one at every entry of LEVELS (scene_copy: SCENE_LEVELS; flow views: 0 / 255) and every blend scalar, against the oracle bit for bit.
Mode 3: every element lies in the model's accepted set (at least 97 % of the vectors have exactly one accepted value).

warp_wg_kernel (the staged kernel) is not run here: its launches need 4 x 8192 wave tiles (tests/test_warp_variants_gpu.py runs them), and
its three bodies finish through the same code -- the staged and the interior-global body call warp_finish_to (csrc/hf_kernels.hip
warp_wg_body), the generic body is warp_fast_body's, i.e. warp_finish_to or warp_element."""
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import output_arith_model as M  # noqa: E402
import warp_variant_model as V  # noqa: E402
from test_batch_scene_gpu import GUARD, Outputs  # noqa: E402
from test_warp_variants_gpu import Buf  # noqa: E402

pytestmark = pytest.mark.gpu

_pool = ThreadPoolExecutor(12)     # (the oracle is plain C behind ctypes)
_cache = {}
ELEM = pytest.mark.parametrize("hdr", [0, 1], ids=["u8", "u16"])


@pytest.fixture(autouse=True)
def _default_flavour():
    from oracle import oracle
    try:
        yield
    finally:
        oracle.set_flavour(1, 1, None)


def calc_class(hdr):
    from hopperrender_amd.calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
    return OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR


def context(hdr, max_res, w=M.W, si=0, so=0, levels=(0.0, 255.0), flags=None):
    from hopperrender_amd import capi
    return calc_class(hdr)(M.H, w, si, so, 8, 6, levels[0], levels[1], max_res, search_radius=5,
                           flags=capi.HF_FLAG_ASYNC | capi.HF_FLAG_NO_TIMING if flags is None else flags)


def set_levels(c, levels):
    c.m_outputBlackLevel, c.m_outputWhiteLevel = levels


def ramps(hdr, stride=0):
    """[(ramp, reversed ramp)] per phase: computed once, shared, never modified."""
    if ("ramps", hdr, stride) not in _cache:
        _cache["ramps", hdr, stride] = [(f, M.partner_frame(f, hdr)) for f in (M.ramp_frame(hdr, p, stride=stride) for p in range(M.PHASES[hdr]))]
    return _cache["ramps", hdr, stride]


def device_rcp(hdr):
    """{levels: {y: v_rcp_f32(y)}} for the two values each setting takes the reciprocal of (at most 8 per setting fit the oracle's override)."""
    if ("rcp", hdr) not in _cache:
        ys = sorted({float(y) for lv in M.LEVELS for y in M.rcp_inputs(*lv, hdr)})
        c = context(hdr, 128)
        try:
            got = np.concatenate([c.deviceRcp(np.array(ys[i:i + 32], np.float32)) for i in range(0, len(ys), 32)])
        finally:
            c.close()
        table = dict(zip(ys, (float(r) for r in got)))
        _cache["rcp", hdr] = {lv: {float(y): table[float(y)] for y in M.rcp_inputs(*lv, hdr)} for lv in M.LEVELS}
    return _cache["rcp", hdr]


def use_rcp(hdr, levels):
    from oracle import oracle
    rcp = device_rcp(hdr)[levels]
    assert len(rcp) <= 8
    oracle.set_flavour(1, 1, rcp)
    return rcp


@ELEM
def test_device_reciprocals_are_within_one_ulp(native_lib, hdr):
    for lv, rcp in device_rcp(hdr).items():
        for y, r in rcp.items():
            exact = M.rcp_exact(y)
            near = (np.nextafter(exact, np.float32(-np.inf)), exact, np.nextafter(exact, np.float32(np.inf)))
            assert np.float32(r) in near, (lv, y, r, float(exact))
    if hdr:
        assert np.float32(device_rcp(1)[(0.0, 180.0)][46080.0]) == M.rcp_one_low(46080.0)


def vcase(hdr, max_res, w, si, so, levels):
    return V.Case("arith", hdr, M.H, w, si, so, max_res, 1, (1,), (2,), (0,), (0,), levels, ("uniform:0:0",), M.T, "single")


def expected_warps(hdr, w, si, so, levels, max_res=128):
    """{(phase, t): oracle.warp_frames at zero flow} at one setting, through the device's reciprocals; kept for the bodies that share a shape.
    (At zero flow the resolution scalar does not enter: the packed and the scalar body share these frames, checked once per shape.)"""
    from oracle import oracle
    key = ("warps", hdr, w, si, so, levels)
    if key not in _cache:
        use_rcp(hdr, levels)
        g = oracle.make_geom(hdr, M.H, w, si, so, max_res)
        flow = np.zeros((2, g.lh, g.lw), np.int16)
        src = ramps(hdr, si)
        jobs = [(p, t) for p in range(M.PHASES[hdr]) for t in M.T]
        res = _pool.map(lambda j: oracle.warp_frames(*src[j[0]], flow, g, np.float32(j[1]), 2, *levels), jobs)
        _cache[key] = dict(zip(jobs, res))
        if levels == M.LEVELS[1]:
            g0 = oracle.make_geom(hdr, M.H, w, si, so, 270)
            assert g0.rs == 0 and g.rs == 1
            assert np.array_equal(oracle.warp_frames(*src[0], np.zeros((2, g0.lh, g0.lw), np.int16), g0, np.float32(M.T[3]), 2, *levels), _cache[key][0, M.T[3]])
    return _cache[key]


def assert_frame(got, want, w, so, what):
    s = so or w
    got, want = got.reshape(-1, s), want.reshape(-1, s)
    bad = got[:, :w] != want[:, :w]
    assert not bad.any(), (what, int(bad.sum()), [(int(y), int(x), int(got[y, x]), int(want[y, x])) for y, x in np.argwhere(bad)[:6]])
    assert (got[:, w:].view(np.uint8) == 0xA5).all(), (what, "stride padding written")


def run_warp_body(hdr, max_res, label, w=M.W, si=0, so=0, out_off=0, single=True):
    """Mode 2 at zero flow at every entry of LEVELS and every blend scalar, phase by phase: a fused interpolateOnly of three outputs (twice) and,
    `single`, warpFrames per scalar.  `label`: what the variant model must say both launch."""
    dt = M.dtype(hdr)
    c = context(hdr, max_res, w, si, so)
    src = [[Buf(f.nbytes, 0) for f in pair] for pair in ramps(hdr, si)]
    outs = [Buf(c.output_frame_bytes, out_off) for _ in M.T]
    try:
        for pair, bufs in zip(ramps(hdr, si), src):
            for f, b in zip(pair, bufs):
                b.put(f)
        for lv in M.LEVELS:
            g = V.geometry(vcase(hdr, max_res, w, si, so, lv))
            assert (g.rs, g.lw, g.lh) == (c.m_opticalFlowResScalar, c.m_opticalFlowFrameWidth, c.m_opticalFlowFrameHeight)
            for i in (0, 3):
                fused = V.interpolate_member(g, 2, V.Member(3, M.T[i:i + 3], 0, out_off, "uniform:0:0"), lv)
                assert len(fused) == 1 and fused[0].label.startswith(label), (lv, fused)
            for t in M.T:
                assert V.launch_warp_t(g, 2, V.Member(1, (t,), 0, out_off, "uniform:0:0"), lv).startswith(label), (lv, t)
        for p, (a, b) in enumerate(src):
            for buf in (a, b, a):
                c.updateFrameDeviceRef(buf.ptr)
            c.sync()
            c.writeBlurredFlow(0, np.zeros((2, c.m_opticalFlowFrameHeight, c.m_opticalFlowFrameWidth), np.int16))
            for lv in M.LEVELS:
                want = expected_warps(hdr, w, si, so, lv)
                set_levels(c, lv)
                for how in (("fused", "single") if single else ("fused",)):
                    if how == "fused":
                        for i in (0, 3):
                            c.interpolateOnly(list(M.T[i:i + 3]), [o.ptr for o in outs[i:i + 3]], 2)
                    else:
                        for o, t in zip(outs, M.T):
                            c.setOutputBuffer(o.ptr)
                            c.warpFrames(t, 2)
                    c.sync()
                    for o, t in zip(outs, M.T):
                        assert_frame(o.get(dt), want[p, t], w, so, (label, how, hdr, p, lv, t))
                        o.reset()
    finally:
        c.setOutputBuffer(0)
        c.close()
        for b in outs + [x for pair in src for x in pair]:
            b.free()


@ELEM
def test_packed_body_over_every_code_value_and_setting(native_lib, hdr):
    """warp_finish_to.  On 16-bit frames it leans on v_cvt_u32_f32 clamping negatives to 0 and the pack saturating at 65535: 16 / 235 and
    200 / 100 hold elements on both sides (asserted from the model)."""
    if hdr:
        for lv in ((16.0, 235.0), (200.0, 100.0)):
            assert lv in M.LEVELS
            for cz in (0, 1):
                v = np.concatenate([M.levels_values(f, 1, *lv, cz).reshape(-1) for f, _ in ramps(1)])
                assert (v < 0).any() and (v > 65535).any(), (lv, cz)
    run_warp_body(hdr, 128, "fast.")


@ELEM
def test_scalar_body_over_every_code_value_and_setting(native_lib, hdr):
    """warp_element through warp_kernel: rs 0, a flow cell of one element."""
    run_warp_body(hdr, 270, "generic.%s.aligned" % ("u16" if hdr else "u8"))


@ELEM
def test_scalar_body_with_the_output_at_base_plus_2_bytes(native_lib, hdr):
    run_warp_body(hdr, 270, "generic.%s.unaligned" % ("u16" if hdr else "u8"), out_off=2, single=False)


@ELEM
def test_ragged_right_edge_of_the_fast_kernel(native_lib, hdr):
    """W = 510 in strides of 512 at rs 1: 8-byte threads (a small frame) hold 8 / 4 elements, 510 is a multiple of neither, so the last
    thread of a row goes element by element through warp_element while the others take the packed body."""
    vec = 8 // (2 if hdr else 1)
    assert 510 % vec != 0
    run_warp_body(hdr, 128, "fast.%s.vb8." % ("u16" if hdr else "u8"), w=510, si=512, so=512, single=False)


@ELEM
@pytest.mark.parametrize("src_off", [0, 2], ids=["aligned", "src2"])
def test_copy_kernel_over_every_code_value_and_setting(native_lib, hdr, src_off):
    from oracle import oracle
    dt = M.dtype(hdr)
    c = context(hdr, 270)
    g = oracle.make_geom(hdr, M.H, M.W, 0, 0, 270)
    vg = V.geometry(vcase(hdr, 270, M.W, 0, 0, (0.0, 255.0)))
    assert V.launch_copy_t(vg, V.Member(1, (0.0,), src_off, 0, "uniform:0:0")) == "copy.%s.%s" % ("u16" if hdr else "u8", "unaligned" if src_off else "aligned")
    src = [Buf(f.nbytes, src_off) for f, _ in ramps(hdr)]
    out = Buf(c.output_frame_bytes, 0)
    try:
        for (f, _), b in zip(ramps(hdr), src):
            b.put(f)
        c.setOutputBuffer(out.ptr)
        for p, b in enumerate(src):
            for _ in range(3):
                c.updateFrameDeviceRef(b.ptr)
            for lv in M.LEVELS:
                use_rcp(hdr, lv)
                set_levels(c, lv)
                c.copyFrame()
                c.sync()
                assert_frame(out.get(dt), oracle.copy_frame(ramps(hdr)[p][0], g, *lv), M.W, 0, ("copy", hdr, p, lv))
                out.reset()
    finally:
        c.setOutputBuffer(0)
        c.close()
        for b in src + [out]:
            b.free()


@ELEM
@pytest.mark.parametrize("strides", [(0, 0), (515, 517)], ids=["vector16", "element"])
def test_scene_copy_kernel_at_three_settings(native_lib, hdr, strides):
    """scene_copy_kernel: a fresh batch of two members per setting and pair of ramp phases, sceneSet, one runPeriodAuto -- the first period is
    a copy of the frame it is fed (m_frameCount < 3), so no cut clip is needed.  Aligned strides take the 16-byte path, 515 / 517 the element path."""
    from hopperrender_amd import capi
    from hopperrender_amd.calc import DeviceBuffer, FlowBatch
    from oracle import oracle
    si, so = strides
    case = (hdr, M.H, M.W, si, so)
    g = oracle.make_geom(hdr, M.H, M.W, si, so, 270)
    frames = [f for f, _ in ramps(hdr, si)]
    dev = []
    for f in frames:
        b = DeviceBuffer(f.nbytes)
        b.upload(f)
        dev.append(b)
    vec = 16 // (2 if hdr else 1)
    assert (g.in_stride % vec == 0 and g.out_stride % vec == 0) == (strides == (0, 0)) and all(b.ptr % 16 == 0 for b in dev) and GUARD % 16 == 0
    rounds = -(-len(frames) // 2)
    phase = lambda m, k: (2 * k + m) % len(frames)
    assert {phase(m, k) for m in (0, 1) for k in range(rounds)} == set(range(len(frames)))
    scalars = [[0.5], [0.25, 0.75]]
    try:
        for lv, k in [(lv, k) for lv in M.SCENE_LEVELS for k in range(rounds)]:
            use_rcp(hdr, lv)
            members = [calc_class(hdr)(M.H, M.W, si, so, 8, 6, lv[0], lv[1], 270, search_radius=5,
                                       flags=capi.HF_FLAG_ASYNC | (capi.HF_FLAG_BATCH_EAGER_PLANES if i == 0 else 0)) for i in range(2)]
            batch = FlowBatch(members)
            outs = [Outputs(c) for c in members]
            try:
                assert not batch.defersPlanes()
                for m in range(2):
                    batch.sceneSet(m, 417083, -1)
                batch.runPeriodAuto([dev[phase(m, k)].ptr for m in range(2)], scalars, [outs[m].new(len(scalars[m])) for m in range(2)], 2)
                batch.sync()
                for m in range(2):
                    recs = batch.sceneRead(m)
                    assert [(r["frame_count"], r["kind"]) for r in recs] == [(1, 0)], recs
                    got = outs[m].read(case)                                     # (asserts the sentinels around every frame)
                    want = oracle.copy_frame(frames[phase(m, k)], g, *lv).reshape(-1, g.out_stride)[:, :M.W]
                    assert len(got[0]) == len(scalars[m])
                    for j, frame in enumerate(got[0]):
                        bad = frame != want
                        assert not bad.any(), (hdr, strides, lv, m, k, j, int(bad.sum()), [(int(y), int(x), int(frame[y, x]), int(want[y, x])) for y, x in np.argwhere(bad)[:6]])
                    for b in outs[m].bufs[0]:
                        raw = b.download(np.uint8)[GUARD:-GUARD].view(M.dtype(hdr)).reshape(-1, g.out_stride)
                        assert (raw[:, M.W:].view(np.uint8) == 0xA5).all(), "stride padding written"
            finally:
                batch.close()
                for c in members:
                    c.close()
                for o in outs:
                    o.free()
    finally:
        for b in dev:
            b.free()


@ELEM
@pytest.mark.parametrize("rs", [1, 3], ids=["rs1-gain4", "rs3-gain1"])
def test_flow_views_over_direction_magnitude_and_gain(native_lib, rs, hdr):
    """Modes 3 and 4 on constant frames at t = 0 (`blended` is the constant whatever the gather does), levels 0 / 255, the flow domain injected
    field by field.  Mode 4: bit-exact against the model and the oracle.  Mode 3: every element in the model's accepted set."""
    from oracle import oracle
    dt = M.dtype(hdr)
    lv = (0.0, 255.0)
    rcp = use_rcp(hdr, lv)
    fg = M.FLOW_GEOMS[rs]
    g = oracle.make_geom(hdr, M.H, M.W, 0, 0, fg.max_res)
    c = context(hdr, fg.max_res)
    assert (g.rs, g.lw, g.lh) == fg[:3] == (c.m_opticalFlowResScalar, c.m_opticalFlowFrameWidth, c.m_opticalFlowFrameHeight)
    vectors = M.flow_domain(rs).astype(np.int64)
    m3, m4 = M.view_tables(rs, hdr, rcp=rcp)
    single = (m3[0] == m3[1]) & (m3[1] == m3[2])
    assert single.all(0).mean() >= 0.97
    frame = M.const_frame(hdr)
    src = Buf(frame.nbytes, 0)
    outs = [Buf(c.output_frame_bytes, 0) for _ in (3, 4)]
    fields = M.flow_fields(rs)
    want4 = list(_pool.map(lambda f: oracle.warp_frames(frame, frame, f[0], g, np.float32(0.0), 4, *lv), fields))
    try:
        src.put(frame)
        for _ in range(3):
            c.updateFrameDeviceRef(src.ptr)
        c.sync()
        for k, (field, idx) in enumerate(fields):
            which, channel = M.seen(rs, idx)
            c.writeBlurredFlow(0, field)
            for o, mode in zip(outs, (3, 4)):
                c.setOutputBuffer(o.ptr)
                c.warpFrames(0.0, mode)
            c.sync()
            got3, got4 = (o.get(dt).reshape(which.shape) for o in outs)
            assert np.array_equal(got4, m4[channel, which]) and np.array_equal(got4.reshape(-1), want4[k]), (rs, hdr, k, "mode 4")
            ok = (m3[:, channel, which] == got3[None]).any(0)
            if not ok.all():
                rows = sorted({(int(vectors[which[y, x], 0]), int(vectors[which[y, x], 1]), int(channel[y, x]), int(got3[y, x]),
                                tuple(int(a) for a in m3[:, channel[y, x], which[y, x]])) for y, x in np.argwhere(~ok)})
                raise AssertionError(f"mode 3 outside the accepted set, rs {rs} hdr {hdr} field {k}: {len(rows)} (vx, vy, channel, device, accepted): {rows[:40]}")
            for o in outs:
                o.reset()
    finally:
        c.setOutputBuffer(0)
        c.close()
        for b in outs + [src]:
            b.free()
