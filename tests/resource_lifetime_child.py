"""Child process of tests/test_resource_lifetime_gpu.py: runs ONE scenario in a fresh process -- hf_debug_live_resources counts per
process, so the counts start at zero and no object another test left alive disturbs them -- and prints one JSON object on its last
line.  Every native call goes through capi.check / FlowBatch._check, which raise on any error code: "error" in the result is the first
one, or null.  All shapes are 180 x 320 at the default max_calc_res.

    python tests/resource_lifetime_child.py everything | cycles | in_flight
"""
import json
import os
import sys
import traceback

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

import planar_ref                                                   # noqa: E402
from hopperrender_amd import capi, synth                            # noqa: E402
from hopperrender_amd.calc import (DeviceBuffer, FlowBatch, OpticalFlowCalcHDR, OpticalFlowCalcSDR, PinnedArray)   # noqa: E402

H, W, R = 180, 320, 8
A, DUAL, PROFILE = capi.HF_FLAG_ASYNC, capi.HF_FLAG_DUAL_STREAM, capi.HF_FLAG_PROFILE
live = capi.live_resources


def device_frame(a):
    a = np.ascontiguousarray(a)
    b = DeviceBuffer(a.nbytes)
    b.upload(a)
    return b


def lone_planar_context(res):
    """A blocking planar context through every lazily allocated resource of a context."""
    c = OpticalFlowCalcSDR(H, W, search_radius=R, flags=PROFILE | capi.HF_FLAG_PLANAR_IN | capi.HF_FLAG_PLANAR_OUT)
    sc = synth.Scene(H, W, False, 3)
    planar = [planar_ref.semiplanar_to_planar(sc.frame(k), H, W, W, False) for k in range(4)]
    for k in range(3):
        c.updateFrame(planar[k])                                    # in_stage
    c.calculateOpticalFlow()                                        # a graph
    outs = [DeviceBuffer(c.output_frame_bytes) for _ in range(7)]
    c.interpolatePeriod(None, [(i + 1) / 8 for i in range(7)], [o.ptr for o in outs])   # six period stages, two chunks
    c.downloadFrame()                                               # out_stage
    pin_in, pin_out = PinnedArray(planar[3].size, np.uint8), PinnedArray(c.output_frame_bytes, np.uint8)
    pin_in.array[:] = planar[3]
    c.updateFrameAsync(pin_in)                                      # side streams, their events, output-ring slots 1 and 2
    c.calculateOpticalFlow()
    c.warpFrames(0.5, 2)
    c.downloadFrameAsync(pin_out)
    c.sync()
    before = res["alive_context"] = live()                          # (ahead of the counters: switching them drops the cached graphs)
    c.countersEnable(True)
    on = live()
    c.countersEnable(False)
    off = live()
    res["counters"] = {"before": before, "on": on, "off": off}
    c.frameError(outs[0].ptr, outs[1].ptr, planar=True)             # error slots
    res["profile"] = c.profile()                                    # spans and their pooled events
    c.close()
    for x in outs:
        x.free()
    pin_in.free()
    pin_out.free()


def batch_then_plain_period(res, dual):
    """Three HF_FLAG_ASYNC contexts through a batch that is destroyed right behind its last enqueue, then one plain period on each former
    member's own stream against a never-batched twin fed the same frames."""
    n, periods, ts = 3, 5, [0.3, 0.7]
    planar = not dual                                               # (the planar sides and HF_FLAG_DUAL_STREAM members do not combine)
    leader = (capi.HF_FLAG_BATCH_PLANAR_IN | capi.HF_FLAG_BATCH_PLANAR_OUT | capi.HF_FLAG_BATCH_AUTO_DEFERRED) if planar else 0
    cs = [OpticalFlowCalcSDR(H, W, search_radius=R, flags=A | (DUAL if dual else 0) | (leader if m == 0 else 0)) for m in range(n)]
    twins = [OpticalFlowCalcSDR(H, W, search_radius=R) for _ in range(n)]
    nv = [[synth.Scene(H, W, False, 11 + m).frame(k) for k in range(periods + 1)] for m in range(n)]
    given = [[planar_ref.semiplanar_to_planar(f, H, W, W, False) if planar else f for f in nv[m][:periods]] for m in range(n)]
    seen = [[planar_ref.planar_to_semiplanar(f, H, W, W, False) if planar else f for f in given[m]] for m in range(n)]   # what the ring holds
    frames = [[device_frame(f) for f in given[m]] for m in range(n)]
    outs = [[DeviceBuffer(cs[0].output_frame_bytes) for _ in ts] for _ in range(n)]
    out_ptrs = [[o.ptr for o in row] for row in outs]
    b = FlowBatch(cs)
    b.timelineEnable(32, 0)
    for m in range(n):
        b.sceneSet(m, 417083)
    for k in range(periods):
        ptrs = [frames[m][k].ptr for m in range(n)]
        if dual:                                                    # the three separate calls
            b.updateFramesDeviceRef(ptrs)
            b.calculateOpticalFlow()
            b.interpolatePeriod([ts] * n, out_ptrs)
        elif k < periods - 1:
            b.runPeriodAuto(ptrs, [ts] * n, out_ptrs)
        else:
            b.runPeriod(b.preparePeriod(ptrs, [ts] * n, out_ptrs))
    res["alive_dual_batch" if dual else "alive_planar_batch"] = live()
    b.close()                                                       # right behind the last enqueue: the caller has not synchronised
    same = True
    for m in range(n):
        last, out, twin_out = device_frame(nv[m][periods]), DeviceBuffer(cs[m].output_frame_bytes), DeviceBuffer(cs[m].output_frame_bytes)
        cs[m].interpolatePeriod(last.ptr, [0.5], [out.ptr])
        cs[m].sync()
        t = twins[m]
        for k in range(periods):
            t.updateFrame(seen[m][k])
            # (a period of hf_batch_run_period_auto keeps the flow of a context whose m_frameCount is below 3, as the filter would)
            if dual or k == periods - 1 or t.m_frameCount >= 3:
                t.calculateOpticalFlow()
        t.interpolatePeriod(last.ptr, [0.5], [twin_out.ptr])
        same = same and bool((out.download(np.uint8) == twin_out.download(np.uint8)).all())
        for x in (last, out, twin_out):
            x.free()
    res["dual_members_equal_twins" if dual else "planar_members_equal_twins"] = same
    for c in cs + twins:
        c.close()
    for x in [f for row in frames for f in row] + [o for row in outs for o in row]:
        x.free()


def everything(res):
    res["start"] = live()
    lone_planar_context(res)
    res["after_context"] = live()
    batch_then_plain_period(res, dual=False)
    batch_then_plain_period(res, dual=True)
    res["end"] = live()


def one_cycle(i):
    """tools/leak_check.py's loop: a context, and a batch of three around contexts; SDR / HDR and single / dual stream alternate."""
    hdr, dual = bool(i & 1), bool(i & 2)
    cls = OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR
    f = synth.random_frame(H, W, hdr, 1 + i)
    ts = [0.2, 0.5, 0.8]
    lone = cls(H, W, search_radius=R)
    outs = [DeviceBuffer(lone.output_frame_bytes) for _ in ts]
    for _ in range(3):
        lone.updateFrame(f)
    lone.calculateOpticalFlow()
    lone.interpolateOnly(ts, [o.ptr for o in outs])
    lone.close()
    cs = [cls(H, W, search_radius=R, flags=A | (DUAL if dual else 0)) for _ in range(3)]
    b = FlowBatch(cs)
    for c in cs:
        for _ in range(3):
            c.updateFrame(f)
    b.calculateOpticalFlow()
    for c in cs:
        c.interpolateOnly(ts, [o.ptr for o in outs])
    for c in cs:
        c.sync()
    b.close()
    for c in cs:
        c.close()
    for o in outs:
        o.free()


def cycles(res):
    res["start"] = live()
    res["after_cycle"] = []
    for i in range(20):
        one_cycle(i)
        res["after_cycle"].append(live())


def in_flight(res):
    """hf_destroy / hf_batch_destroy directly behind enqueued work (the caller never synchronises), then a fresh context against the oracle."""
    from oracle import oracle
    res["start"] = live()
    sc = synth.Scene(H, W, False, 21)
    f = [sc.frame(k) for k in range(3)]
    dev = [device_frame(x) for x in f]
    ts = [0.25, 0.5, 0.75]
    outs = [DeviceBuffer(H * W * 3 // 2) for _ in ts]
    c = OpticalFlowCalcSDR(H, W, search_radius=R, flags=A)
    for d in dev[:2]:
        c.updateFrameDevice(d.ptr)
    c.interpolatePeriod(dev[2].ptr, ts, [o.ptr for o in outs])      # update, chain and the period's warps enqueued ...
    c.close()                                                       # ... and the context closed behind them
    cs = [OpticalFlowCalcSDR(H, W, search_radius=R, flags=A) for _ in range(3)]
    b = FlowBatch(cs)
    for d in dev[:2]:
        b.updateFramesDeviceRef([d.ptr] * 3)
    b.runPeriod(b.preparePeriod([dev[2].ptr] * 3, [ts[:1]] * 3, [[o.ptr] for o in outs]))
    b.close()
    for m in cs:
        m.close()
    res["after_destroys"] = live()
    g = oracle.make_geom(0, H, W)
    off_o, blur_o, tot_o, oob = oracle.calculate_optical_flow(f[1], f[2], g, R)
    n = OpticalFlowCalcSDR(H, W, search_radius=R)
    for x in f:
        n.updateFrame(x)
    n.calculateOpticalFlow()
    flow_ok = oob == 0 and bool((n.readOffsets() == off_o).all() and (n.readBlurredFlow(1) == blur_o).all()) and n.m_totalFrameDelta == tot_o
    n.calculateOpticalFlow()                                        # the same pair again: the previous flow is this flow
    n.warpFrames(0.5994, 2)
    res["period_bit_exact"] = flow_ok and bool((n.downloadFrame() == oracle.warp_frames(f[0], f[1], blur_o, g, 0.5994, 2)).all())
    n.close()
    for x in dev + outs:
        x.free()
    res["end"] = live()


if __name__ == "__main__":
    result = {"error": None}
    try:
        {"everything": everything, "cycles": cycles, "in_flight": in_flight}[sys.argv[1]](result)
    except Exception:
        result["error"] = traceback.format_exc()
    print(json.dumps(result))
