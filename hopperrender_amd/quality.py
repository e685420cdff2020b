"""Leave-one-out interpolation quality of a clip, measured on the device.

    python -m hopperrender_amd.quality clip.y4m [--radius 16] [--sweep radius=5,16 --sweep blur=4,32] [--ssim] [--map 16] [--ssim-map 16] [--map-dir DIR]
                                       [--disagreement 16] [--report out.json]
    python -m hopperrender_amd.quality clip.y4m --confidence --target-fps 59.94 [--disagreement 16] [--report out.json]
    python -m hopperrender_amd.quality clip.nv12 --width 1920 --height 1080 [--hdr | --pix-fmt yuv420p10le] ...

Every second frame of the clip is withheld: the sources S_j = frames[2 j] go through one asynchronous context exactly as a filter would
feed them (hf_interpolate_period on device frames, ONE output at t = 0.5, blended mode), and what comes out for the pair (S_p, S_p+1) is
compared with the withheld frame T_p = frames[2 p + 1] between them.  That is the only question the six knobs that change the picture
(search radius, delta and neighbour scalar, blur radius, iterations, calculation resolution) can be asked without a reference to copy.

Which period shows which pair follows the filter's gating (protocol.FilterReplay.deliver, HopperRender.cpp:955,1179): a flow is only
calculated once three frames have arrived, and the period of source S_j shows the pair (S_j-2, S_j-1) with the flow calculated ONE period
earlier.  So pair 0 is shown before any flow exists -- it is listed as warm-up and not evaluated -- and the last source is submitted once
more so that the last pair is reached (schedule()).

Outputs carry the context's levels (HDR: the x 65535 / 65280 stretch of the default 0 .. 255 levels), so the truth of a pair is the
withheld frame through copyFrame's arithmetic at the same levels, from a second context; the baseline "frame repeat" is copyFrame of the
pair's first source against the same truth.  The comparison itself is the device's integer frame error (hf_frame_error_enqueue:
sum of squared / absolute differences, largest difference, differing elements per plane, padding excluded), enqueued straight behind
each period with no host sync and read once per chunk of 128 pairs -- once at the end for any ordinary clip.

The report is a plain dict (json.dump-able): per evaluated pair and plane the integer sums and psnr = 10 log10(peak^2 count / sse)
(peak 255 or 65535; None where sse == 0) for the interpolation and for the repeat baseline, clip aggregates (PSNR of the summed sse, the
worst pair), the settings, and -- on request -- what the filter's scene-change detection would have made of each period.

--ssim / evaluate(ssim=True) adds the windowed SSIM (hf_frame_ssim_enqueue: 8 x 8 windows at stride 4, the block form of x264 and of FFmpeg's
ssim filter, in integers) beside every error sum, on the same pairs and slot numbers, read once per chunk like them.  PSNR alone rewards
smoothing -- a larger blur radius, or a blend that averages two frames, trades a sharp and slightly misplaced edge for a ghost and the
squared error falls -- and cannot tell a frame a little wrong everywhere from one torn in a single place; SSIM is the second judge for
exactly the knobs a sweep turns.  Per plane the report gains sum_loss_q32, max_loss_q32, count (loss = 2^32 - round(ssim 2^32) per window)
and the floats ssim = 1 - sum / 2^32 / count (the mean) and min_ssim = 1 - max / 2^32 (the worst window), None where there is no window;
the clip aggregates are summed loss over summed count and the largest loss; gain_ssim_y per pair and for the clip is interpolation
minus repeat, and clip["worst_pair_ssim"] names the pair with the lowest mean Y.  Without it the report is what it was.

--map TILE / evaluate(error_map=TILE) says WHERE in the picture the error sits (TILE = 16, 32 or 64 luma pixels): behind each evaluated
pair's error launch the per-tile map of the interpolation against the truth (hf_frame_error_map_enqueue: sse, sad, max_abs per tile and
plane) is enqueued into one device buffer per chunk, which is read once per chunk like the sums -- 48 bytes per tile, not the frames.
Each pair's "interpolated" dict gains "map": tile, shape [th, tw], and per plane "worst" -- the five tiles of largest sse as {x, y, sse,
max_abs}, x and y the luma pixels of the tile's corner, ties by lower y and then lower x -- and "share_top1pct", the share of the
plane's sse that its ceil(tiles / 100) worst tiles hold (1.0: the error is one tear; about 0.01: it is spread evenly; None where sse is
0).  clip["worst_tile"] names pair, plane Y, x, y and sse of the worst luma tile of the clip.  --map-dir DIR / evaluate(map_dir=DIR)
also writes one 8-bit PGM per evaluated pair (map_pair0001.pgm ...): the Y plane, one pixel per tile, sqrt(sse / count) scaled so that
the clip's largest value is 255; that is host work on the maps already read.  Without --map none of this is called or reported.

--ssim-map TILE / evaluate(ssim_map=TILE) says where the STRUCTURE is worst: the error map holds squared and absolute error, the judge
that a ghost passes, and --ssim gives the score of the worst window but not its place.  Behind each evaluated pair's error launch the
per-tile SSIM map of the interpolation against the truth (hf_frame_ssim_map_enqueue: summed and largest window loss and window count
per tile and plane, a window belonging to the tile of its first element) goes into a device buffer of its own per chunk, read once per
chunk -- 72 bytes per tile.  It is independent of --ssim and --map and uses the error map's tile grid.  Each pair's "interpolated"
dict gains "ssim_map": tile, shape [th, tw], and per plane "worst" -- the five tiles of lowest mean SSIM (largest sum_loss_q32 / count,
compared as integers; ties by lower y and then lower x; tiles without a window left out) as {x, y, ssim, min_ssim, sum_loss_q32,
max_loss_q32, count}, with "sse" of the same tile beside them where --map runs at the same tile size -- and "worst_window_tile",
{x, y, max_loss_q32} of the tile that holds the plane's worst window (None in a plane without windows).  clip["worst_tile_ssim"] names
pair, plane Y, x, y and mean SSIM of the clip's worst luma tile.  With --map-dir one more PGM per evaluated pair (ssim_pair0001.pgm ...):
the Y plane, one pixel per tile, round(255 min(1, sum_loss_q32 / count / 2^32)), 0 where count is 0 -- an absolute scale, so maps of
different pairs and clips compare.  Without --ssim-map none of this is called, allocated or reported.

--disagreement TILE / evaluate(disagreement=TILE) puts the one judge that needs no truth beside the ones that do: an output is blended
from two warped halves, frame N-2 pushed forward by t and frame N-1 pulled back by 1 - t, and where the flow is wrong the two differ.
Straight behind each evaluated pair's period, before the next period moves the ring, the disagreement map at t = 0.5
(hf_warp_disagreement_map_enqueue: sse, sad, max_abs of the two halves' difference per tile and plane, one launch, no frame written) goes
into a device buffer of its own per chunk, read once per chunk.  Each pair's "interpolated" dict gains "disagreement": the shape of
"map" -- tile, shape, and per plane "worst" and "share_top1pct" -- and per plane the totals sse, sad, max_abs; where --map runs at the
same tile size each plane also carries "overlap_top1pct": with k = ceil(tiles / 100), how many of the k worst tiles of the error map
are among the k worst of the disagreement map (both in the order of "worst"), over k -- how well disagreement predicts where the real
error is; None where either plane's sse is 0.  clip["disagreement"][plane] holds the summed sse and the hits summed over the k's summed
of the pairs where that is defined, clip["worst_tile_disagreement"] is worst_tile's twin, and --map-dir gains dis_pair0001.pgm ... by
the rule of the error maps' PGMs, scaled to their own clip maximum.  Without the option none of this is called, allocated or reported.

--confidence --target-fps F / confidence() is that judge ON ITS OWN, on every frame of the clip at the real output schedule: nothing is
withheld, frame j is the source of period j, the t's of a period are those of protocol.BlendSchedule(source, target).plan, the period is
submitted with no outputs (update and flow only) and the disagreement maps of its t's are enqueued behind it -- no output frame exists
in this mode.  Gating as above: nothing before a flow exists, the pair shown before any flow is listed as warm-up, the last frame is
submitted once more.  The report has per period the pair, the t's and per t and plane sse, sad, max_abs, rms = sqrt(sse / count) and
the worst tile; per clip the plane totals, the worst (period, t) by the rms of Y and the per-period mean rms of Y as a list.  The maps
are read once per chunk, a chunk being the periods whose maps fit CONFIDENCE_MAP_BYTES and whose sources fit CONFIDENCE_SOURCE_BYTES.
On the command line --confidence takes the flow settings, --disagreement TILE and --sweep; the options of the leave-one-out run
(--ssim, --map, --ssim-map, --map-dir, --guard, --detect-cuts, --black, --white) are refused beside it.

--guard TILE:LO:HI / evaluate(guard=(tile, lo_q4, hi_q4)) asks whether ACTING on that confidence helps on this clip: straight behind each
evaluated pair's period the withheld frame is produced a second time by hf_guarded_blend_enqueue at t = 0.5 (the blend, faded into the
plain cross-fade of the two source frames where a tile's mean luma disagreement lies between LO and HI sixteenths of an 8-bit code) and
judged against the same truth by every metric the run asked for.  Each pair gains "guarded" -- the plane dicts of "interpolated", with
"map" / "ssim_map" where those run, and "mask": tiles, tiles_firing (tile weight above 0) and mean_weight (0 .. 1 over the luma
pixels) -- and "guard_gain_db", guarded minus plain PSNR of Y (with --ssim also "guard_gain_ssim"); the clip gains the same from the
summed errors, and the report "guard".  A chunk then holds two thirds of the pairs (a third result slot each).  With --map-dir the luma
mask of every pair is written as guard_pair0001.pgm ..., one pixel per luma pixel, min(w, 255).  There are no default thresholds:
nobody has measured good ones; (4080, 4081) is guard off.  Without the option none of this is called, allocated or reported.
"""
import argparse
import itertools
import json
import math
import os
import sys

PLANES = ("Y", "U", "V")
SUMS = ("sse", "sad", "max_abs", "n_differ", "count")
SSIM_SUMS = ("sum_loss_q32", "max_loss_q32", "count")
SETTINGS = {"search_radius": 16, "delta_scalar": 8, "neighbor_scalar": 6, "blur_radius": 0, "iterations": 0, "max_calc_res": 270}
PAIRS_PER_READ = 128   # two result slots per pair (interpolation, repeat) out of HF_ERROR_SLOTS
CONFIDENCE_MAP_BYTES = 32 << 20   # confidence(): device bytes of disagreement maps between two reads (2160p at tile 16: 10 periods of 2 or 3 outputs)
CONFIDENCE_SOURCE_BYTES = 512 << 20   # ... and device bytes of a chunk's sources, which are all uploaded before it is submitted (2160p HDR: 21 periods)
MAX_DISAGREEMENT_OUTPUTS = 24    # blending scalars of one hf_warp_disagreement_map_enqueue launch


def psnr(sse, count, peak):
    """10 log10(peak^2 count / sse) in dB; None where the frames are equal (or nothing was compared)."""
    if sse == 0 or count == 0:
        return None
    return 10.0 * math.log10(float(peak) * float(peak) * float(count) / float(sse))


def schedule(n_frames):
    """The periods of a leave-one-out run over n_frames frames: one dict per call the evaluator makes, in order --
         period        j
         source_frame  index of the frame submitted (frames[2 j]; the last source once more at the end)
         flow          a flow is calculated (the filter's gating: from the third frame on)
         pair          the pair (S_pair, S_pair+1) the period's output shows, None before there is one
         truth_frame   index of the withheld frame between them
         evaluated     False for pair 0, which is shown before any flow has been calculated (warm-up)"""
    n_src = (n_frames + 1) // 2
    if n_src < 3:
        raise ValueError(f"leave-one-out needs at least 5 frames (3 sources), got {n_frames}")
    out = []
    for j in range(n_src + 1):
        pair = j - 2 if j >= 2 else None
        out.append({"period": j, "source_frame": 2 * min(j, n_src - 1), "flow": j >= 2, "pair": pair,
                    "truth_frame": None if pair is None else 2 * pair + 1, "evaluated": pair is not None and pair >= 1})
    return out


class _Device:
    """What evaluate() needs of the library: calculators and device buffers (a test hands in a recording fake)."""

    def __init__(self, device_index=0):
        self.device_index = device_index

    def calc(self, hdr, H, W, black, white, settings):
        from . import capi
        from .calc import OpticalFlowCalcHDR, OpticalFlowCalcSDR
        return (OpticalFlowCalcHDR if hdr else OpticalFlowCalcSDR)(
            H, W, 0, 0, settings["delta_scalar"], settings["neighbor_scalar"], black, white, settings["max_calc_res"],
            device_index=self.device_index, iterations=settings["iterations"], blur_radius=settings["blur_radius"],
            search_radius=settings["search_radius"], flags=capi.HF_FLAG_ASYNC)

    def buffer(self, nbytes):
        from .calc import DeviceBuffer
        return DeviceBuffer(nbytes, self.device_index)

    def scene_filter(self, source_frame_time, threshold):
        from .protocol import NativeFilter
        return NativeFilter(source_frame_time, scene_change_threshold=threshold)


def _with_psnr(err, peak):
    return {p: dict({k: int(err[p][k]) for k in SUMS}, psnr=psnr(err[p]["sse"], err[p]["count"], peak)) for p in PLANES}


def _aggregate(rows, key, peak):
    out = {}
    for p in PLANES:
        sse, cnt = sum(r[key][p]["sse"] for r in rows), sum(r[key][p]["count"] for r in rows)
        out[p] = {"sse": sse, "sad": sum(r[key][p]["sad"] for r in rows), "max_abs": max(r[key][p]["max_abs"] for r in rows),
                  "n_differ": sum(r[key][p]["n_differ"] for r in rows), "count": cnt, "psnr": psnr(sse, cnt, peak)}
    return out


def _ssim_floats(total, worst, count):
    return {"ssim": 1.0 - total / 4294967296.0 / count if count else None, "min_ssim": 1.0 - worst / 4294967296.0 if count else None}


def _add_ssim(planes, got):
    """the SSIM integers of one slot and the floats derived from them, into a pair's plane dicts (their "count" stays the elements compared)"""
    for p in PLANES:
        total, worst, count = (int(got[p][k]) for k in SSIM_SUMS)
        planes[p].update({"sum_loss_q32": total, "max_loss_q32": worst, "ssim_count": count}, **_ssim_floats(total, worst, count))


def _add_ssim_aggregate(agg, rows, key):
    for p in PLANES:
        total, count = sum(r[key][p]["sum_loss_q32"] for r in rows), sum(r[key][p]["ssim_count"] for r in rows)
        worst = max(r[key][p]["max_loss_q32"] for r in rows)
        agg[p].update({"sum_loss_q32": total, "max_loss_q32": worst, "ssim_count": count}, **_ssim_floats(total, worst, count))


def _worst_tiles(m, tile, k=5):
    """the k tiles of largest sse of one plane's map [th][tw] (calc.frame_error_maps): ties by lower y, then lower x"""
    import numpy as np
    tw = m.shape[1]
    order = np.argsort(-m["sse"].astype(np.int64).reshape(-1), kind="stable")[:k]   # (a tile's sse stays below 2^44)
    return [{"x": int(i % tw) * tile, "y": int(i // tw) * tile, "sse": int(m["sse"].flat[i]), "max_abs": int(m["max_abs"].flat[i])} for i in order]


def _share_top1pct(m):
    """share of the plane's sse held by its ceil(tiles / 100) worst tiles; None where the sse is 0"""
    sse = sorted((int(v) for v in m["sse"].flat), reverse=True)
    total = sum(sse)
    return None if total == 0 else sum(sse[:(len(sse) + 99) // 100]) / total


def _map_dict(m, tile):
    """one pair's map [3][th][tw] as the report's "map" entry"""
    return dict({"tile": tile, "shape": [int(m.shape[1]), int(m.shape[2])]},
                **{p: {"worst": _worst_tiles(m[i], tile), "share_top1pct": _share_top1pct(m[i])} for i, p in enumerate(PLANES)})


def _top1pct(m, tile):
    """the ceil(tiles / 100) worst tiles of one plane's map, in the order of _worst_tiles, as (y, x) in tiles"""
    return [(t["y"] // tile, t["x"] // tile) for t in _worst_tiles(m, tile, (m.size + 99) // 100)]


def _overlap_top1pct(err, dis, tile):
    """(hits, k): how many of the k = ceil(tiles / 100) worst tiles of the error map's plane are among the k worst of the disagreement
    map's; None where either plane's sse is 0"""
    if not int(err["sse"].astype(object).sum()) or not int(dis["sse"].astype(object).sum()):
        return None
    a, b = _top1pct(err, tile), _top1pct(dis, tile)
    return len(set(a) & set(b)), len(a)


def _plane_totals(m):
    """sse, sad, max_abs of one plane's map as plain ints"""
    return {"sse": int(m["sse"].astype(object).sum()), "sad": int(m["sad"].astype(object).sum()), "max_abs": int(m["max_abs"].max())}


def _disagreement_dict(m, tile, overlap=None):
    """one pair's disagreement map [3][th][tw] as the report's "disagreement" entry; overlap: per plane _overlap_top1pct against the
    pair's error map at the same tile, or None where there is no such map"""
    out = _map_dict(m, tile)
    for i, p in enumerate(PLANES):
        out[p].update(_plane_totals(m[i]))
        if overlap is not None:
            out[p]["overlap_top1pct"] = None if overlap[i] is None else overlap[i][0] / overlap[i][1]
    return out


def _write_map_pgms(map_dir, luma, tile, H, W, prefix="map"):
    """luma: [(pair, Y map [th][tw])] -> one binary PGM per pair, sqrt(sse / count) per tile scaled to the largest value of the clip"""
    import numpy as np
    os.makedirs(map_dir, exist_ok=True)
    th, tw = luma[0][1].shape
    rows = np.minimum((np.arange(th) + 1) * tile, H) - np.arange(th) * tile
    cols = np.minimum((np.arange(tw) + 1) * tile, W) - np.arange(tw) * tile
    rms = [np.sqrt(m["sse"].astype(np.float64) / np.outer(rows, cols)) for _, m in luma]
    top = max(float(r.max()) for r in rms)
    for (pair, _), r in zip(luma, rms):
        with open(os.path.join(map_dir, f"{prefix}_pair{pair:04d}.pgm"), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (tw, th))
            f.write(np.rint(r * (255.0 / top) if top > 0 else r).astype(np.uint8).tobytes())


def _ssim_tile_order(m):
    """the tiles of one plane's SSIM map [th][tw] that own a window, as (sum, count, y, x), lowest mean SSIM first: largest sum / count
    by cross-multiplication (integers: a float quotient could order 6 / 2 and 3 / 1 either way), ties by lower y, then lower x"""
    import functools
    tiles = [(int(m["sum_loss_q32"][y, x]), int(m["count"][y, x]), y, x) for y in range(m.shape[0]) for x in range(m.shape[1]) if m["count"][y, x]]
    def cmp(a, b):
        l, r = a[0] * b[1], b[0] * a[1]
        return -1 if l > r else 1 if l < r else (a[2:] > b[2:]) - (a[2:] < b[2:])
    return sorted(tiles, key=functools.cmp_to_key(cmp))


def _worst_ssim_tiles(m, tile, sse=None, k=5):
    """the k tiles of lowest mean SSIM of one plane's SSIM map; sse: the same plane of an error map of the same tile size, or None"""
    out = []
    for total, count, y, x in _ssim_tile_order(m)[:k]:
        worst = int(m["max_loss_q32"][y, x])
        out.append(dict({"x": x * tile, "y": y * tile}, **_ssim_floats(total, worst, count), sum_loss_q32=total, max_loss_q32=worst, count=count))
        if sse is not None:
            out[-1]["sse"] = int(sse["sse"][y, x])
    return out


def _worst_window_tile(m, tile):
    """the tile that holds the plane's largest window loss (ties by lower y, then lower x); None in a plane without a window"""
    best = None
    for y in range(m.shape[0]):
        for x in range(m.shape[1]):
            if m["count"][y, x] and (best is None or int(m["max_loss_q32"][y, x]) > best["max_loss_q32"]):
                best = {"x": x * tile, "y": y * tile, "max_loss_q32": int(m["max_loss_q32"][y, x])}
    return best


def _ssim_map_dict(m, tile, err=None):
    """one pair's SSIM map [3][th][tw] as the report's "ssim_map" entry; err: the pair's error map at the same tile size, or None"""
    return dict({"tile": tile, "shape": [int(m.shape[1]), int(m.shape[2])]},
                **{p: {"worst": _worst_ssim_tiles(m[i], tile, None if err is None else err[i]), "worst_window_tile": _worst_window_tile(m[i], tile)}
                   for i, p in enumerate(PLANES)})


def _write_ssim_pgms(map_dir, luma):
    """luma: [(pair, Y SSIM map [th][tw])] -> one binary PGM per pair: round(255 min(1, mean loss / 2^32)) per tile, 0 without a window"""
    import numpy as np
    os.makedirs(map_dir, exist_ok=True)
    for pair, m in luma:
        th, tw = m.shape
        cnt = m["count"].astype(np.float64)
        loss = np.where(cnt > 0, m["sum_loss_q32"].astype(np.float64) / np.maximum(cnt, 1.0) / 4294967296.0, 0.0)
        with open(os.path.join(map_dir, f"ssim_pair{pair:04d}.pgm"), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (tw, th))
            f.write(np.rint(255.0 * np.minimum(1.0, loss)).astype(np.uint8).tobytes())


def _minus(a, b):
    return None if a is None or b is None else a - b


def parse_guard(spec):
    """"TILE:LO:HI" (the command line) or a sequence of three -> (tile, lo_q4, hi_q4) as hf_guarded_blend_enqueue takes them; ValueError otherwise"""
    parts = spec.split(":") if isinstance(spec, str) else list(spec)
    try:
        tile, lo, hi = (int(str(x), 10) for x in parts)
    except (TypeError, ValueError):
        raise ValueError(f"guard {spec!r}: TILE:LO:HI, three integers (for example 16:32:96)") from None
    if tile not in (16, 32, 64):
        raise ValueError(f"guard {spec!r}: tile {tile}, not 16, 32 or 64")
    if not 0 <= lo < hi <= 65535:
        raise ValueError(f"guard {spec!r}: thresholds outside 0 <= LO < HI <= 65535 (sixteenths of an 8-bit code of mean luma difference)")
    return tile, lo, hi


def evaluate(frames, hdr, H, W, *, black=0.0, white=255.0, detect_scene_cuts=False, scene_threshold=200, source_frame_time=417083,
             device_index=0, device=None, ssim=False, error_map=0, map_dir=None, ssim_map=0, disagreement=0, guard=None, **settings):
    """Leave-one-out evaluation of `frames` (a sequence of flat NV12 uint8 / P010 uint16 host frames of H x W, stride W) -> report dict.
    settings: search_radius, delta_scalar, neighbor_scalar, blur_radius, iterations, max_calc_res (defaults: SETTINGS; 0 = the
    library's default for blur_radius and iterations).  detect_scene_cuts: also report the warp / copy decision the filter's
    scene-change detection would have taken per period (costs one wait per period; the outputs evaluated are always the warps).
    ssim: also score every comparison with the device's windowed SSIM (module docstring); off, nothing of it is called or reported.
    error_map: 16, 32 or 64 -- also the per-tile error map of every interpolation (module docstring); 0, nothing of it is called or
    reported.  ssim_map: 16, 32 or 64 -- also the per-tile SSIM map of every interpolation (module docstring); 0, nothing of it is
    called, allocated or reported.  disagreement: 16, 32 or 64 -- also the warp disagreement map of every evaluated pair at t = 0.5, the
    judge that needs no truth, and beside error_map of the same tile how well it predicts the real error (module docstring); 0, nothing
    of it is called, allocated or reported.  map_dir: with error_map, ssim_map or disagreement, a directory for one PGM heat map of the
    Y plane per evaluated pair and map.  guard: (tile, lo_q4, hi_q4) -- every withheld frame is produced a second time by the guarded blend
    (module docstring) and judged by the same metrics beside the plain one; None, nothing of it is called, allocated or reported."""
    if guard is not None:
        guard = parse_guard(guard)
    if error_map not in (0, 16, 32, 64):
        raise ValueError(f"evaluate: error_map {error_map}, a tile of 16, 32 or 64 luma pixels (0: none)")
    if ssim_map not in (0, 16, 32, 64):
        raise ValueError(f"evaluate: ssim_map {ssim_map}, a tile of 16, 32 or 64 luma pixels (0: none)")
    if disagreement not in (0, 16, 32, 64):
        raise ValueError(f"evaluate: disagreement {disagreement}, a tile of 16, 32 or 64 luma pixels (0: none)")
    if map_dir and not error_map and not ssim_map and not disagreement and not guard:
        raise ValueError("evaluate: map_dir needs error_map, ssim_map, disagreement or guard")
    unknown = set(settings) - set(SETTINGS)
    if unknown:
        raise TypeError(f"evaluate: unknown settings {sorted(unknown)} (known: {sorted(SETTINGS)})")
    st = dict(SETTINGS, **{k: int(v) for k, v in settings.items()})
    dev = device or _Device(device_index)
    sched = schedule(len(frames))
    peak = 65535 if hdr else 255
    main = dev.calc(hdr, H, W, black, white, st)
    aux = dev.calc(hdr, H, W, black, white, st)     # copyFrame at the same levels: the truths and the repeat baseline
    filt = dev.scene_filter(source_frame_time, scene_threshold) if detect_scene_cuts else None
    frame_bytes, out_bytes = int(main.input_frame_bytes), int(main.output_frame_bytes)
    free_in, free_out, rows, cuts = [], [], [], []
    maps_buf, luma_maps = None, []                  # error_map: the chunk's maps on the device; map_dir: (pair, Y map) of every pair
    if error_map:
        from .calc import frame_error_maps
        tiles_x, tiles_y, map_bytes = main.frameErrorMapShape(error_map)
        maps_buf = dev.buffer(map_bytes * min(PAIRS_PER_READ, sum(s["evaluated"] for s in sched)))
    smaps_buf, luma_smaps = None, []                # ssim_map: the same for the SSIM maps, in a buffer of their own
    if ssim_map:
        from .calc import frame_ssim_maps
        stiles_x, stiles_y, smap_bytes = main.frameSsimMapShape(ssim_map)
        smaps_buf = dev.buffer(smap_bytes * min(PAIRS_PER_READ, sum(s["evaluated"] for s in sched)))
    dis_buf, luma_dis, overlaps = None, [], []       # disagreement: the same again; overlaps: per pair and plane (hits, k) or None
    if disagreement:
        from .calc import frame_error_maps
        dtiles_x, dtiles_y, dmap_bytes = main.frameErrorMapShape(disagreement)
        dis_buf = dev.buffer(dmap_bytes * min(PAIRS_PER_READ, sum(s["evaluated"] for s in sched)))
    # guard: per chunk fewer pairs, a third result slot each behind the two of every pair; its maps (the confidence the call stores, and
    # those of the metrics asked for) in buffers of their own
    per_read = max(1, PAIRS_PER_READ * 2 // 3) if guard else PAIRS_PER_READ
    gbase = 2 * per_read
    gdis_buf = gmaps_buf = gsmaps_buf = None
    luma_masks = []
    if guard:
        from .calc import frame_error_maps, guard_weights
        n_maps = min(per_read, sum(s["evaluated"] for s in sched))
        gtiles_x, gtiles_y, gdis_bytes = main.frameErrorMapShape(guard[0])
        gdis_buf = dev.buffer(gdis_bytes * n_maps)
        if error_map:
            gmaps_buf = dev.buffer(map_bytes * n_maps)
        if ssim_map:
            gsmaps_buf = dev.buffer(smap_bytes * n_maps)
    take = lambda pool, nbytes: pool.pop() if pool else dev.buffer(nbytes)
    src = {}    # period -> device frame of its source; the last three outlive a chunk (the context's ring still references them)
    try:
        todo = list(sched)
        while todo:
            # a chunk: the periods up to PAIRS_PER_READ evaluated pairs
            chunk, n_eval = [], 0
            while todo and n_eval < per_read:
                chunk.append(todo.pop(0))
                n_eval += chunk[-1]["evaluated"]
            used_in, used_out = [], []
            # sources, truths and baselines of the chunk first; the second context is waited for ONCE, before the clip context starts
            for s in chunk:
                src[s["period"]] = take(free_in, frame_bytes)
                src[s["period"]].upload(frames[s["source_frame"]])
            jobs, gouts = {}, {}
            for s in (s for s in chunk if s["evaluated"]):
                t_raw = take(free_in, frame_bytes)
                t_raw.upload(frames[s["truth_frame"]])
                used_in.append(t_raw)
                truth, repeat, out = take(free_out, out_bytes), take(free_out, out_bytes), take(free_out, out_bytes)
                used_out += [truth, repeat, out]
                for raw, dst in ((t_raw, truth), (src[s["period"] - 2], repeat)):   # the pair's first source was submitted two periods earlier
                    aux.m_frameCount = 0            # copyFrame then shows the frame just submitted (opticalFlowCalcSDR.cpp:173)
                    aux.setOutputBuffer(dst.ptr)
                    aux.updateFrameDevice(raw.ptr)
                    aux.copyFrame()
                jobs[s["period"]] = (truth, repeat, out)
                if guard:
                    gouts[s["period"]] = take(free_out, out_bytes)
                    used_out.append(gouts[s["period"]])
            aux.sync()
            # the clip: periods and comparisons back to back, nothing waits on the host (unless the caller asked for the cut decisions)
            scratch = take(free_out, out_bytes)     # where the warm-up pair's output goes
            used_out.append(scratch)
            slot = 0
            for s in chunk:
                b = src[s["period"]]
                if filt is not None:
                    filt.begin_source_frame()
                if not s["flow"]:
                    main.updateFrameDeviceRef(b.ptr)
                    continue
                truth, repeat, out = jobs.get(s["period"], (None, None, scratch))
                main.interpolatePeriod(b.ptr, [0.5], [out.ptr], 2)
                if s["evaluated"]:
                    if disagreement:                # the frames and the flow this period's warp used: before the next period moves the ring
                        main.warpDisagreementMapEnqueue([0.5], disagreement, dis_buf.ptr + (slot // 2) * dmap_bytes)
                    main.frameErrorEnqueue([out.ptr, repeat.ptr], [truth.ptr, truth.ptr], slot)
                    if ssim:
                        main.frameSsimEnqueue([out.ptr, repeat.ptr], [truth.ptr, truth.ptr], slot)
                    if error_map:
                        main.frameErrorMapEnqueue([out.ptr], [truth.ptr], error_map, maps_buf.ptr + (slot // 2) * map_bytes)
                    if ssim_map:
                        main.frameSsimMapEnqueue([out.ptr], [truth.ptr], ssim_map, smaps_buf.ptr + (slot // 2) * smap_bytes)
                    slot += 2
                if s["evaluated"] and guard:        # the same frames and flow again, still ahead of the next period; judged like `out`
                    i, gout = slot // 2 - 1, gouts[s["period"]]
                    main.guardedBlendEnqueue([0.5], guard[0], guard[1], guard[2], gdis_buf.ptr + i * gdis_bytes, [gout.ptr])
                    main.frameErrorEnqueue([gout.ptr], [truth.ptr], gbase + i)
                    if ssim:
                        main.frameSsimEnqueue([gout.ptr], [truth.ptr], gbase + i)
                    if error_map:
                        main.frameErrorMapEnqueue([gout.ptr], [truth.ptr], error_map, gmaps_buf.ptr + i * map_bytes)
                    if ssim_map:
                        main.frameSsimMapEnqueue([gout.ptr], [truth.ptr], ssim_map, gsmaps_buf.ptr + i * smap_bytes)
                if filt is not None:
                    main.waitFlow()
                    fc, delta = int(main.m_frameCount), int(main.m_totalFrameDelta)
                    filt.push(fc, delta)
                    cuts.append({"period": s["period"], "pair": s["pair"], "total_frame_delta": delta,
                                 "kind": "copy" if filt.detect(fc) else "warp"})
            got = main.frameErrorRead(0, slot) if slot else []
            got_ssim = main.frameSsimRead(0, slot) if ssim and slot else []
            if error_map and slot:                  # (the read above has waited for the context)
                import numpy as np
                got_maps = frame_error_maps(maps_buf.download(np.uint8, (slot // 2) * map_bytes), slot // 2, tiles_x, tiles_y)
            if ssim_map and slot:
                import numpy as np
                got_smaps = frame_ssim_maps(smaps_buf.download(np.uint8, (slot // 2) * smap_bytes), slot // 2, stiles_x, stiles_y)
            if disagreement and slot:
                import numpy as np
                got_dis = frame_error_maps(dis_buf.download(np.uint8, (slot // 2) * dmap_bytes), slot // 2, dtiles_x, dtiles_y)
            if guard and slot:
                import numpy as np
                n = slot // 2
                got_g = main.frameErrorRead(gbase, n)
                got_gssim = main.frameSsimRead(gbase, n) if ssim else []
                got_gdis = frame_error_maps(gdis_buf.download(np.uint8, n * gdis_bytes), n, gtiles_x, gtiles_y)
                if error_map:
                    got_gmaps = frame_error_maps(gmaps_buf.download(np.uint8, n * map_bytes), n, tiles_x, tiles_y)
                if ssim_map:
                    got_gsmaps = frame_ssim_maps(gsmaps_buf.download(np.uint8, n * smap_bytes), n, stiles_x, stiles_y)
            for i, s in enumerate(s for s in chunk if s["evaluated"]):
                row = {"pair": s["pair"], "period": s["period"], "source_frames": [2 * s["pair"], 2 * s["pair"] + 2],
                       "withheld_frame": s["truth_frame"], "interpolated": _with_psnr(got[2 * i], peak), "repeat": _with_psnr(got[2 * i + 1], peak)}
                a, r = row["interpolated"]["Y"]["psnr"], row["repeat"]["Y"]["psnr"]
                row["gain_db_y"] = None if a is None or r is None else a - r
                if ssim:
                    _add_ssim(row["interpolated"], got_ssim[2 * i])
                    _add_ssim(row["repeat"], got_ssim[2 * i + 1])
                    row["gain_ssim_y"] = _minus(row["interpolated"]["Y"]["ssim"], row["repeat"]["Y"]["ssim"])
                if error_map:
                    row["interpolated"]["map"] = _map_dict(got_maps[i], error_map)
                    if map_dir:
                        luma_maps.append((s["pair"], got_maps[i][0].copy()))
                if ssim_map:
                    row["interpolated"]["ssim_map"] = _ssim_map_dict(got_smaps[i], ssim_map, got_maps[i] if error_map == ssim_map else None)
                    if map_dir:
                        luma_smaps.append((s["pair"], got_smaps[i][0].copy()))
                if disagreement:
                    over = [_overlap_top1pct(got_maps[i][k], got_dis[i][k], disagreement) for k in range(3)] if error_map == disagreement else None
                    row["interpolated"]["disagreement"] = _disagreement_dict(got_dis[i], disagreement, over)
                    if over is not None:
                        overlaps.append(over)
                    if map_dir:
                        luma_dis.append((s["pair"], got_dis[i][0].copy()))
                if guard:
                    g = row["guarded"] = _with_psnr(got_g[i], peak)
                    row["guard_gain_db"] = _minus(g["Y"]["psnr"], row["interpolated"]["Y"]["psnr"])
                    if ssim:
                        _add_ssim(g, got_gssim[i])
                        row["guard_gain_ssim"] = _minus(g["Y"]["ssim"], row["interpolated"]["Y"]["ssim"])
                    if error_map:
                        g["map"] = _map_dict(got_gmaps[i], error_map)
                    if ssim_map:
                        g["ssim_map"] = _ssim_map_dict(got_gsmaps[i], ssim_map, got_gmaps[i] if error_map == ssim_map else None)
                    wt, w = guard_weights(got_gdis[i:i + 1], guard[0], guard[1], guard[2], H, W, hdr)
                    g["mask"] = {"tiles": int(wt.size), "tiles_firing": int(np.count_nonzero(wt)), "mean_weight": float(w.mean()) / 256.0}
                    if map_dir:
                        luma_masks.append((s["pair"], np.minimum(w[0], 255).astype(np.uint8)))
                rows.append(row)
            # everything has finished: the chunk's buffers can be used again, but for the three sources the ring still references
            last = chunk[-1]["period"]
            free_in += used_in + [src.pop(j) for j in sorted(src) if j <= last - 3]
            free_out += used_out
    finally:
        main.close()
        aux.close()
        if filt is not None:
            filt.close()
        for b in free_in + free_out + list(src.values()) + [b for b in (maps_buf, smaps_buf, dis_buf, gdis_buf, gmaps_buf, gsmaps_buf) if b is not None]:
            b.free()
    worst = min(rows, key=lambda r: float("inf") if r["interpolated"]["Y"]["psnr"] is None else r["interpolated"]["Y"]["psnr"])
    clip = {"interpolated": _aggregate(rows, "interpolated", peak), "repeat": _aggregate(rows, "repeat", peak),
            "worst_pair": {"pair": worst["pair"], "psnr_y": worst["interpolated"]["Y"]["psnr"]}}
    a, r = clip["interpolated"]["Y"]["psnr"], clip["repeat"]["Y"]["psnr"]
    clip["gain_db_y"] = None if a is None or r is None else a - r
    if ssim:
        _add_ssim_aggregate(clip["interpolated"], rows, "interpolated")
        _add_ssim_aggregate(clip["repeat"], rows, "repeat")
        clip["gain_ssim_y"] = _minus(clip["interpolated"]["Y"]["ssim"], clip["repeat"]["Y"]["ssim"])
        low = min(rows, key=lambda r: float("inf") if r["interpolated"]["Y"]["ssim"] is None else r["interpolated"]["Y"]["ssim"])
        clip["worst_pair_ssim"] = {"pair": low["pair"], "ssim_y": low["interpolated"]["Y"]["ssim"]}
    if error_map:
        top = max(rows, key=lambda r: r["interpolated"]["map"]["Y"]["worst"][0]["sse"])   # (the first of equals: the earlier pair)
        t = top["interpolated"]["map"]["Y"]["worst"][0]
        clip["worst_tile"] = {"pair": top["pair"], "plane": "Y", "x": t["x"], "y": t["y"], "sse": t["sse"]}
        if map_dir:
            _write_map_pgms(map_dir, luma_maps, error_map, H, W)
    if ssim_map:
        # the worst luma tile of the clip by the pairs' own order (cross-multiplied integers; the first of equals: the earlier pair)
        low = None
        for r in rows:
            for t in r["interpolated"]["ssim_map"]["Y"]["worst"][:1]:
                if low is None or t["sum_loss_q32"] * low[1]["count"] > low[1]["sum_loss_q32"] * t["count"]:
                    low = (r["pair"], t)
        clip["worst_tile_ssim"] = None if low is None else {"pair": low[0], "plane": "Y", "x": low[1]["x"], "y": low[1]["y"], "ssim": low[1]["ssim"]}
        if map_dir:
            _write_ssim_pgms(map_dir, luma_smaps)
    if disagreement:
        clip["disagreement"] = {}
        for k, p in enumerate(PLANES):
            clip["disagreement"][p] = {"sse": sum(r["interpolated"]["disagreement"][p]["sse"] for r in rows)}
            if error_map == disagreement:
                seen = [o[k] for o in overlaps if o[k] is not None]
                clip["disagreement"][p]["overlap_top1pct"] = sum(h for h, _ in seen) / sum(n for _, n in seen) if seen else None
        top = max(rows, key=lambda r: r["interpolated"]["disagreement"]["Y"]["worst"][0]["sse"])   # (the first of equals: the earlier pair)
        t = top["interpolated"]["disagreement"]["Y"]["worst"][0]
        clip["worst_tile_disagreement"] = {"pair": top["pair"], "plane": "Y", "x": t["x"], "y": t["y"], "sse": t["sse"]}
        if map_dir:
            _write_map_pgms(map_dir, luma_dis, disagreement, H, W, prefix="dis")
    if guard:
        clip["guarded"] = _aggregate(rows, "guarded", peak)
        clip["guard_gain_db"] = _minus(clip["guarded"]["Y"]["psnr"], clip["interpolated"]["Y"]["psnr"])
        if ssim:
            _add_ssim_aggregate(clip["guarded"], rows, "guarded")
            clip["guard_gain_ssim"] = _minus(clip["guarded"]["Y"]["ssim"], clip["interpolated"]["Y"]["ssim"])
        clip["guarded"]["mask"] = {"tiles": sum(r["guarded"]["mask"]["tiles"] for r in rows),
                                   "tiles_firing": sum(r["guarded"]["mask"]["tiles_firing"] for r in rows),
                                   "mean_weight": sum(r["guarded"]["mask"]["mean_weight"] for r in rows) / len(rows)}
        if map_dir:
            os.makedirs(map_dir, exist_ok=True)
            for pair, w in luma_masks:              # the luma mask itself, one pixel per luma pixel: 0 .. 255 = min(w, 255)
                with open(os.path.join(map_dir, f"guard_pair{pair:04d}.pgm"), "wb") as f:
                    f.write(b"P5\n%d %d\n255\n" % (W, H))
                    f.write(w.tobytes())
    out = {"geometry": {"width": W, "height": H, "hdr": bool(hdr), "peak": peak, "frames": len(frames)},
           "settings": dict(st, black_level=float(black), white_level=float(white)),
           "warmup_pairs": [s["pair"] for s in sched if s["pair"] is not None and not s["evaluated"]],
           "pairs": rows, "clip": clip, "scene_cuts": cuts if detect_scene_cuts else None}
    if guard:
        out["guard"] = {"tile": guard[0], "lo_q4": guard[1], "hi_q4": guard[2]}
    return out


# ---- confidence without a truth frame: the disagreement of the two warped halves at the real output schedule ----
def confidence_schedule(n_frames, source_frame_time, target_frame_time):
    """The periods of a confidence run over n_frames frames, every frame a source: one dict per period, in order --
         period        j
         source_frame  index of the frame submitted (frames[j]; the last one once more at the end, so that the last pair is reached)
         flow          a flow is calculated (the filter's gating: from the third frame on)
         pair          the pair (frames[pair], frames[pair + 1]) the period's outputs would show, None before there is one
         evaluated     False for pair 0, which is shown before any flow has been calculated (warm-up)
         t             the blending scalars of the period's outputs: protocol.BlendSchedule(source, target).plan, period by period"""
    from .protocol import BlendSchedule
    if n_frames < 3:
        raise ValueError(f"a confidence run needs at least 3 frames, got {n_frames}")
    plan = BlendSchedule(source_frame_time, target_frame_time).plan(n_frames + 1)
    out = []
    for j in range(n_frames + 1):
        pair = j - 2 if j >= 2 else None
        out.append({"period": j, "source_frame": min(j, n_frames - 1), "flow": j >= 2, "pair": pair,
                    "evaluated": pair is not None and pair >= 1, "t": [float(t) for t in plan[j]]})
    return out


def confidence(frames, hdr, H, W, *, source_frame_time, target_frame_time, tile=16, device_index=0, device=None, **settings):
    """How far the two warped halves of every output of a clip are apart, at the real output schedule and with nothing withheld -> report
    dict (module docstring).  frames: flat NV12 uint8 / P010 uint16 host frames of H x W, stride W; source_frame_time / target_frame_time
    in 100 ns units, as the filter counts them; tile: 16, 32 or 64 luma pixels; settings: those of evaluate().  No output frame exists:
    every period is submitted with no outputs and the maps of its t's are enqueued behind it."""
    if tile not in (16, 32, 64):
        raise ValueError(f"confidence: tile {tile}, 16, 32 or 64 luma pixels")
    unknown = set(settings) - set(SETTINGS)
    if unknown:
        raise TypeError(f"confidence: unknown settings {sorted(unknown)} (known: {sorted(SETTINGS)})")
    import numpy as np
    from .calc import frame_error_maps
    st = dict(SETTINGS, **{k: int(v) for k, v in settings.items()})
    dev = device or _Device(device_index)
    sched = confidence_schedule(len(frames), source_frame_time, target_frame_time)
    main = dev.calc(hdr, H, W, 0.0, 255.0, st)       # (no levels are applied to the two halves)
    frame_bytes = int(main.input_frame_bytes)
    tiles_x, tiles_y, map_bytes = main.frameErrorMapShape(tile)
    # chunks by bytes: the periods whose maps fit CONFIDENCE_MAP_BYTES and whose sources -- all uploaded before the chunk is submitted --
    # fit CONFIDENCE_SOURCE_BYTES, one period at the least
    chunks, held, sources = [[]], 0, 0
    for s in sched:
        need = len(s["t"]) * map_bytes if s["evaluated"] else 0
        if chunks[-1] and ((held and held + need > CONFIDENCE_MAP_BYTES) or sources + frame_bytes > CONFIDENCE_SOURCE_BYTES):
            chunks.append([])
            held = sources = 0
        chunks[-1].append(s)
        held += need
        sources += frame_bytes
    maps_buf = dev.buffer(max(sum(len(s["t"]) * map_bytes for s in chunk if s["evaluated"]) for chunk in chunks))
    counts = {"Y": H * W, "U": (H // 2) * (W // 2), "V": (H // 2) * (W // 2)}
    free_in, src, rows = [], {}, []
    try:
        for chunk in chunks:
            for s in chunk:
                src[s["period"]] = free_in.pop() if free_in else dev.buffer(frame_bytes)
                src[s["period"]].upload(frames[s["source_frame"]])
            used = 0
            for s in chunk:
                b = src[s["period"]]
                if not s["flow"]:
                    main.updateFrameDeviceRef(b.ptr)
                    continue
                main.interpolatePeriod(b.ptr, [], [], 2)        # update and flow only
                if s["evaluated"]:
                    for k in range(0, len(s["t"]), MAX_DISAGREEMENT_OUTPUTS):
                        ts = s["t"][k:k + MAX_DISAGREEMENT_OUTPUTS]
                        main.warpDisagreementMapEnqueue(ts, tile, maps_buf.ptr + used)
                        used += len(ts) * map_bytes
            main.sync()
            got = frame_error_maps(maps_buf.download(np.uint8, used), used // map_bytes, tiles_x, tiles_y) if used else []
            at = 0
            for s in (s for s in chunk if s["evaluated"]):
                outputs = []
                for t in s["t"]:
                    o = {"t": t}
                    for i, p in enumerate(PLANES):
                        o[p] = _plane_totals(got[at][i])
                        o[p]["rms"] = math.sqrt(o[p]["sse"] / counts[p])
                        o[p]["worst"] = _worst_tiles(got[at][i], tile, 1)[0]
                    outputs.append(o)
                    at += 1
                rows.append({"period": s["period"], "pair": s["pair"], "source_frames": [s["pair"], s["pair"] + 1], "t": list(s["t"]),
                             "outputs": outputs, "mean_rms_y": sum(o["Y"]["rms"] for o in outputs) / len(outputs)})
            last = chunk[-1]["period"]                          # the ring still references the last three sources
            free_in += [src.pop(j) for j in sorted(src) if j <= last - 3]
    finally:
        main.close()
        for b in free_in + list(src.values()) + [maps_buf]:
            b.free()
    every = [(r, o) for r in rows for o in r["outputs"]]
    clip = {}
    for p in PLANES:
        sse = sum(o[p]["sse"] for _, o in every)
        clip[p] = {"sse": sse, "sad": sum(o[p]["sad"] for _, o in every), "max_abs": max(o[p]["max_abs"] for _, o in every),
                   "rms": math.sqrt(sse / (counts[p] * len(every)))}
    r, o = max(every, key=lambda ro: ro[1]["Y"]["sse"])         # (the first of equals: the earlier period, the earlier t)
    clip["worst"] = {"period": r["period"], "pair": r["pair"], "t": o["t"], "rms_y": o["Y"]["rms"]}
    clip["mean_rms_y"] = [r["mean_rms_y"] for r in rows]
    return {"geometry": {"width": W, "height": H, "hdr": bool(hdr), "frames": len(frames)}, "settings": st,
            "schedule": {"source_frame_time": int(source_frame_time), "target_frame_time": int(target_frame_time)},
            "tile": tile, "shape": [int(tiles_y), int(tiles_x)],
            "warmup_pairs": [s["pair"] for s in sched if s["pair"] is not None and not s["evaluated"]],
            "periods": rows, "clip": clip}


# ---- command line ----
SWEEP_KEYS = {"radius": "search_radius", "delta": "delta_scalar", "neighbor": "neighbor_scalar", "blur": "blur_radius",
              "iterations": "iterations", "max-calc-res": "max_calc_res", "max_calc_res": "max_calc_res"}
SWEEP_KEYS.update({v: v for v in list(SWEEP_KEYS.values())})


class _ClipFrames:
    """The frames of a cli._Clip as a sequence of NV12 / P010 host frames (planar raw files re-laid on the host: this is measurement)."""

    def __init__(self, clip, planar_raw, limit=0):
        self.clip, self.planar_raw = clip, planar_raw
        self.n = min(clip.n_frames, limit) if limit else clip.n_frames

    def __len__(self):
        return self.n

    def __getitem__(self, k):
        import numpy as np
        c = self.clip
        out = np.empty(c.n_el, dtype=c.dt)
        if c.y4m or not self.planar_raw:
            c.read_into(k, out)
            return out
        from .y4m import planar_to_semiplanar
        c.read_raw_into(k, out)
        H, W = c.height, c.width
        return planar_to_semiplanar(out[:H * W].reshape(H, W), out[H * W:H * W * 5 // 4].reshape(H // 2, W // 2),
                                    out[H * W * 5 // 4:].reshape(H // 2, W // 2), c.hdr).reshape(-1)


def parse_sweeps(specs):
    """['radius=5,16', 'blur=4,32'] -> [{'search_radius': 5, 'blur_radius': 4}, ...]: the cartesian product, in order."""
    keys, values = [], []
    for spec in specs or []:
        k, _, v = spec.partition("=")
        if k.strip() not in SWEEP_KEYS or not v:
            raise ValueError(f"--sweep {spec!r}: KEY=v1,v2,... with KEY one of {sorted(set(SWEEP_KEYS))}")
        keys.append(SWEEP_KEYS[k.strip()])
        values.append([int(x) for x in v.split(",")])
    return [dict(zip(keys, combo)) for combo in itertools.product(*values)]


def parse_args(argv=None):
    from .cli import PIX_FMTS
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input")
    ap.add_argument("--width", type=int); ap.add_argument("--height", type=int)
    ap.add_argument("--hdr", action="store_true")
    ap.add_argument("--pix-fmt", choices=sorted(PIX_FMTS), default=None,
                    help="layout of a raw input: nv12 / p010 (default, by --hdr) or planar yuv420p / yuv420p10le (10-bit formats imply --hdr)")
    ap.add_argument("--radius", type=int, default=SETTINGS["search_radius"]); ap.add_argument("--delta", type=int, default=SETTINGS["delta_scalar"])
    ap.add_argument("--neighbor", type=int, default=SETTINGS["neighbor_scalar"]); ap.add_argument("--blur", type=int, default=SETTINGS["blur_radius"], help="blur radius (0: the reference's 4)")
    ap.add_argument("--iterations", type=int, default=SETTINGS["iterations"], help="refinement iterations (0: auto)")
    ap.add_argument("--max-calc-res", type=int, default=SETTINGS["max_calc_res"])
    ap.add_argument("--black", type=float, default=0.0); ap.add_argument("--white", type=float, default=255.0)
    ap.add_argument("--source-fps", type=float, default=None, help="only for --detect-cuts: default 23.976, or the .y4m header's rate")
    ap.add_argument("--detect-cuts", action="store_true", help="also report the filter's warp / copy decision per period")
    ap.add_argument("--scene-threshold", type=int, default=200)
    ap.add_argument("--max-frames", type=int, default=0, help="evaluate only the first N frames")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--sweep", action="append", metavar="KEY=v1,v2,...",
                    help="evaluate every value of a knob (radius, delta, neighbor, blur, iterations, max-calc-res); repeatable: the cartesian product")
    ap.add_argument("--ssim", action="store_true",
                    help="also score every comparison with the windowed SSIM (8 x 8 windows at stride 4): mean and worst window per plane")
    ap.add_argument("--map", type=int, default=0, choices=(0, 16, 32, 64), metavar="TILE",
                    help="also locate the error: per-tile error maps of every interpolation, tiles of 16, 32 or 64 luma pixels")
    ap.add_argument("--ssim-map", type=int, default=0, choices=(0, 16, 32, 64), metavar="TILE",
                    help="also locate the structural loss: per-tile SSIM maps of every interpolation on the tile grid of --map; beside --map TILE of "
                         "the same size each worst tile carries its squared error too")
    ap.add_argument("--disagreement", type=int, default=0, choices=(0, 16, 32, 64), metavar="TILE",
                    help="also the judge that needs no truth: per-tile disagreement of the two warped halves of every evaluated pair at t = 0.5; beside "
                         "--map TILE of the same size, how well it predicts where the real error is.  With --confidence: the tile (default 16)")
    ap.add_argument("--confidence", action="store_true",
                    help="no leave-one-out: every frame is a source, and the disagreement of the two warped halves is reported for every output of "
                         "the real schedule (--target-fps); no output frame is made")
    ap.add_argument("--target-fps", type=float, default=None, help="with --confidence: the output rate whose blending scalars are judged")
    ap.add_argument("--guard", default=None, metavar="TILE:LO:HI",
                    help="also produce every withheld frame with the guarded blend (a cross-fade where the warped halves disagree) and judge it by the "
                         "same metrics: tile 16, 32 or 64, thresholds in sixteenths of an 8-bit code of mean luma difference, for example 16:32:96; "
                         "no default, measure them on your material")
    ap.add_argument("--map-dir", default=None, metavar="DIR",
                    help="with --map, --ssim-map, --disagreement or --guard: write one PGM heat map per evaluated pair (Y plane, one pixel per tile; with "
                         "--guard the luma mask, one pixel per luma pixel; host work); with --sweep one sub-directory per setting")
    ap.add_argument("--report", default=None, help="write the reports as JSON")
    a = ap.parse_args(argv)
    if a.pix_fmt is None:
        a.pix_fmt = "p010" if a.hdr else "nv12"
    elif PIX_FMTS[a.pix_fmt][0]:
        a.hdr = True
    elif a.hdr:
        ap.error(f"--pix-fmt {a.pix_fmt} is an 8-bit format, --hdr needs p010 or yuv420p10le")
    if a.guard is not None:
        try:
            a.guard = parse_guard(a.guard)
        except ValueError as e:
            ap.error(f"--{e}")
    if a.map_dir and not a.map and not a.ssim_map and not a.disagreement and not a.guard:
        ap.error("--map-dir needs --map TILE, --ssim-map TILE, --disagreement TILE or --guard TILE:LO:HI")
    if a.confidence and not (a.target_fps and a.target_fps > 0):
        ap.error("--confidence needs --target-fps F")
    if a.confidence:   # no truth, no output frame, no levels: what only the leave-one-out run can honour is refused, not ignored
        given = [name for name, on in (("--ssim", a.ssim), ("--map", a.map), ("--ssim-map", a.ssim_map), ("--map-dir", a.map_dir),
                                       ("--guard", a.guard), ("--detect-cuts", a.detect_cuts), ("--black", a.black != 0.0), ("--white", a.white != 255.0)) if on]
        if given:
            ap.error(f"--confidence does not take {', '.join(given)}")
    elif a.target_fps is not None:
        ap.error("--target-fps needs --confidence")
    try:
        a.sweeps = parse_sweeps(a.sweep)
    except ValueError as e:
        ap.error(str(e))
    return a


def _db(x):
    return "  equal" if x is None else f"{x:7.3f}"


def _ss(x):
    return "  none" if x is None else f"{x:6.4f}"


def main(argv=None, device=None):
    """Evaluates the clip once per setting of the sweep (once without --sweep), prints one line per setting; returns the reports."""
    from .cli import PIX_FMTS, _Clip
    a = parse_args(argv)
    clip = _Clip(a.input, a.width, a.height, a.hdr, a.source_fps)
    frames = _ClipFrames(clip, PIX_FMTS[a.pix_fmt][1], a.max_frames)
    base = {"search_radius": a.radius, "delta_scalar": a.delta, "neighbor_scalar": a.neighbor, "blur_radius": a.blur,
            "iterations": a.iterations, "max_calc_res": a.max_calc_res}
    reports = []
    for sweep in (a.sweeps if a.confidence else []):
        st = dict(base, **sweep)
        rep = confidence(frames, clip.hdr, clip.height, clip.width, source_frame_time=int(round(1e7 / clip.source_fps)),
                         target_frame_time=int(round(1e7 / a.target_fps)), tile=a.disagreement or 16, device_index=a.device, device=device, **st)
        reports.append(rep)
        c = rep["clip"]
        print(" ".join(f"{k}={st[k]}" for k in SETTINGS) + f"  periods {len(rep['periods'])}  outputs {sum(len(r['t']) for r in rep['periods'])}  "
              f"disagreement rms Y/U/V {c['Y']['rms']:.3f} {c['U']['rms']:.3f} {c['V']['rms']:.3f}  worst period {c['worst']['period']} "
              f"t {c['worst']['t']:.4f} ({c['worst']['rms_y']:.3f})")
    for k, sweep in enumerate([] if a.confidence else a.sweeps):
        st = dict(base, **sweep)
        map_dir = a.map_dir and (os.path.join(a.map_dir, f"setting{k:02d}") if len(a.sweeps) > 1 else a.map_dir)
        rep = evaluate(frames, clip.hdr, clip.height, clip.width, black=a.black, white=a.white, detect_scene_cuts=a.detect_cuts,
                       scene_threshold=a.scene_threshold, source_frame_time=int(round(1e7 / clip.source_fps)), device_index=a.device,
                       device=device, ssim=a.ssim, error_map=a.map, map_dir=map_dir, ssim_map=a.ssim_map, disagreement=a.disagreement, guard=a.guard, **st)
        reports.append(rep)
        c = rep["clip"]
        knobs = " ".join(f"{k}={st[k]}" for k in SETTINGS)
        print(f"{knobs}  pairs {len(rep['pairs'])}  PSNR Y/U/V {_db(c['interpolated']['Y']['psnr'])} {_db(c['interpolated']['U']['psnr'])} "
              f"{_db(c['interpolated']['V']['psnr'])} dB  repeat Y {_db(c['repeat']['Y']['psnr'])} dB  gain {_db(c['gain_db_y'])} dB  "
              f"worst pair {c['worst_pair']['pair']} ({_db(c['worst_pair']['psnr_y'])} dB)" + (
                  f"  SSIM Y/U/V {_ss(c['interpolated']['Y']['ssim'])} {_ss(c['interpolated']['U']['ssim'])} {_ss(c['interpolated']['V']['ssim'])}  "
                  f"repeat Y {_ss(c['repeat']['Y']['ssim'])}  worst window {_ss(c['interpolated']['Y']['min_ssim'])}  "
                  f"worst pair {c['worst_pair_ssim']['pair']} ({_ss(c['worst_pair_ssim']['ssim_y'])})" if a.ssim else "") + (
                  f"  worst tile pair {c['worst_tile']['pair']} at ({c['worst_tile']['x']}, {c['worst_tile']['y']}) sse {c['worst_tile']['sse']}" if a.map else "") + (
                  f"  worst SSIM tile pair {c['worst_tile_ssim']['pair']} at ({c['worst_tile_ssim']['x']}, {c['worst_tile_ssim']['y']}) "
                  f"{_ss(c['worst_tile_ssim']['ssim'])}" if a.ssim_map and c.get("worst_tile_ssim") else "") + (
                  f"  worst disagreement pair {c['worst_tile_disagreement']['pair']} at ({c['worst_tile_disagreement']['x']}, "
                  f"{c['worst_tile_disagreement']['y']})" + (f"  overlap Y {_ss(c['disagreement']['Y']['overlap_top1pct'])}" if a.map == a.disagreement else "")
                  if a.disagreement else "") + (
                  f"  guarded Y {_db(c['guarded']['Y']['psnr'])} dB  guard gain {_db(c['guard_gain_db'])} dB  mean weight {c['guarded']['mask']['mean_weight']:.4f}"
                  + (f"  guarded SSIM Y {_ss(c['guarded']['Y']['ssim'])}" if a.ssim else "") if a.guard else ""))
    if a.report:
        with open(a.report, "w") as f:
            json.dump({"input": a.input, "reports": reports}, f, indent=1)
    return reports


if __name__ == "__main__":
    main()
    sys.exit(0)
