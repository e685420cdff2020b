"""ctypes face of tests/launch_plan_probe.cpp: the launchers' plan functions (csrc/hf_launch_plan.h), called on the CPU.

load(dir) compiles the probe with plain g++ -- no ROCm include path, so the compile proves the header HIP-free -- once per process.
Shapes are given the way tests/warp_variant_model.py gives them: a geometry tuple, members with byte offsets for alignment."""
import collections
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hopperrender_amd", "csrc")

CONSTANTS = ("kWarpTX kWarpTY kWarpWavesSmall kWarpWavesLarge kWgWaves kWgRows kWgChunksPerWave kWgMinWaves kMaxWarpBatch kMaxWarpOutputs "
             "kMaxFlowBatch kSmallFrameBytes kWarpRounds kWarpFastRows kRowPerLaneMaxBatch kLevel32OneWaveMinBatch kBigOneWaveMinBatch "
             "kBigOneWaveMinRs kBigWavesPerBlock kBlurWindowSumMinDim wg_chunks_1 launch_fields sizeof_member").split()
WarpLaunch = collections.namedtuple(
    "WarpLaunch", "family first count vb group dw rows y_groups out_chunk n_chunks waves grid block plane_blocks blocks_per_member wpr max_unit "
                  "lds_bytes planes")
NONE, FAST, STAGED = 0, 1, 2
PlanePass = collections.namedtuple("PlanePass", "aligned grid_x grid_y block")
SmallLevel = collections.namedtuple("SmallLevel", "one_wave32 rows1 tile_w waves tabk block")
Blur = collections.namedtuple("Blur", "kernel tile grid_x grid_y lds_bytes")
BLUR_KERNELS = ("blur.32x4.window_sums", "blur.32x4.taps", "blur.32x0", "blur.16x0")
PhaseLayout = collections.namedtuple("PhaseLayout", "rs nph nph2 mx lwp bytes")


class Member(ctypes.Structure):
    _fields_ = [("n_out", ctypes.c_int), ("ts", ctypes.c_float * 6), ("out_off", ctypes.c_uint32 * 6), ("src12_off", ctypes.c_uint32),
                ("src21_off", ctypes.c_uint32), ("has_flow_xy", ctypes.c_int), ("wants_plane", ctypes.c_int), ("black", ctypes.c_float),
                ("white", ctypes.c_float)]


def member(n_out, ts, src_off=0, out_off=0, levels=(0.0, 255.0), has_flow_xy=True, wants_plane=False, src21_off=None):
    """One period: n_out outputs with blend scalars ts; the sources at base + src_off (frame21: src21_off), every output at base + out_off."""
    m = Member()
    m.n_out = n_out
    for i, t in enumerate(tuple(ts)[:6]):
        m.ts[i] = t
    for i in range(6):
        m.out_off[i] = out_off
    m.src12_off, m.src21_off = src_off, src_off if src21_off is None else src21_off
    m.has_flow_xy, m.wants_plane = int(has_flow_xy), int(wants_plane)
    m.black, m.white = levels
    return m


def members_array(ms):
    """(ctypes array, count) of a list of Member -- worth keeping when the same members are planned for many geometries."""
    return (Member * max(len(ms), 1))(*ms), len(ms)


class Probe:
    def __init__(self, lib):
        self.lib = lib
        lib.hfp_fastdiv_exact.argtypes = [ctypes.c_ulonglong, ctypes.c_uint32]
        n = len(CONSTANTS)
        buf = (ctypes.c_longlong * n)()
        lib.hfp_constants(buf)
        self.constants = dict(zip(CONSTANTS, buf))
        assert self.constants["launch_fields"] == len(WarpLaunch._fields) and self.constants["sizeof_member"] == ctypes.sizeof(Member)
        self._out = (ctypes.c_longlong * (2 * len(WarpLaunch._fields)))()
        self._geoms = {}

    def _g(self, g):
        a = self._geoms.get(g)
        if a is None:
            a = self._geoms[g] = (ctypes.c_int * 8)(*g)
        return a

    def plan_warp(self, g, mode, members, have_pl=False, max_iters=0):
        """The launches of plan_warp_periods ([] = nothing is launched).  members: a list of Member, or what members_array made of one."""
        arr, n = members if isinstance(members, tuple) else members_array(members)
        k = self.lib.hfp_plan_warp(self._g(g), n, arr, mode, int(have_pl), max_iters, self._out)
        f = len(WarpLaunch._fields)
        return [WarpLaunch(*self._out[i * f:(i + 1) * f]) for i in range(k)]

    def can_build_planes(self, g, max_iters, n_members):
        return bool(self.lib.hfp_can_build_planes(self._g(g), max_iters, n_members))

    def phase_layout(self, g, max_iters):
        o = (ctypes.c_longlong * 6)()
        self.lib.hfp_phase_layout(self._g(g), max_iters, o)
        return PhaseLayout(*o)

    def plane_fast_geometry(self, g, max_iters):
        """(plane_fast_geometry, plane_emission_geometry) of the geometry with the layout make_phase_layout gives it."""
        o = (ctypes.c_longlong * 2)()
        self.lib.hfp_plane_fast_geometry(self._g(g), max_iters, o)
        return bool(o[0]), bool(o[1])

    def plan_warp_generic(self, g, out_off):
        o = (ctypes.c_longlong * 4)()
        self.lib.hfp_plan_warp_generic(self._g(g), out_off, o)
        return PlanePass(*o)

    def plan_copy(self, g, src_off, out_off):
        o = (ctypes.c_longlong * 4)()
        self.lib.hfp_plan_copy(self._g(g), src_off, out_off, o)
        return PlanePass(*o)

    def fastdiv_exact(self, max_u, d):
        return bool(self.lib.hfp_fastdiv_exact(max_u, d))

    def plan_flow_level_small(self, n, window, R, tables_present, sad_read, sad_write):
        o = (ctypes.c_longlong * 6)()
        self.lib.hfp_plan_flow_level_small(n, window, R, int(tables_present), int(sad_read), int(sad_write), o)
        return SmallLevel(*o)

    def plan_flow_big_waves(self, n, rs):
        return self.lib.hfp_plan_flow_big_waves(n, rs)

    def plan_sad_tables(self, windows, k, tables):
        """(sad_read, sad_write) of level k of a chain with these window sizes."""
        o = (ctypes.c_longlong * 2)()
        self.lib.hfp_plan_sad_tables((ctypes.c_int * len(windows))(*windows), len(windows), k, int(tables), o)
        return bool(o[0]), bool(o[1])

    def plan_blur(self, g, n, radius, last_window, nwx=None, nwy=None):
        """last_window: window size of the chain's last level (0: the chain has no level); its table covers the grid unless nwx / nwy say otherwise."""
        o = (ctypes.c_longlong * 5)()
        w = max(last_window, 1)
        lw, lh = g[6], g[7]
        self.lib.hfp_plan_blur(self._g(g), n, int(last_window > 0), w.bit_length() - 1, -(-lw // w) if nwx is None else nwx,
                               -(-lh // w) if nwy is None else nwy, radius, o)
        return Blur(*o)


_probe = None


def load(build_dir):
    """Compile tests/launch_plan_probe.cpp into build_dir (first call of the process) and load it."""
    global _probe
    if _probe is None:
        so = os.path.join(str(build_dir), "liblaunch_plan_probe.so")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                               os.path.join(ROOT, "tests", "launch_plan_probe.cpp"), "-o", so])
        _probe = Probe(ctypes.CDLL(so))
    return _probe
