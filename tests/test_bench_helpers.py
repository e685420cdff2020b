"""CPU: the parts of bench.py that need no GPU -- the sysfs reader behind the line's `device` block, the writer of
--dump-outputs and the --full switch."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_device_sample_reads_the_levels_in_force(tmp_path):
    import bench
    assert bench.device_sample(None) is None
    d = tmp_path / "dev"
    hw = d / "hwmon" / "hwmon3"
    hw.mkdir(parents=True)
    (d / "pp_dpm_sclk").write_text("0: 132Mhz\n1: 2389Mhz *\n2: 2400Mhz\n")
    (d / "pp_dpm_mclk").write_text("0: 900Mhz\n1: 2000Mhz *\n")
    (hw / "power1_average").write_text("1255000000\n")
    (hw / "power1_cap").write_text("1400000000\n")
    (hw / "temp1_input").write_text("61000\n")
    s = bench.device_sample(str(d))
    assert s == {"sclk_mhz": 2389, "mclk_mhz": 2000, "power_w": 1255.0, "power_cap_w": 1400.0, "temp_c": 61.0}


def test_device_sysfs_without_a_gpu_is_none_or_a_directory():
    import bench
    p = bench.device_sysfs(0)
    assert p is None or os.path.isdir(p)


def test_dump_outputs_writes_a_fixed_float_sample_under_64_mb(tmp_path):
    """--dump-outputs at the default workload's shape (48 pair streams of 2160p HDR, 6 outputs in a period): float32 / float64
    files, under 64 MB in all, the same elements sampled on every run, each sampled value the frame's value at its index."""
    import numpy as np
    import bench
    H, W, streams, ts = 2160, 3840, 48, [0.1, 0.3, 0.5, 0.7, 0.9, 0.95]
    elems = (H + H // 2) * W

    class Buf:
        def __init__(self, seed):
            self.seed = seed

        def download(self, dtype, count):
            return (np.arange(count, dtype=np.uint32) * 7 + self.seed).astype(dtype)

    class Calc:
        output_frame_bytes = elems * 2

        def __init__(self, s):
            self.m_totalFrameDelta = 1000 + s

    calcs = [Calc(s) for s in range(streams)]
    bufs = [[Buf(100 * s + j) for j in range(len(ts))] for s in range(streams)]
    runs = []
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), calcs, bufs, ts, 1)
        runs.append({f: np.load(tmp_path / run / f) for f in sorted(os.listdir(tmp_path / run))})
    a, b = runs
    assert sorted(a) == ["blend_scalars.npy", "output_frames_sample.npy", "output_sample_index.npy", "total_frame_delta.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in a) < 64 << 20
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    assert all(np.array_equal(a[f], b[f]) for f in a)
    idx = a["output_sample_index.npy"].astype(np.int64)
    fr = a["output_frames_sample.npy"]
    assert fr.shape == (streams, len(ts), len(idx)) and len(np.unique(idx)) == len(idx) and idx.max() < elems
    assert np.array_equal(fr[5, 3], bufs[5][3].download(np.uint16, elems)[idx])
    assert list(a["blend_scalars.npy"]) == ts and list(a["total_frame_delta.npy"]) == [1000 + s for s in range(streams)]


def test_full_is_off_unless_asked_for(monkeypatch):
    """A plain `bench.py --gpus 1 --steps K --warmup W` leaves everything beside the headline to --full."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2"])
    a = bench.parse_args()
    assert a.full is False and (a.steps, a.warmup) == (5, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-host-io"])
    a = bench.parse_args()
    assert a.full is True and a.no_host_io and (a.steps, a.warmup) == (20, 3)
