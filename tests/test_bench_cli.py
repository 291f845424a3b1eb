"""bench.py without a GPU: the threaded synthetic stream is synth.frame_stream bit for bit (what every timed step reads), and the
command line -- --full off by default, --dump-outputs DIR, --steps of at least one."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from dvm_slam_amd import synth  # noqa: E402


@pytest.mark.parametrize("texture", ["rich", "low"])
def test_threaded_stream_is_synth_stream(texture):
    ref = synth.frame_stream(5, start=37, texture=texture)
    for workers in (1, 3):
        assert np.array_equal(bench.frame_stream(5, start=37, texture=texture, workers=workers), ref)


def test_command_line(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()
