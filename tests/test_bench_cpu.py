"""CPU tests of bench.py's --dump-outputs writer and argument checks.  No GPU here."""
import os
import subprocess
import sys

import numpy as np
import torch

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_writes_the_loss(tmp_path):
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), torch.tensor(1.4511011838912964))
    assert sorted(os.listdir(out)) == ["loss.npy"]
    a = np.load(out / "loss.npy")
    assert a.dtype == np.float32 and a.shape == (1,)
    assert a[0] == np.float32(1.4511011838912964)


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps must be at least 1" in r.stderr
