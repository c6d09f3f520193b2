"""CPU: bench.py --dump-outputs helpers -- the fixed parameter / gradient sample and the .npy writer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_pack_sample_is_whole_when_small_and_fixed_when_large():
    small = torch.arange(1000, dtype=torch.float32)
    assert torch.equal(bench.pack_sample(small), small)
    big = torch.arange(bench.DUMP_SAMPLE * 3, dtype=torch.float32)
    a, b = bench.pack_sample(big), bench.pack_sample(big.clone())
    assert a.numel() == bench.DUMP_SAMPLE and torch.equal(a, b)              # same size, same indices
    assert bool((a[1:] >= a[:-1]).all())                                   # sorted indices into an increasing tensor
    assert not torch.equal(a, bench.pack_sample(big, seed=1))


def test_dump_outputs_writes_float32_and_float64(tmp_path):
    bench.dump_outputs(str(tmp_path / "out"), {"loss": torch.tensor(1.5), "emb": torch.ones(4, 3, dtype=torch.bfloat16),
                                               "stats": torch.zeros(3, dtype=torch.float64)})
    got = {f: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["emb.npy", "loss.npy", "stats.npy"]
    assert got["loss.npy"].dtype == np.float64 and float(got["loss.npy"]) == 1.5
    assert got["emb.npy"].dtype == np.float32 and got["emb.npy"].shape == (4, 3)
    assert got["stats.npy"].dtype == np.float64


def test_dump_outputs_refuses_more_than_the_limit(tmp_path):
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "big"), {"x": torch.zeros(bench.DUMP_LIMIT // 4 + 1)})
    assert not os.path.exists(tmp_path / "big")
