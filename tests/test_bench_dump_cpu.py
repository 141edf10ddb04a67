"""CPU: bench.py --dump-outputs writes what the last timed step's explain() returned as float32 / float64 .npy files, at most 64 MB
in all; an array beyond its share of that is replaced by the same seeded sample of its elements in every run."""
import os

import numpy as np
import torch


def _outputs(B, g):
    return dict(R_tok=torch.randn(B, 2048, generator=g), idx=torch.randint(0, 128256, (B,), generator=g, dtype=torch.int32),
                logit=torch.randn(B, generator=g), logits=torch.randn(B, 128256, generator=g))


def test_dump_outputs_writes_every_array_whole(tmp_path):
    import bench
    out = _outputs(4, torch.Generator().manual_seed(0))
    bench.dump_outputs(str(tmp_path), out, 4, write=True)
    assert sorted(os.listdir(tmp_path)) == ["R_tok.npy", "idx.npy", "logit.npy", "logits.npy"]
    for name, v in out.items():
        a = np.load(tmp_path / f"{name}.npy")
        want = v.double() if name == "idx" else v
        assert a.dtype == want.numpy().dtype and np.array_equal(a, want.numpy()), name


def test_dump_outputs_caps_the_total_with_a_fixed_sample(tmp_path):
    import bench
    out = _outputs(140, torch.Generator().manual_seed(1))          # logits alone: 72 MB in float32
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), out, 140, write=True)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 64 << 20
    for name in ("R_tok", "idx", "logit"):
        assert np.load(tmp_path / "a" / f"{name}.npy").shape == tuple(out[name].shape), name
    a, b = np.load(tmp_path / "a" / "logits.npy"), np.load(tmp_path / "b" / "logits.npy")
    assert a.ndim == 1 and 0 < a.size < out["logits"].numel() and np.array_equal(a, b)
    pick = torch.randint(out["logits"].numel(), (a.size,), generator=torch.Generator().manual_seed(0)).sort().values
    assert np.array_equal(a, out["logits"].reshape(-1)[pick].numpy())
