"""bench.py --dump-outputs on the host: the last step's proofs as float32 byte values, every proof while they fit in the budget,
else the same seeded sample of rows on every run (two builds are compared row for row)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_sample_is_fixed_and_within_64_mb(tmp_path):
    b = _bench()
    proofs = np.random.default_rng(1).integers(0, 256, (192, 132744), dtype=np.uint8)     # one headline step: 192 proofs
    for run in ("a", "b"):
        b.dump_outputs(str(tmp_path / run), proofs)
    got, idx = np.load(tmp_path / "a" / "proofs.npy"), np.load(tmp_path / "a" / "proof_index.npy")
    assert got.dtype == np.float32 and idx.dtype == np.float64
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    assert 0 < len(idx) < 192 and np.all(np.diff(idx) > 0)
    assert np.array_equal(got.astype(np.uint8), proofs[idx.astype(np.int64)])
    assert np.array_equal(got, np.load(tmp_path / "b" / "proofs.npy")) and np.array_equal(idx, np.load(tmp_path / "b" / "proof_index.npy"))


def test_dump_outputs_keeps_every_proof_that_fits(tmp_path):
    b = _bench()
    proofs = np.random.default_rng(2).integers(0, 256, (6, 1000), dtype=np.uint8)
    b.dump_outputs(str(tmp_path), proofs)
    assert np.array_equal(np.load(tmp_path / "proofs.npy"), proofs.astype(np.float32))
    assert np.load(tmp_path / "proof_index.npy").tolist() == list(range(6))
