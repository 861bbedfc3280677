"""bench.py --dump-outputs, the writer alone (no GPU): what it keeps of a keep mask, in which types, and that the files
stay under 64 MB at the headline size; the run on the GPU is tests/test_gpu_bench_contract.py::test_dump_outputs_is_the_timed_mask."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _mask(rng, n):
    bits = (rng.random(n) < 0.05).astype(np.uint8)
    words = np.zeros((n + 63) // 64 * 8, np.uint8)
    words[:(n + 7) // 8] = np.packbits(bits, bitorder="little")
    return bits, words.view(np.uint64)


def _load(d):
    return [np.load(os.path.join(d, f)) for f in ("keep_sample.npy", "keep_sample_index.npy", "kept_per_block.npy")]


def test_small_masks_are_written_whole(tmp_path):
    rng = np.random.default_rng(1)
    (b0, m0), (b1, m1) = _mask(rng, 1000), _mask(rng, 777)
    bench.dump_outputs(str(tmp_path), [m0, m1], [1000, 777])     # two ranks' masks, concatenated
    keep, idx, per_block = _load(tmp_path)
    bits = np.concatenate([b0, b1])
    assert keep.dtype == np.float32 and idx.dtype == np.float64 and per_block.dtype == np.float32
    assert np.array_equal(idx, np.arange(bits.size)) and np.array_equal(keep, bits)
    assert np.array_equal(per_block, np.add.reduceat(bits.astype(np.int64), np.arange(0, bits.size, 256)))


def test_headline_size_is_sampled_the_same_way_every_time_and_stays_under_64_mb(tmp_path):
    n = 100_000_000                                               # the cfg4 workload's reads per GPU
    bits, m = _mask(np.random.default_rng(2), n)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [m], [n])
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    keep, idx, per_block = a
    assert keep.size == 1 << 21 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < n
    assert np.array_equal(keep, bits[idx.astype(np.int64)])
    assert per_block.size == (n + 255) // 256 and per_block.sum() == bits.sum()
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64e6
