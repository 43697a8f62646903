"""bench.py --dump-outputs without a GPU: dump_outputs() over a stand-in backend writes every part's numbers and the part trees as
float32 / float64 .npy files, exactly, and within its byte limit it keeps a seeded sample of the trees instead.  On the GPU: a plain
run (no --full) writes them beside the headline and measures nothing else."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from delphy_amd.engine import FlatTree  # noqa: E402


class _Backend:
    def __init__(self, n, seed=5):
        rng = np.random.default_rng(seed)
        self.trees = []
        for p in range(n):
            nn, nm = int(rng.integers(3, 40)), int(rng.integers(1, 30))
            t = FlatTree.empty(nn, nm, 3, 2)
            t.root = p % nn
            t.parent[:] = rng.integers(-1, nn, nn); t.t[:] = rng.normal(size=nn); t.mut_site[:] = rng.integers(0, 29903, nm)
            t.mut_to[:] = rng.integers(0, 4, nm); t.mut_t[:] = rng.normal(size=nm)
            self.trees.append(t)

    def part_download(self, p):
        return self.trees[p]

    def part_derived(self, p, num_nodes):
        return None, None, -1000.0 - p, 0.25 * p

    def part_stats(self, p):
        return dict(status=0, moves_done=1000 * p, rng_draws=3000 * p + 1, proposed=[p, 1, 2, 3, 4], accepted=[0, 1, 0, 1, p])

    def totals(self):
        return -123.5, 7.25


class _Engine:
    def __init__(self, n, lo=0):
        self.backend, self.num_local_parts, self.part_lo = _Backend(n), n, lo


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_holds_every_part_exactly(tmp_path):
    eng = _Engine(60)
    info = bench.dump_outputs(str(tmp_path), eng, 0, 1)
    z = _load(str(tmp_path))
    assert info["parts_with_trees"] == 60 and all(a.dtype in (np.float32, np.float64) for a in z.values())
    assert np.array_equal(z["part_log_G"], -1000.0 - np.arange(60)) and np.array_equal(z["part_moves_done"], 1000.0 * np.arange(60))
    assert np.array_equal(z["part_accepted"][:, 4], np.arange(60)) and np.array_equal(z["totals_log_G_log_augmented_prior"], [-123.5, 7.25])
    trees = eng.backend.trees
    assert np.array_equal(z["tree_part_num_nodes"], [t.num_nodes for t in trees]) and np.array_equal(z["tree_part_root"], [t.root for t in trees])
    for f in ("parent", "t", "mut_site", "mut_to", "mut_t", "mut_offset", "t_min"):
        assert np.array_equal(z["tree_" + f], np.concatenate([getattr(t, f) for t in trees])), f


def test_dump_samples_the_trees_within_its_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 512 << 10)
    eng = _Engine(2000, lo=300)
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), eng, 1, 2)
    bench.dump_outputs(str(b), eng, 1, 2)
    assert sum(os.path.getsize(os.path.join(str(a), f)) for f in os.listdir(str(a))) <= 512 << 10
    assert all(f.startswith("rank1_") for f in os.listdir(str(a)))
    za, zb = _load(str(a)), _load(str(b))
    assert 0 < info["parts_with_trees"] < 2000 and za["rank1_part_ids"][0] == 300 and za["rank1_part_log_G"].shape == (2000,)
    ids = za["rank1_tree_part_ids"].astype(np.int64)
    assert np.all(np.diff(ids) > 0) and ids[0] >= 300 and ids[-1] < 2300
    assert za.keys() == zb.keys() and all(np.array_equal(za[k], zb[k]) for k in za)        # the sample is fixed
    picked = [eng.backend.trees[i - 300] for i in ids]
    assert np.array_equal(za["rank1_tree_t"], np.concatenate([t.t for t in picked]))


@pytest.mark.gpu
def test_plain_run_writes_the_headline_and_its_outputs_only(tmp_path):
    """`bench.py --steps 2 --warmup 1 --dump-outputs DIR` without --full: the headline and the arrays of the last timed step, none of
    the figures --full measures (their fields are null), and no launch after the timed steps."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["unit"] == "moves/s" and out["higher_is_better"] is True and out["dtype"] == "f64" and out["steps"] == 2 and out["warmup"] == 1
    assert all(out[k] is None for k in ("secondary", "decompositions", "roofline", "cpu_baseline", "inclusive", "mixing", "scale_check"))
    assert out["per_rank"]["kernel_ms"] is None and out["check"]["parts_stopped"] == 0 and out["check"]["after_passes"] == 3
    z = _load(str(tmp_path))
    parts = z["part_ids"].shape[0]
    assert out["dumped_outputs"]["files"] == len(z) and out["dumped_outputs"]["parts"] == parts > 7000
    assert np.all(z["part_moves_done"] == 3000) and np.all(z["part_status"] == 0)
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 - parts * 1000) < 1e-6 * parts * 1000          # value = the moves of a step / ms_per_step
    assert np.allclose(z["totals_log_G_log_augmented_prior"], [out["check"]["log_G"], out["check"]["log_augmented_coalescent_prior"]], rtol=1e-12, atol=0)
