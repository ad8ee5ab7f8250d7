"""bench.py's plain run, ``--full`` and ``--dump-outputs``: what a dump holds
(CPU, on host tensors), which configuration reads the image build() left in
the tree, and — on the GPU — a small plain run whose dump is compared with
``oracle/evalref.c`` lane for lane and whose line carries no CPU leg."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from mythril_amd import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(path):
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def _words(sample):
    """(units, cols, 2) float64 halves -> (units, cols) uint64 words."""
    return sample[:, :, 0].astype(np.uint64) | sample[:, :, 1].astype(np.uint64) << np.uint64(32)


def test_dump_holds_first_indices_row_sums_and_sampled_words(tmp_path):
    import torch
    n, units = 1000, 7                                  # 16 words, the last one partial
    words = (n + 63) // 64
    g = torch.Generator().manual_seed(1)
    bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (units, words), dtype=torch.int64, generator=g)
    first = torch.tensor([5, shard.NONE, 7, 9, 11, shard.NONE, 1 << 40])
    want = bits.numpy().view(np.uint64).copy()
    want[:, -1] &= np.uint64((1 << (n % 64)) - 1)       # bits past n_assign are cleared
    bench.dump_outputs(str(tmp_path), bits, first, n)
    d = _load(str(tmp_path))
    assert sorted(d) == ["first_sat", "root_bits_cols", "root_bits_rowsum", "root_bits_sample"]
    assert all(a.dtype == np.float64 for a in d.values())
    assert d["first_sat"].tolist() == [5, -1, 7, 9, 11, -1, 1 << 40]
    assert d["root_bits_cols"].tolist() == list(range(words))     # they all fit
    assert np.array_equal(_words(d["root_bits_sample"]), want)
    halves = (want & np.uint64(0xFFFFFFFF)).sum(1) + (want >> np.uint64(32)).sum(1)
    assert np.array_equal(d["root_bits_rowsum"], halves.astype(np.float64))


def test_dump_samples_the_same_columns_within_its_size(tmp_path, monkeypatch):
    import torch
    units, words = 8, 4096
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", units * 16 * 100)     # room for 100 columns
    bits = torch.arange(units * words, dtype=torch.int64).reshape(units, words) * 0x100000001
    first = torch.full((units,), shard.NONE, dtype=torch.int64)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), bits, first, words * 64)
    bench.dump_outputs(str(b), bits.clone(), first, words * 64)
    da, db = _load(str(a)), _load(str(b))
    cols = da["root_bits_cols"].astype(np.int64)
    assert len(cols) == 100 and len(set(cols.tolist())) == 100 and (np.diff(cols) > 0).all()
    assert all(np.array_equal(da[k], db[k]) for k in da)
    assert np.array_equal(_words(da["root_bits_sample"]), bits.numpy().view(np.uint64)[:, cols])
    assert da["root_bits_sample"].nbytes <= bench.DUMP_SAMPLE_BYTES


def test_only_the_default_configuration_reads_the_prebuilt_image():
    n = bench.default_units("c2")
    assert bench.prebuilt_cache("c2", range(n)) == bench.PREBUILT_JIT_CACHE
    assert bench.prebuilt_cache("c2", range(256)) is None
    assert bench.prebuilt_cache("c3", range(bench.default_units("c3"))) is None
    assert bench.prebuilt_cache("c2", list(range(1, n)) + [0]) is None


def test_a_run_only_reads_the_prebuilt_image_and_build_only_writes_it(tmp_path, monkeypatch):
    """A timed run never writes into the tree (it may not be allowed to):
    without a prebuilt image it assembles in process, as any other
    configuration does; ``--jit-build-only`` (``store``) puts the file where
    the run then finds it, under the name jit.cached_image gives it."""
    from mythril_amd import jit
    cache = tmp_path / "jit_cache"
    built = []
    monkeypatch.delenv("MYTHGPU_JIT_CACHE", raising=False)
    monkeypatch.setattr(bench, "PREBUILT_JIT_CACHE", str(cache))
    monkeypatch.setattr(bench, "prebuilt_cache", lambda workload, ids: str(cache))
    monkeypatch.setattr(jit, "compile_batch", lambda *a, **k: built.append(1) or b"image")
    corpus = bench.build_corpus(2, 1)
    assert bench.node_image("c2", corpus, 1, 1) == (b"image", False)
    assert len(built) == 1 and not cache.exists()
    assert bench.node_image("c2", corpus, 1, 1, store=True) == (b"image", False)
    files = sorted(f for f in os.listdir(cache) if f.endswith(".hsaco"))
    assert len(built) == 2 and len(files) == 1
    before = sorted(os.listdir(cache))
    assert bench.node_image("c2", corpus, 1, 1) == (b"image", True)
    assert bench.node_image("c2", corpus, 1, 1, store=True) == (b"image", True)
    assert len(built) == 2 and sorted(os.listdir(cache)) == before
    key = files[0][:-len("_%s.hsaco" % jit.source_digest())]
    assert bench.prebuilt_path(key) == str(cache / files[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step_and_leaves_the_cpu_leg_out(tmp_path):
    from mythril_amd.engine import unpack_bits
    from oracle import evalref
    dags, log2, steps, warmup = 24, 10, 2, 1
    env = dict(os.environ)
    for k in ("MYTHGPU_NREG", "MYTHGPU_LDS_SLOTS", "MYTHGPU_LIB", "MYTHGPU_JIT_CACHE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", "bench.py", "--gpus", "1", "--dags", str(dags),
                        "--assign-log2", str(log2), "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    line = json.loads(r.stdout[r.stdout.rindex('{"metric"'):])
    assert line["steps"] == steps and line["ms_per_step"] > 0
    assert not {"cpu_baseline", "selfcheck", "vs_cpu"} & set(line)
    d = _load(str(tmp_path))
    n = 1 << log2
    first = (warmup + steps - 1) * n                    # lane 0 of the last timed step
    assert d["root_bits_cols"].tolist() == list(range(n // 64))
    rows = _words(d["root_bits_sample"])
    nreg = line["config"]["layout_rule"]["nreg"]
    for u in range(dags):
        _, prog, _, _ = bench.compile_unit(("c2", u, nreg))
        want = evalref.run_gen(evalref.serialize(bench.workload_roots("c2", u), prog), prog,
                               bench.SEED, u, first, n, 4)
        assert np.array_equal(unpack_bits(rows[u], n), want), u
        hit = np.flatnonzero(want)
        assert d["first_sat"][u] == (first + int(hit[0]) if hit.size else -1), u
        halves = (rows[u] & np.uint64(0xFFFFFFFF)).sum() + (rows[u] >> np.uint64(32)).sum()
        assert d["root_bits_rowsum"][u] == float(halves), u
    assert int((d["first_sat"] >= 0).sum()) == line["sat_dags"]
