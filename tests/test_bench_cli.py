"""bench.py's command line: what a plain run leaves out and --full brings
back, --prepare (fills the corpus cache without a GPU) and --dump-outputs
(the last timed step's outputs as .npy, checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_help_lists_the_options():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    for opt in ("--full", "--dump-outputs", "--prepare", "--steps", "--warmup", "--gpus"):
        assert opt in r.stdout


def test_plain_run_times_steps_once_and_nothing_else(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert (a.steps, a.warmup, a.windows) == (7, 2, 1) and not a.full
    assert (a.serial_steps, a.e2e_steps, a.one_threads) == (0, 0, 0)


def test_full_restores_the_other_legs(monkeypatch):
    a = _parse(monkeypatch, "--full")
    assert a.full and (a.windows, a.serial_steps, a.e2e_steps, a.one_threads) == (5, 5, 3, 32)
    a = _parse(monkeypatch, "--full", "--windows", "2", "--serial-steps", "0", "--one-threads", "4")
    assert (a.windows, a.serial_steps, a.e2e_steps, a.one_threads) == (2, 0, 3, 4)
    a = _parse(monkeypatch, "--serial-steps", "1")  # a leg asked for by name runs without --full
    assert (a.windows, a.serial_steps, a.e2e_steps) == (1, 1, 0)


def test_prepare_fills_the_cache(tmp_path):
    from datago_amd import synth
    env = dict(os.environ, DATAGO_CORPUS_CACHE=str(tmp_path / "cache"))
    cmd = [sys.executable, BENCH, "--prepare", "--pool", "6", "--short-min", "32", "--short-max", "64", "--workers", "1"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    got = synth.load_pool_images(2, 6, range(6), 32, 64, cache_dir=str(tmp_path / "cache"))
    assert got == synth.mixed_corpus(2, 6, 32, 64)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "(0 generated now)" in r.stderr


@pytest.mark.gpu
def test_dump_outputs_of_the_last_timed_step(tmp_path):
    from datago_amd import synth
    from oracle import buckets as B
    from oracle import oracle as O
    steps, warmup, batch, pool, samples = 2, 1, 8, 24, 64
    env = dict(os.environ, DATAGO_CORPUS_CACHE=str(tmp_path / "cache"))
    env.pop("WORLD_SIZE", None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--batch", str(batch), "--pool", str(pool), "--samples", str(samples), "--short-max", "512",
                        "--dump-outputs", str(tmp_path / "a")], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["windows"]["n"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["cpu_baseline"] is None and line["e2e_decode_one"] is None and line["roofline_isolated"] is None
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert set(got) == {"meta", "image_sums", "pixels_sample", "image0"}
    assert got["meta"].dtype == np.float64 and got["image_sums"].dtype == np.float64
    assert got["pixels_sample"].dtype == np.float32 and got["image0"].dtype == np.float32
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    # the last timed step's batch (bench.py jpeg_pool / batch_idx), through the oracle in the run's semantics
    k = warmup + steps - 1
    imgs = [((k * batch + j) % samples) % pool for j in range(batch)]
    datas = synth.mixed_corpus(2, pool, 256, 512)
    t = B.ARAwareTransform(1024, 32, 0.5, 2.0)
    refs = []
    for i in imgs:
        with O.semantics(O.SEM_ZUNE):
            dec = O.jpeg_decode(datas[i])[1]
        refs.append(O.crop_and_resize(dec, *t.target_size(dec.shape[1], dec.shape[0]), O.MODE_FIR))
    meta = got["meta"]
    assert meta.shape == (batch, 8) and not meta[:, 5].any()
    for j, ref in enumerate(refs):
        assert (meta[j, 2], meta[j, 3], meta[j, 7]) == (ref.shape[1], ref.shape[0], ref.size)
        assert got["image_sums"][j] == float(ref.sum(dtype=np.uint64))
    assert np.array_equal(got["image0"], refs[0].reshape(got["image0"].shape).astype(np.float32))
    flat = np.concatenate([r.reshape(-1) for r in refs])
    assert flat.size > got["pixels_sample"].size  # this batch is sampled, not written whole
    import bench
    pos = np.sort(np.random.default_rng(bench.DUMP_SEED).integers(0, flat.size, size=bench.DUMP_SAMPLE))
    assert np.array_equal(got["pixels_sample"], flat[pos].astype(np.float32))
