"""bench.py's run modes on CPU: a plain run keeps only the headline (every measurement with runs
of its own is behind --full), and --dump-outputs writes the exported film as float64 .npy files
(whole, or the same seeded pixel sample of every array when it exceeds the size cap)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_switches_every_extra_measurement_off():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert a.fast_leg == 0 and a.nanovdb_leg == 0 and a.no_cpu_baseline and a.pmc == "off"
    assert a.dump_outputs is None
    # explicit leg options do not bring a leg back without --full
    b = bench.parse(["--fast-leg", "1", "--nanovdb-leg", "1", "--pmc", "on"])
    assert b.fast_leg == 0 and b.nanovdb_leg == 0 and b.no_cpu_baseline and b.pmc == "off"


def test_full_run_keeps_the_legs_and_their_options():
    a = bench.parse(["--full", "--steps", "20", "--warmup", "5"])
    assert a.full and a.fast_leg == 1 and a.nanovdb_leg == 1 and not a.no_cpu_baseline and a.pmc == "auto"
    b = bench.parse(["--full", "--fast-leg", "0", "--no-cpu-baseline", "--pmc", "off", "--dump-outputs", "d"])
    assert b.fast_leg == 0 and b.nanovdb_leg == 1 and b.no_cpu_baseline and b.pmc == "off" and b.dump_outputs == "d"
    # the counter child is a plain run of the parent's configuration
    child = bench.pmc_child_argv(a, 16384)
    assert "--full" not in child and "--dump-outputs" not in child


def test_steps_must_be_positive():
    with pytest.raises(SystemExit):
        bench.parse(["--steps", "0"])


def _film(npix, nbuckets=0):
    import torch
    return torch.arange((4 + 2 * nbuckets) * npix, dtype=torch.float64) * 0.5


def test_dump_outputs_writes_the_film_arrays(tmp_path):
    W, H = 5, 3
    npix = W * H
    film = _film(npix)
    names = bench.dump_outputs(str(tmp_path / "out"), film, W, H)
    assert names == ["film_rgb_sum", "film_weight_sum"]
    rgb = np.load(tmp_path / "out" / "film_rgb_sum.npy")
    w = np.load(tmp_path / "out" / "film_weight_sum.npy")
    assert rgb.dtype == np.float64 and rgb.shape == (H, W, 3) and w.dtype == np.float64 and w.shape == (H, W)
    host = film.numpy()
    assert np.array_equal(rgb.reshape(-1), host[:3 * npix]) and np.array_equal(w.reshape(-1), host[3 * npix:])
    # spectral film: bucket sums and bucket weights per pixel
    nb = 4
    film = _film(npix, nb)
    names = bench.dump_outputs(str(tmp_path / "spec"), film, W, H, nbuckets=nb)
    assert names == ["film_rgb_sum", "film_weight_sum", "spectral_bucket_sum", "spectral_weight_sum"]
    bs = np.load(tmp_path / "spec" / "spectral_bucket_sum.npy")
    bw = np.load(tmp_path / "spec" / "spectral_weight_sum.npy")
    host = film.numpy()
    assert bs.shape == bw.shape == (H, W, nb)
    assert np.array_equal(bs.reshape(-1), host[4 * npix:(4 + nb) * npix])
    assert np.array_equal(bw.reshape(-1), host[(4 + nb) * npix:])


def test_dump_outputs_samples_a_film_over_the_cap(tmp_path, monkeypatch):
    W, H = 16, 8
    npix = W * H
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 1024)   # the whole film is 4 KiB
    film = _film(npix)
    got = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), film, W, H)
        got.append({f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))})
    a, b = got
    assert sorted(a) == ["film_rgb_sum", "film_weight_sum", "pixel_index"]
    assert sum(v.nbytes for v in a.values()) <= 1024
    idx = a["pixel_index"].astype(np.int64)
    assert len(idx) == 1024 // 40 and len(set(idx)) == len(idx) and np.all(np.diff(idx) > 0) and idx.max() < npix
    host = film.numpy()
    assert np.array_equal(a["film_rgb_sum"], host[:3 * npix].reshape(npix, 3)[idx])
    assert np.array_equal(a["film_weight_sum"][:, 0], host[3 * npix:][idx])
    for k in a:   # the same pixels from run to run
        assert a[k].dtype == np.float64 and np.array_equal(a[k], b[k])
