"""A plain `bench.py` run end to end on a small S-cloud (one child process): `--steps` sets the
timed steps, the line carries `ms_per_step` and leaves every `--full` block null, and
`--dump-outputs` writes the film of the timed steps — equal to an in-process render of the same
sample indices (launch.sample_plan) of the same device-generated cloud."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, W, H, S, STEPS, WARMUP = 64, 48, 32, 4, 3, 1


def test_plain_bench_line_and_dumped_film(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--res", str(N), "--width", str(W), "--height", str(H),
                        "--spp-per-step", str(S), "--tune-walk", "off", "--dump-outputs", str(out)],
                       capture_output=True, text=True, env=env, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1                      # the JSON line is the only stdout output
    line = json.loads(lines[0])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0
    # value = samples of the timed steps / their wall time (ms_per_step is rounded to 1 us, value to 1e-4)
    ms = line["ms_per_step"]
    assert line["value"] == pytest.approx(W * H * S / (ms * 1e3), rel=5e-4 / ms + 1e-6, abs=1e-4)
    assert line["roofline"]["launches"] == STEPS           # one k_paths launch per timed step
    assert line["fast_mode"] is None and line["nanovdb"] is None and line["cpu_baseline"] is None
    assert line["roofline"]["traffic"] is None and line["roofline"]["limiter"] is None
    assert sorted(os.listdir(out)) == ["film_rgb_sum.npy", "film_weight_sum.npy"]
    rgb, w = np.load(out / "film_rgb_sum.npy"), np.load(out / "film_weight_sum.npy")
    assert rgb.dtype == np.float64 and rgb.shape == (H, W, 3) and w.dtype == np.float64 and w.shape == (H, W)

    # the same cloud and sample indices in this process
    from acceleratedvolrenderer_amd import VolPathIntegrator, scenes, capi
    from acceleratedvolrenderer_amd.launch import sample_plan
    P, _, timed = sample_plan(1, STEPS, WARMUP, S)
    assert line["config"]["pixelsamples"] == P
    density = torch.empty((N, N, N), dtype=torch.float32, device="cuda:0")
    gen = capi.Context(0)
    gen.generate_cloud(density.data_ptr(), N, 0, N ** 3)
    gen.sync()
    gen.close()
    scene = scenes.s_cloud(density, width=W, height=H, sampler="zsobol", spp=P, filter="gaussian")
    integ = VolPathIntegrator(scene, maxdepth=scenes.CLOUD_MAXDEPTH, spp=S, seed=0, device=0)
    try:
        integ.ctx.film_clear()
        for b in timed[0]:
            integ.ctx.render(b, b + S, 0, scenes.CLOUD_MAXDEPTH)
        rgb_i, w_i = integ.film_sums()
    finally:
        integ.close()
    assert np.all(w_i > 0) and np.any(rgb_i > 0)
    # replay mode: the same samples; each pixel's fp64 sum has at most STEPS * S * (filter
    # footprint) terms, whose order (atomics) may differ: a few hundred ulp at the very most
    assert np.allclose(w.reshape(-1), w_i, rtol=1e-12, atol=0)
    assert np.allclose(rgb.reshape(-1), rgb_i, rtol=1e-12, atol=1e-300)
