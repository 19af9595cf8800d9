"""avr_render and a graph render interleaved on one context. The two integrators share the pass
plan, the kernel-argument fill, the camera and film launches and the last-pass record, and the
path integrator keeps state across calls (the pass table and camera records made ahead for the
next call, the camera sets): a graph render between two calls must leave all of that intact.

The scene is the smallest one on which pass overlap is taken: tests/test_graph_render.py's gray
non-emissive 12^3 GridMedium with its one distant light, a 16 x 16 film, ZSobol. The sequence
runs with the overlap on and off; the films must be equal bit for bit, and after every call the
last-pass readbacks must answer for the integrator that ran it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAXDEPTH = 50
NPIX = 16 * 16
KERNEL = "k_paths<false, true, 2, 0, false, false>"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


def _scene():
    from acceleratedvolrenderer_amd import scenes, GridMedium, ZSobolSampler
    from acceleratedvolrenderer_amd.scene import Scene
    base = scenes.s_uniform(n=2, width=16, height=16, variant="scatter")
    dens = (0.2 + 0.8 * np.random.default_rng(5).random((12, 12, 12), dtype=np.float32)).astype(np.float32)
    return Scene(base.camera, base.film, GridMedium(dens, sigma_a=0.4, sigma_s=6.0, g=0.5), base.lights[:1],
                 sampler=ZSobolSampler(pixelsamples=32))


def _index():
    from acceleratedvolrenderer_amd import capi
    rng = np.random.default_rng(7)
    verts = rng.random((600, 3), dtype=np.float32)
    light = (rng.random(600, dtype=np.float32) + np.float32(0.05)).astype(np.float32)
    return capi.GraphIndex(verts, light, None, radius=0.2)


def _path_pass_is_last(ctx, first):
    got_first, ns = ctx.last_pass_samples(NPIX, 8)[:2]
    assert (got_first, ns) == (first, 8)
    assert ctx.last_kernel() == KERNEL
    with pytest.raises(RuntimeError, match="not avr_graph_render"):
        ctx.graph_last_pass(NPIX, 8)


def _run(overlap):
    from acceleratedvolrenderer_amd import VolPathIntegrator
    integ = VolPathIntegrator(_scene(), maxdepth=MAXDEPTH, spp=32, seed=0, device=0)
    ctx = integ.ctx
    try:
        ctx.set_pass_overlap(overlap)
        ctx.film_clear()
        ctx.reset_stats()
        idx = _index()
        active = []
        ctx.render(0, 8, 0, MAXDEPTH)
        active.append(ctx.pass_overlap_active())
        _path_pass_is_last(ctx, 0)
        ctx.graph_render(idx, 0, 2, 0)
        counts = ctx.graph_last_pass(NPIX, 2)[3]
        assert counts.shape == (2 * NPIX,) and counts.max() > 0
        # (the wavefront path state holds the graph pass's two samples)
        assert ctx.last_pass_samples(NPIX, 8)[:2] == (0, 2)
        ctx.render(8, 16, 0, MAXDEPTH)
        active.append(ctx.pass_overlap_active())
        _path_pass_is_last(ctx, 8)
        # two calls with nothing between them: the second takes the camera records the first
        # made ahead (a readback between two calls makes them stale)
        ctx.render(16, 24, 0, MAXDEPTH)
        active.append(ctx.pass_overlap_active())
        assert ctx.last_kernel() == KERNEL
        ctx.render(24, 32, 0, MAXDEPTH)
        active.append(ctx.pass_overlap_active())
        _path_pass_is_last(ctx, 24)
        rgb, w = integ.film_sums()
        st = ctx.stats()
        assert st["medium_launches"] == 5   # four k_paths passes and the graph pass
        assert st["ms_camera"] > 0 and st["ms_medium"] > 0 and st["ms_film"] > 0
        return rgb, w, active
    finally:
        integ.close()


def test_graph_render_between_path_renders():
    on = _run(True)
    off = _run(False)
    assert float(off[0].sum()) > 0 and float(off[1].sum()) > 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert on[2] == [False, False, False, True]
    assert off[2] == [False] * 4
