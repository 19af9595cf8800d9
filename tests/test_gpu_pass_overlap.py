"""Pass overlap (avr_set_pass_overlap): the next pass's camera stage runs on the
side stream, into the other set of camera buffers, records and work heads, while k_paths runs.

The same kernels do the same arithmetic on the same inputs, so every test renders one sequence
of calls twice, with the overlap on and off, and asks for array_equal films. The shapes are
those of tests/test_gpu_kpaths_parked.py (the 24 x 40 x 56 cut of the cloud grid, a 48 x 32
film, ZSobol with the Gaussian filter, 8 indices per call). The sequences are the ones in which
records made ahead can be wrong or read from the wrong set: equal strides (taken), jumps,
backward steps and calls of another size (discarded), a setter between two calls that makes
them stale, readbacks and a clear directly after a call, one call split into passes, and the
configurations in which the chain stays serial."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MAXDEPTH = 100
W, H = 48, 32
NPIX = W * H


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    torch.cuda.init()


@pytest.fixture(scope="module")
def density():
    from oracle import binding
    return np.ascontiguousarray(binding.cloud_grid(56)[:, :40, :24])


def _scene(density, sampler="zsobol", filter="gaussian"):
    from acceleratedvolrenderer_amd import scenes
    base = scenes.s_cloud(density, width=W, height=H, sampler=sampler, spp=64, filter=filter)
    base.medium.majorant_res = (16, 16, 16)
    return base


def _run(scene, seq, overlap, passes, max_paths=0, lightsampler="bvh", stream=None):
    """Render the sequence `seq(integ, log)` with the overlap on or off; returns (rgb, w, log).
    Checks what holds after every sequence: stats() raises nothing, one k_paths launch per pass,
    and every stage was timed."""
    from acceleratedvolrenderer_amd import VolPathIntegrator
    integ = VolPathIntegrator(scene, maxdepth=MAXDEPTH, spp=64, seed=0, device=0, max_paths=max_paths,
                              lightsampler=lightsampler)
    try:
        if stream is not None:
            integ.ctx.set_stream(stream.cuda_stream)
        integ.ctx.set_pass_overlap(overlap)
        integ.ctx.film_clear()
        integ.ctx.reset_stats()
        log = {"active": [], "extra": []}
        seq(integ, log)
        rgb, w = integ.film_sums()
        st = integ.ctx.stats()
        assert st["medium_launches"] == passes
        assert st["ms_camera"] > 0 and st["ms_medium"] > 0 and st["ms_film"] > 0
        return rgb, w, log
    finally:
        integ.close()


def _calls(ranges):
    def seq(integ, log):
        for a, b in ranges:
            integ.ctx.render(a, b, 0, MAXDEPTH)
            log["active"].append(integ.ctx.pass_overlap_active())
    return seq


def _equal(scene, seq, passes, **kw):
    on = _run(scene, seq, True, passes, **kw)
    off = _run(scene, seq, False, passes, **kw)
    assert float(off[0].sum()) > 0
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert not any(off[2]["active"])
    return on[2], off[2]


def test_equal_stride_calls_take_the_records_made_ahead(density):
    from oracle import binding
    scene = _scene(density)
    ranges = [(8 * k, 8 * k + 8) for k in range(6)]

    def seq(integ, log):
        _calls(ranges)(integ, log)
        assert integ.ctx.last_kernel() == "k_paths<false, true, 2, 0, false, false>"
        log["extra"].append(integ.ctx.last_pass_samples(NPIX, 8))

    on, off = _equal(scene, seq, 6)
    assert on["active"] == [False] + [True] * 5
    # the last pass's records are read from the set it was rendered into: all of its samples
    # bit-identical to the canonical oracle
    first, ns, L, lam, _ = on["extra"][0]
    assert (first, ns) == (40, 8)
    canon = binding.OracleRun(scene, max_depth=MAXDEPTH, seed=0, libm="canonical")
    exact = 0
    for s in range(8):
        for pix in range(NPIX):
            Lo, lo, _, _ = canon.pixel_sample(pix % W, pix // W, 40 + s)
            g = s * NPIX + pix
            exact += int(np.array_equal(L[g].view(np.uint32), Lo.view(np.uint32)) and
                         np.array_equal(lam[g].view(np.uint32), lo.view(np.uint32)))
    print(f"last pass of six: {exact}/{NPIX * 8} samples bit-identical")
    assert exact == NPIX * 8


def test_mispredicted_passes_run_their_own_camera_stage(density):
    """A jump, a step backwards, a call that is not quad-aligned and one of another size."""
    ranges = [(0, 8), (8, 16), (16, 24), (40, 48), (24, 32), (32, 38), (38, 50)]
    on, _ = _equal(_scene(density), _calls(ranges), len(ranges))
    assert on["active"] == [False, True, True, False, False, False, False]


def _set_pixel_order(integ, scene):
    integ.ctx.set_pixel_order(np.arange(NPIX, dtype=np.int32)[::-1])


def _set_camera(integ, scene):
    from acceleratedvolrenderer_amd import capi
    f32 = lambda a: np.ascontiguousarray(np.asarray(a, np.float32))
    rfc = f32(scene.render_from_camera).copy().reshape(-1)
    rfc[3] += 0.05   # the camera's x translation
    cfr = f32(scene.camera_from_raster)
    capi._check(integ.ctx.lib.avr_camera(integ.ctx.h, int(scene.camera.type_id), capi._fp(cfr), capi._fp(rfc)))


def _set_filter(integ, scene):
    from acceleratedvolrenderer_amd import capi
    flt = scene.film.filter
    r = np.ascontiguousarray(np.asarray(flt.radius, np.float32))
    capi._check(integ.ctx.lib.avr_set_filter(integ.ctx.h, int(flt.type_id), capi._fp(r), float(flt.sigma) * 1.5))


def _set_render_mode(integ, scene):
    integ.ctx.set_render_mode(1)


def _set_sampler(integ, scene):
    from acceleratedvolrenderer_amd import capi
    capi._check(integ.ctx.lib.avr_set_sampler(integ.ctx.h, int(scene.sampler.type_id), 256))


@pytest.mark.parametrize("setter", [_set_pixel_order, _set_camera, _set_filter, _set_render_mode, _set_sampler],
                         ids=["pixel-order", "camera", "filter", "render-mode", "sampler"])
def test_a_setter_between_calls_discards_the_records(density, setter):
    scene = _scene(density)

    def seq(integ, log):
        _calls([(0, 8), (8, 16)])(integ, log)
        setter(integ, scene)
        _calls([(16, 24), (24, 32)])(integ, log)

    on, _ = _equal(scene, seq, 4)
    assert on["active"] == [False, True, False, True]
    # ... and the setter changed the film, so stale records would have shown (the pixel order
    # changes no sample, only the slot a pixel's records are in: stale ones land on other pixels)
    if setter is not _set_pixel_order:
        plain = _run(scene, _calls([(0, 8), (8, 16), (16, 24), (24, 32)]), True, 4)
        changed = _run(scene, seq, True, 4)
        assert not np.array_equal(plain[0], changed[0])


def test_readbacks_and_clear_directly_after_a_call(density):
    scene = _scene(density)

    def seq(integ, log):
        _calls([(0, 8), (8, 16)])(integ, log)
        log["extra"].append(integ.ctx.film_read(NPIX))
        dev = torch.zeros(4 * NPIX, dtype=torch.float64, device="cuda:0")
        integ.ctx.film_export_device(dev.data_ptr())
        log["extra"].append(dev.cpu().numpy())
        _calls([(16, 24)])(integ, log)
        integ.ctx.film_clear()
        _calls([(24, 32)])(integ, log)

    on, off = _equal(scene, seq, 4)
    for a, b in zip(on["extra"], off["extra"]):
        if isinstance(a, tuple):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and float(a[0].sum()) > 0
        else:
            assert np.array_equal(a, b) and float(a.sum()) > 0
    rgb, w = on["extra"][0]
    assert np.array_equal(on["extra"][1][:3 * NPIX], rgb) and np.array_equal(on["extra"][1][3 * NPIX:], w)
    # the clear and one more call leave that call alone on the film
    alone = _run(scene, _calls([(24, 32)]), False, 1)
    final = _run(scene, seq, True, 4)
    assert np.array_equal(final[0], alone[0]) and np.array_equal(final[1], alone[1])


def test_one_call_split_into_passes(density):
    on, _ = _equal(_scene(density), _calls([(0, 16)]), 4, max_paths=4 * NPIX)
    assert on["active"] == [True]   # the call's last pass took the records made during the third


def test_serial_configurations_stay_serial(density):
    ranges = [(0, 8), (8, 16), (16, 24)]
    # the independent sampler's camera stage reads the per-pass advance table, which has one buffer
    on, _ = _equal(_scene(density, sampler="independent", filter="box"), _calls(ranges), 3)
    assert on["active"] == [False] * 3
    # the power light sampler takes k_paths' image-light instantiation, which fills the register
    # file at four waves per SIMD
    on, _ = _equal(_scene(density), _calls(ranges), 3, lightsampler="power")
    assert on["active"] == [False] * 3
    # a NanoVDBMedium: four waves per SIMD at 128 VGPRs
    from acceleratedvolrenderer_amd import scenes
    vdb = scenes.s_cloud_vdb(np.ascontiguousarray(density[:24, :24, :24]), width=W, height=H, sampler="zsobol",
                             spp=64, filter="gaussian")
    on, _ = _equal(vdb, _calls(ranges), 3)
    assert on["active"] == [False] * 3
    # a caller's stream: the side stream is ordered against the context's own stream only
    stream = torch.cuda.Stream(device=0)
    on, _ = _equal(_scene(density), _calls(ranges), 3, stream=stream)
    stream.synchronize()
    assert on["active"] == [False] * 3
