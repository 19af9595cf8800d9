"""Thin-lens and spherical cameras over the medium, film and counts of tests/camera_cases.py (the
unit box, its 6^3 scattering grid, the lights of scenes.s_uniform, film 20 x 12, 8 samples,
maxdepth 6, both samplers), shared by tests/test_camera_models.py (CPU: csrc/avr_camera.h against
tests/camera_model_ref.py, the host logic, the conditions on the inputs) and
tests/test_gpu_camera_models.py (the camera stage of the device) — TEST INFRASTRUCTURE, no device.

The truth of a ray is the host-compiled chain the kernels run — the pinhole's cameraFromRaster
point, csrc/avr_camera.h, xf_ray of csrc/avr_numerics.h (chain()) — fed with the oracle's own
per-sample pFilm (a pinhole over the same film, filter and sampler: pFilm does not depend on the
camera) and the sampler's lens draw at dimensions 4 and 5 (lens_draws()). The oracle knows
pinholes only: no lens or spherical scene is handed to it."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import camera_cases as cc        # noqa: E402
import camera_model_ref as ref   # noqa: E402

ROOT = cc.ROOT
W, H, SPP, MAXDEPTH = cc.W, cc.H, cc.SPP, cc.MAXDEPTH
SPHERE = ((0.5, 0.5, 0.5), 0.6)

# "lens-sphere-outside": the pose of "persp-roll" with a field of view of 44 degrees. The origin's
# margin is measured on this pose as a pinhole (SPHERE_PINHOLE_DEVIATION), and a margin speaks only
# for rays as well conditioned as those it was measured on: the float32 crossing of a ray that
# nearly grazes the sphere errs as 1 / sqrt(discriminant). So the case's condition on its inputs
# (tests/test_camera_models.py) is that no lens ray is nearer the tangent than the nearest ray of
# the pinhole measurement. persp-roll's own 40 degrees fails it (lens 1.2e-4 of the discriminant's
# scale against the pinhole's 9.8e-4), 44 degrees holds it (5.5e-4 against 7.6e-5).
SPHERE_POSE = dict(fov=44.0, pos=(1.7, 1.6, 1.9), look=(0.45, 0.5, 0.55), up=(0.3, 1.0, -0.2))
# the largest distance of the pinhole's origin after the interface entry from the float64 first
# crossing, over both samplers' 1920 samples (the canonical oracle's entry, which the device's
# pinhole origins equal bit for bit); the lens case's margin is 4 x that
SPHERE_PINHOLE_DEVIATION = 1.66e-6
SPHERE_MARGIN = 4 * SPHERE_PINHOLE_DEVIATION

# name -> (kind, pose: a name of camera_cases.CAMERAS, keywords or None, lens / mapping keywords, filter, interface sphere)
CASES = {
    "lens-persp": ("perspective", "persp-roll", dict(lensradius=0.05, focaldistance=2.2), "box", None),
    "lens-default-focus": ("perspective", "persp-roll", dict(lensradius=0.02), "box", None),
    # (0.4, 0.55, 0.3) is 0.3 from the nearest face: a lens disc of radius 0.1 stays inside the box
    "lens-inside": ("perspective", "persp-inside", dict(lensradius=0.1), "box", None),
    "lens-ortho": ("orthographic", "ortho-oblique", dict(lensradius=0.1, focaldistance=1.5), "box", None),
    "lens-sphere-outside": ("perspective", SPHERE_POSE, dict(lensradius=0.05), "box", SPHERE),
    "sph-ea-inside": ("spherical", None, dict(mapping="equalarea", pos=(0.4, 0.55, 0.3), look=(0.9, 0.2, 1.0)), "box", None),
    "sph-er-inside": ("spherical", None, dict(mapping="equirectangular", pos=(0.4, 0.55, 0.3), look=(0.9, 0.2, 1.0)),
                      "box", None),
    "sph-ea-outside": ("spherical", None, dict(mapping="equalarea", pos=(0.5, 0.5, -0.2), look=(0.5, 0.5, 0.5)), "box", None),
    "sph-er-outside": ("spherical", None, dict(mapping="equirectangular", pos=(0.5, 0.5, -0.2), look=(0.5, 0.5, 0.5)),
                       "box", None),
    "sph-ea-wide": ("spherical", None, dict(mapping="equalarea", pos=(0.5, 0.5, -0.2), look=(0.5, 0.5, 0.5)),
                    "gauss-64", None),
}
LENS_CASES = [c for c in CASES if c.startswith("lens-")]
HIT_SHARE = {c: (0.20, 0.80) for c in CASES}
HIT_SHARE["lens-inside"] = HIT_SHARE["sph-ea-inside"] = HIT_SHARE["sph-er-inside"] = (1.0, 1.0)
SAMPLERS = cc.SAMPLERS


def make_camera(case, lens=True):
    """The camera of a case; lens=False: the same pose built without the lens arguments."""
    from acceleratedvolrenderer_amd.scene import OrthographicCamera, PerspectiveCamera, SphericalCamera
    kind, pose, kw, _, _ = CASES[case]
    if kind == "spherical":
        return SphericalCamera(up=(0.0, 1.0, 0.0), **kw)
    pk = cc.CAMERAS[pose][1] if isinstance(pose, str) else pose
    args = dict(pos=pk["pos"], look=pk["look"], up=pk["up"], screenwindow=pk.get("screenwindow"),
                frameaspectratio=pk.get("frameaspectratio"))
    if lens:
        args.update(kw)
    return OrthographicCamera(**args) if kind == "orthographic" else PerspectiveCamera(fov=pk["fov"], **args)


def scene_for(case, sampler="independent", spp=SPP, cam=None, filt=None, variant="scatter", pixelbounds=None,
              density=True):
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import IndependentSampler, RGBFilm, Scene, ZSobolSampler
    kw = dict(density=cc.density()) if density else {}
    base = scenes.s_uniform(n=cc.GRID_N, width=W, height=H, variant=variant, **kw)
    smp = IndependentSampler(pixelsamples=spp) if sampler == "independent" else ZSobolSampler(pixelsamples=spp)
    fkw = dict(filter=cc.make_filter(filt or CASES[case][3]))
    if pixelbounds is not None:
        fkw["pixelbounds"] = pixelbounds
    return Scene(make_camera(case) if cam is None else cam, RGBFilm(W, H, **fkw), base.medium, base.lights,
                 sampler=smp, interface_sphere=CASES[case][4])


def pinhole_scene(case, sampler, spp=SPP, filt=None):
    """A pinhole over the case's film, filter, sampler and interface: what the oracle is asked for
    pFilm, u, the filter weight and the wavelengths (none depends on the camera)."""
    from acceleratedvolrenderer_amd.scene import PerspectiveCamera
    cam = make_camera(case, lens=False) if CASES[case][0] != "spherical" else PerspectiveCamera(
        fov=60.0, pos=(0.5, 0.5, -1.2), look=(0.5, 0.5, 0.5), up=(0.0, 1.0, 0.0))
    return scene_for(case, sampler, spp=spp, cam=cam, filt=filt)


# ---------------------------------------------------------------------------
# float64 geometry of the pixel-centre rays (the lens centre's: the pinhole's)

def pixel_centre_rays(scene):
    cam = scene.camera
    if int(cam.type_id) != 2:
        return cc.pixel_centre_rays(scene)
    f = scene.film
    y, x = np.mgrid[0:f.height, 0:f.width]
    pf = np.stack([x.ravel() + 0.5, y.ravel() + 0.5], 1)
    d_c = ref.spherical_dir(cam.mapping, pf, (f.width, f.height), np.float64)
    m = np.asarray(scene.render_from_camera, np.float64)
    return np.tile(m[:3, 3], (len(pf), 1)), d_c @ m[:3, :3].T


def hit_share(scene):
    """The share of pixel-centre rays that cross the medium's box: camera_cases.hit_mask's slab test."""
    o, d = pixel_centre_rays(scene)
    mfr = np.asarray(scene.medium_from_render, np.float64)
    om, dm = o @ mfr[:3, :3].T + mfr[:3, 3], d @ mfr[:3, :3].T
    b = np.asarray(scene.medium.bounds, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (b[:3] - om) / dm, (b[3:] - om) / dm
    lo = np.nanmax(np.minimum(t0, t1), axis=1)
    hi = np.nanmin(np.maximum(t0, t1), axis=1)
    return float((np.maximum(lo, 0.0) < hi).mean())


def sphere_crossing(scene, o, d):
    """float64 first crossing of the interface sphere SPHERE from render-space rays (o, d):
    (crosses (n,), the point (n, 3), the discriminant over its scale a R^2 (n,): how far the ray
    is from grazing)."""
    c = (np.asarray(scene.render_from_world, np.float64) @ np.array([*SPHERE[0], 1.0]))[:3]
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    oc = o - c
    a, b, q = (d * d).sum(1), (oc * d).sum(1), (oc * oc).sum(1) - SPHERE[1] ** 2
    disc = b * b - a * q
    t = (-b - np.sqrt(np.maximum(disc, 0))) / a
    return (disc > 0) & (t > 0), o + d * t[:, None], disc / (a * SPHERE[1] ** 2)


# ---------------------------------------------------------------------------
# the host-compiled headers

_SHIM = r'''
#include "%(csrc)s/avr_numerics.h"
#include "%(csrc)s/avr_camera.h"
using namespace avr;
extern "C" {
void disk(long long n, const float *u, float *out) {
  for (long long i = 0; i < n; ++i) cam::concentric_disk(u[2 * i], u[2 * i + 1], out + 2 * i, out + 2 * i + 1); }
// rows: radius, focal, u0, u1, o[3], d[3] -> o'[3], d'[3]
void lens(long long n, const float *in, float *out) {
  for (long long i = 0; i < n; ++i) { const float *r = in + 10 * i; float *w = out + 6 * i;
    for (int k = 0; k < 3; ++k) { w[k] = r[4 + k]; w[3 + k] = r[7 + k]; }
    cam::thin_lens(r[0], r[1], r[2], r[3], w, w + 3); } }
void sph(long long n, int mapping, int resx, int resy, const float *pf, float *out) {
  for (long long i = 0; i < n; ++i) cam::spherical_dir(mapping, pf[2 * i], pf[2 * i + 1], resx, resy, out + 3 * i); }
void wrap(long long n, const float *uv, float *out) {
  for (long long i = 0; i < n; ++i) { out[2 * i] = uv[2 * i]; out[2 * i + 1] = uv[2 * i + 1];
    cam::wrap_equal_area_square(out + 2 * i, out + 2 * i + 1); } }
// the camera stage's ray: cameraFromRaster's point and the pinhole ray as the kernels state them,
// the general cameras of avr_camera.h, xf_ray(render_from_camera)
void chain(long long n, int type, const float *r, const float *rfc, float radius, float focal, int mapping, int resx,
           int resy, const float *pf, const float *lu, float *o, float *d) {
  Xf x; for (int i = 0; i < 12; ++i) x.m[i] = rfc[i];
  for (long long i = 0; i < n; ++i) {
    const float pFilmX = pf[2 * i], pFilmY = pf[2 * i + 1];
    V3 pCam = {r[0] * pFilmX + r[1] * pFilmY + r[2] * 0.f + r[3], r[4] * pFilmX + r[5] * pFilmY + r[6] * 0.f + r[7],
               r[8] * pFilmX + r[9] * pFilmY + r[10] * 0.f + r[11]};
    const float wp = r[12] * pFilmX + r[13] * pFilmY + r[14] * 0.f + r[15];
    if (wp != 1) pCam = pCam / wp;
    Ray ray;
    if (type == 0) ray = {pCam, {0.f, 0.f, 1.f}};
    else ray = {{0.f, 0.f, 0.f}, normalize(pCam)};
    float oo[3] = {ray.o.x, ray.o.y, ray.o.z}, dd[3] = {ray.d.x, ray.d.y, ray.d.z};
    if (type == 2) { oo[0] = oo[1] = oo[2] = 0.f; cam::spherical_dir(mapping, pFilmX, pFilmY, resx, resy, dd); }
    else if (radius > 0) cam::thin_lens(radius, focal, lu[2 * i], lu[2 * i + 1], oo, dd);
    ray = xf_ray(x, Ray{{oo[0], oo[1], oo[2]}, {dd[0], dd[1], dd[2]}}, nullptr, true);
    o[3 * i] = ray.o.x; o[3 * i + 1] = ray.o.y; o[3 * i + 2] = ray.o.z;
    d[3 * i] = ray.d.x; d[3 * i + 1] = ray.d.y; d[3 * i + 2] = ray.d.z; } }
// IndependentSampler: the stream of pixel (px, py), sample s — values 0..n-1 (rng.h, samplers.h:442-476)
void independent(int px, int py, int seed, long long s, int n, float *out) {
  const uint64_t seq = hash_3u32((uint32_t)px, (uint32_t)py, (uint32_t)seed);
  Pcg32 rng; rng.set_sequence(seq, mix_bits(seq)); rng.advance((uint64_t)s * 65536ull);
  for (int i = 0; i < n; ++i) out[i] = rng.uniform(); }
}
'''
_lib = None
FP = ctypes.POINTER(ctypes.c_float)


def _fp(a):
    return a.ctypes.data_as(FP)


def shim():
    """csrc/avr_camera.h and csrc/avr_numerics.h compiled for the host (g++, -ffp-contract=off, as
    tests/test_media_cases_reference.py compiles the latter)."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="camera_models_")
        src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "shim.so")
        with open(src, "w") as f:
            f.write(_SHIM % dict(csrc=os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc")))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                               "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), src, "-o", so])
        L = ctypes.CDLL(so)
        ll, i, fl = ctypes.c_longlong, ctypes.c_int, ctypes.c_float
        L.disk.argtypes = [ll, FP, FP]
        L.lens.argtypes = [ll, FP, FP]
        L.sph.argtypes = [ll, i, i, i, FP, FP]
        L.wrap.argtypes = [ll, FP, FP]
        L.chain.argtypes = [ll, i, FP, FP, fl, fl, i, i, i, FP, FP, FP, FP]
        L.independent.argtypes = [i, i, i, ll, i, FP]
        _lib = L
    return _lib


def _f32(a):
    return np.ascontiguousarray(a, np.float32)


def hdr_disk(u):
    u = _f32(u)
    out = np.zeros_like(u)
    shim().disk(len(u), _fp(u), _fp(out))
    return out


def hdr_lens(radius, focal, u, o, d):
    rows = _f32(np.column_stack([radius, focal, u, o, d]))
    out = np.zeros((len(rows), 6), np.float32)
    shim().lens(len(rows), _fp(rows), _fp(out))
    return out[:, :3], out[:, 3:]


def hdr_spherical(mapping, p_film, res):
    pf = _f32(p_film)
    out = np.zeros((len(pf), 3), np.float32)
    shim().sph(len(pf), {"equalarea": 0, "equirectangular": 1}[mapping], int(res[0]), int(res[1]), _fp(pf), _fp(out))
    return out


def chain(scene, p_film, lens_u):
    """Render-space (o, d) of the scene's camera at raster points p_film with lens draws lens_u,
    before any interface entry."""
    cam = scene.camera
    pf, lu = _f32(p_film), _f32(lens_u)
    o, d = np.zeros((len(pf), 3), np.float32), np.zeros((len(pf), 3), np.float32)
    r, rfc = _f32(scene.camera_from_raster).ravel(), _f32(scene.render_from_camera).ravel()
    shim().chain(len(pf), int(cam.type_id), _fp(r), _fp(rfc), float(cam.lensradius), float(cam.focaldistance),
                 int(getattr(cam, "mapping_id", 0)), scene.film.width, scene.film.height, _fp(pf), _fp(lu), _fp(o), _fp(d))
    return o, d


# ---------------------------------------------------------------------------
# the samplers' camera draws, per sample in the last-pass layout (record s * npix + pix)

def independent_stream(px, py, s, n, seed=0):
    out = np.zeros(n, np.float32)
    shim().independent(px, py, seed, s, n, _fp(out))
    return out


def camera_draws(sampler, spp, first, ns, seed=0, bounds=None, res=(W, H)):
    """GetCameraSample's draws and the first segment's: rows (wavelength u, filter u0, u1, time,
    lens u0, u1, h0, h1, u) for samples [first, first + ns) of the pixels of `bounds`
    (x0, y0, x1, y1; the whole film by default) of a film of full resolution `res`. ZSobol: the oracle's zsobol_stream with pattern
    "1212" (wavelength, pixel, time, lens) + "111"; independent: the project's PCG32 header."""
    from oracle import binding
    x0, y0, x1, y1 = bounds or (0, 0, res[0], res[1])
    bw, npix = x1 - x0, (x1 - x0) * (y1 - y0)
    out = np.zeros((ns * npix, 9), np.float32)
    for s in range(ns):
        for pix in range(npix):
            px, py = x0 + pix % bw, y0 + pix // bw
            if sampler == "zsobol":
                out[s * npix + pix] = binding.zsobol_stream(spp, res[0], res[1], px, py, first + s, seed, "1212111")
            else:
                out[s * npix + pix] = independent_stream(px, py, first + s, 9, seed)
    return out


def oracle_film_points(run, first, ns, bounds=None):
    """The oracle's per-sample (pFilm (n, 2), u (n), filter weight (n)) over `bounds`."""
    x0, y0, x1, y1 = bounds or (0, 0, W, H)
    bw, npix = x1 - x0, (x1 - x0) * (y1 - y0)
    pf, u, w = np.zeros((ns * npix, 2), np.float32), np.zeros(ns * npix, np.float32), np.zeros(ns * npix, np.float32)
    for s in range(ns):
        for pix in range(npix):
            g = s * npix + pix
            _, _, u[g], pf[g], w[g] = run.camera_ray(x0 + pix % bw, y0 + pix // bw, first + s)
    return pf, u, w


_truth = {}


def truth(case, sampler, spp=SPP, first=0, ns=SPP, filt=None):
    """(scene, o, d, u, weight, p_film, lens draws) of a case: the chain's rays before any interface
    entry; u, weight and pFilm are the canonical oracle's for a pinhole over the same film. Asserts
    first that the draws routine reproduces the oracle's u (column 8) — the check of the routine
    that hands out the lens draw (columns 4, 5)."""
    key = (case, sampler, spp, first, ns, filt)
    if key not in _truth:
        from oracle import binding
        scene = scene_for(case, sampler, spp=spp, filt=filt)
        run = binding.OracleRun(pinhole_scene(case, sampler, spp=spp, filt=filt), max_depth=MAXDEPTH, seed=0,
                                libm="canonical")
        pf, u, w = oracle_film_points(run, first, ns)
        draws = camera_draws(sampler, spp, first, ns)
        assert cc.same_bits(draws[:, 8], u).all(), "the draws routine does not reproduce the pinhole's u"
        o, d = chain(scene, pf, draws[:, 4:6])
        _truth[key] = (scene, o, d, u, w, pf, draws[:, 4:6])
    return _truth[key]
