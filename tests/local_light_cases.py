"""PointLight and SpotLight cases shared by tests/test_local_lights.py (CPU: csrc/avr_local_light.h,
host-compiled, against tests/local_light_ref.py) and tests/test_gpu_local_lights.py (the device
against the host-compiled header, the oracle anchors, the known answer) — TEST INFRASTRUCTURE.

All scenes are tests/light_cases.py's: the unit box [0, 1]^3 with a 6^3 random scattering grid, the
orthographic camera of scenes.s_uniform at (0.5, 0.5, -1) looking down +z, film 20 x 12, 8 samples
per pixel, maxdepth 6. Light positions are world-space; render space is world - (0.5, 0.5, -1).

  LIGHTS   named point and spot lights: inside the box, outside it, a narrow and a wide cone, a
           cone with conedeltaangle 0 (SmoothStep's a == b branch), zero intensity.
  LISTS    the render cases: one point light, one spot light, a point light with a distant one,
           eight mixed lights (lights past the k_paths LDS records, a zero-phi one in the middle).
  BVH      light lists of 1, 2, 3 and 8 for the tree: collinear and coincident points, a point and
           a spot light, a zero-phi light among live ones, all zero. Coincident lights differ in
           power: equal ones would put the traversal's bin edges on k / 8, which
           light_cases.PICK_U probes on purpose, and more than 2 % of the draws would sit on an edge."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np

import light_cases as lc

ROOT = lc.ROOT
W, H, SPP, MAXDEPTH = lc.W, lc.H, lc.SPP, lc.MAXDEPTH
CAM = np.array([0.5, 0.5, -1.0])

# name -> ("point" | "spot", keywords of scene.PointLight / scene.SpotLight)
LIGHTS = {
    "p-centre": ("point", dict(from_=(0.5, 0.5, 0.5), scale=3.0)),
    "p-inside": ("point", dict(from_=(0.3, 0.7, 0.4), scale=2.0)),
    "p-outside": ("point", dict(from_=(1.6, 1.2, -0.3), scale=8.0)),
    "p-far": ("point", dict(from_=(-2.0, 0.4, 0.6), I=("blackbody", 3200.0), scale=30.0)),
    "p-zero": ("point", dict(from_=(0.4, 0.4, 0.4), scale=0.0)),
    "p-power": ("point", dict(from_=(0.8, 0.2, 0.9), power=40.0)),
    "s-in": ("spot", dict(from_=(0.5, 1.4, 0.5), to=(0.5, 0.0, 0.5), coneangle=35.0, conedeltaangle=10.0, scale=12.0)),
    "s-wide": ("spot", dict(from_=(0.2, 0.2, 0.2), to=(0.9, 0.8, 0.7), coneangle=80.0, conedeltaangle=30.0, scale=4.0)),
    "s-sharp": ("spot", dict(from_=(-0.4, 0.5, 0.5), to=(1.0, 0.5, 0.5), coneangle=25.0, conedeltaangle=0.0, scale=6.0)),
    "s-power": ("spot", dict(from_=(0.5, 0.5, -0.5), to=(0.5, 0.5, 1.0), coneangle=40.0, conedeltaangle=5.0, power=60.0,
                             I=0.7)),
    # aimed away from the box, which lies wholly outside its cone: importance 0 at every point of it
    "s-away": ("spot", dict(from_=(0.5, 0.5, -0.5), to=(0.5, 0.5, -2.0), coneangle=30.0, conedeltaangle=5.0, scale=5.0)),
}

# name -> (light specs, g). A spec is a LIGHTS name, a light_cases.DISTANT name, or
# (LIGHTS name, light_cases.TRANSFORMS name) for a world_from_light.
LISTS = {
    "point": (["p-inside"], 0.3),
    "spot": (["s-in"], 0.3),
    "point+distant": (["p-centre", "distant-base"], 0.3),
    "eight-mixed": (["distant-rot", "p-outside", "s-wide", "uniform-d65", "p-zero", "s-sharp", ("p-far", "rot-axis"),
                     "p-power"], 0.3),
}
SAMPLERS = ("bvh", "uniform", "power")

# the tree cases: name -> light specs
_line = [("point", dict(from_=(0.1 + 0.1 * k, 0.5, 0.5), scale=1.0 + k)) for k in range(8)]
BVH = {
    "one-point": ["p-inside"],
    "one-spot": ["s-in"],
    "two-coincident": [("point", dict(from_=(0.3, 0.7, 0.4), scale=2.0)), ("point", dict(from_=(0.3, 0.7, 0.4), scale=4.6))],
    "point+spot": ["p-centre", "s-wide"],
    "three-collinear": _line[:3],
    "three-zero-among-live": ["p-outside", "p-zero", "s-in"],
    "three-all-zero": ["p-zero", "p-zero", "p-zero"],
    "eight-collinear": _line,
    "eight-coincident": [("point", dict(from_=(0.5, 0.5, 0.5), scale=1.0 + 0.37 * k * k)) for k in range(8)],
    "eight-mixed": LISTS["eight-mixed"][0],
    "eight-spread": ["p-centre", "p-inside", "p-outside", "p-far", "s-in", "s-wide", "s-sharp", "s-power"],
    "infinite+locals": ["distant-base", "p-inside", "uniform-d65", "s-in", "p-outside"],
}


def make_light(spec):
    """The scene light of a spec."""
    from acceleratedvolrenderer_amd.scene import PointLight, SpotLight
    xform = None
    if isinstance(spec, tuple) and isinstance(spec[1], str):
        spec, xform = spec
    if isinstance(spec, str) and spec in lc.DISTANT:
        return lc.make_light(spec)
    kind, kw = LIGHTS[spec] if isinstance(spec, str) else spec
    kw = dict(kw)
    if "I" in kw:
        kw["I"] = lc._spectrum(kw["I"])
    if xform is not None:
        kw["world_from_light"] = lc.transform(xform)
    return (PointLight if kind == "point" else SpotLight)(**kw)


def scene_of(specs, g=0.3, sampler="independent", spp=SPP, interface_sphere=None, medium=None, film=None):
    from acceleratedvolrenderer_amd import scenes
    from acceleratedvolrenderer_amd.scene import GridMedium, IndependentSampler, RGBFilm, Scene, ZSobolSampler
    lights = [s if hasattr(s, "type_id") else make_light(s) for s in specs]
    base = scenes.s_uniform(n=lc.GRID_N, width=W, height=H, variant="scatter", density=lc.density())
    med = GridMedium(lc.density(), sigma_a=0.5, sigma_s=2.0, g=g) if medium is None else medium
    smp = IndependentSampler(pixelsamples=spp) if sampler == "independent" else ZSobolSampler(pixelsamples=spp)
    return Scene(base.camera, RGBFilm(W, H) if film is None else film, med, lights, sampler=smp,
                 interface_sphere=interface_sphere)


def scene_for(case, **kw):
    specs, g = LISTS[case]
    return scene_of(specs, g=g, **kw)


def is_general(scene):
    """Whether k_paths runs a general instantiation: an image or local light (or the power sampler)."""
    return any(l.type_id >= 2 for l in scene.lights)


def lattice(n=5, lo=-0.25, hi=1.25):
    """Render-space points on an n^3 lattice through and around the box (world [lo, hi]^3)."""
    t = np.linspace(lo, hi, n)
    g = np.stack(np.meshgrid(t, t, t, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(g - CAM, np.float32)


def box_lattice(n=7):
    """Render-space lattice over the box itself, faces included."""
    return lattice(n, 0.0, 1.0)


def pick_inputs(n=5):
    """Every lattice point with every draw of light_cases.PICK_U: (p (N, 3), u (N))."""
    p = lattice(n)
    u = lc.PICK_U
    return (np.ascontiguousarray(np.repeat(p, len(u), axis=0)), np.ascontiguousarray(np.tile(u, len(p))))


def probe_points(scene, index):
    """Render-space reference points for SampleLi of light `index`: the lattice, points on the
    light's axis, on the cone's two edges, inside and outside it, at the light, and 1e-6 and 1e6
    away from it."""
    m = np.asarray(scene.light_rfl[index], np.float64)
    light = scene.lights[index]
    pl = m[:3, 3]
    ax = m[:3, :3] @ np.array([0.0, 0.0, 1.0])
    ax /= np.linalg.norm(ax)
    sx = m[:3, :3] @ np.array([1.0, 0.0, 0.0])
    sx -= ax * (sx @ ax)
    sx /= np.linalg.norm(sx)
    pts = [pl, pl + 0.7 * ax, pl - 0.7 * ax, pl + 1e-6 * ax, pl + 1e6 * ax, pl + 1e-6 * sx, pl + 1e6 * (ax + 0.1 * sx)]
    cs, ce = float(light.cos_falloff_start), float(light.cos_falloff_end)
    for c in (cs, ce, 0.5 * (cs + ce), min(1.0, cs + 0.01), ce - 0.01):
        c = float(np.clip(c, -1.0, 1.0))
        pts.append(pl + 0.9 * (c * ax + np.sqrt(max(0.0, 1 - c * c)) * sx))
    return np.ascontiguousarray(np.concatenate([np.array(pts), lattice(4).astype(np.float64)]), np.float32)


def light_records(scene):
    """Per light what the C ABI receives: (types, rfl (n, 16), lfr (n, 16), scale, max I, cos start, cos end)."""
    n = len(scene.lights)
    types = np.array([l.type_id for l in scene.lights], np.int32)
    eye = np.eye(4, dtype=np.float32)
    rfl = np.stack([np.asarray(scene.light_rfl[i], np.float32) if types[i] >= 3 else eye for i in range(n)])
    lfr = np.stack([np.asarray(scene.light_lfr[i], np.float32) if types[i] >= 3 else eye for i in range(n)])
    scale = np.array([l.scale for l in scene.lights], np.float32)
    max_i = np.array([np.asarray(l.L, np.float32).max() for l in scene.lights], np.float32)
    cs = np.array([getattr(l, "cos_falloff_start", 1.0) for l in scene.lights], np.float32)
    ce = np.array([getattr(l, "cos_falloff_end", -1.0) for l in scene.lights], np.float32)
    return types, rfl.reshape(n, 16), lfr.reshape(n, 16), scale, max_i, cs, ce


def ref_tree(scene):
    """tests/local_light_ref.py's Tree of a scene's light list, and per node-building light its LB."""
    import local_light_ref as ref
    types, rfl, _, scale, max_i, cs, ce = light_records(scene)
    bounds = []
    for i, t in enumerate(types):
        if t < 3:
            bounds.append(None)
        elif t == 3:
            bounds.append(ref.point_bounds(rfl[i].reshape(4, 4), scale[i], max_i[i]))
        else:
            bounds.append(ref.spot_bounds(rfl[i].reshape(4, 4), scale[i], max_i[i], cs[i], ce[i]))
    return ref.Tree(bounds), bounds


# ---------------------------------------------------------------------------
# the host-compiled header

_SHIM = r'''
#include "%(csrc)s/avr_numerics.h"
#include "%(csrc)s/avr_local_light.h"
using namespace avr;
static ll::Tree g_tree;
extern "C" {
// BVHLightSampler's constructor over a light list (types < 3: infinite lights); the node arrays as
// avr_light_bvh returns them. Returns the node count; the tree stays for pick().
int build(int n, const int *types, const float *rfl, const float *scale, const float *maxI, const float *cs,
          const float *ce, float *phi, float *w3, int *qcos, int *qb, int *link, int *leaf, float *allb, int *ninf) {
  bool bounded[8]; ll::LightBounds lb[8];
  for (int i = 0; i < n; ++i) { bounded[i] = types[i] >= ll::kPoint;
    if (bounded[i]) lb[i] = ll::light_bounds(types[i], rfl + 16 * i, scale[i], maxI[i], cs[i], ce[i]); }
  ll::build_tree(n, bounded, lb, &g_tree);
  for (int i = 0; i < g_tree.nNodes; ++i) { const ll::Node &nd = g_tree.nodes[i];
    phi[i] = nd.phi; ll::oct_decode(nd.wx, nd.wy, w3 + 3 * i);
    qcos[2 * i] = (int)nd.q_cos_o(); qcos[2 * i + 1] = (int)nd.q_cos_e();
    for (int k = 0; k < 6; ++k) qb[6 * i + k] = nd.qb[k / 3][k %% 3];
    link[i] = (int)nd.index(); leaf[i] = nd.leaf(); }
  for (int k = 0; k < 6; ++k) allb[k] = g_tree.allb[k];
  *ninf = g_tree.nInf;
  return g_tree.nNodes; }
void pick(long long n, const float *p, const float *u, int *idx, float *pmf) {
  for (long long i = 0; i < n; ++i) { float pm = 0.f; idx[i] = ll::bvh_sample(g_tree, p + 3 * i, u[i], &pm);
    pmf[i] = idx[i] >= 0 ? pm : 0.f; } }
float pmf_infinite() { return ll::bvh_pmf_infinite(g_tree); }
// SampleLi at n points: I = the 471-entry table at the wavelengths lam4
void sample(long long n, int type, const float *rfl, const float *lfr16, float cs, float ce, float scale, const float *L,
            const float *lam4, const float *p, float *wi, float *Li, float *dist, float *I4) {
  float pl[3], lfr[9]; ll::light_position(rfl, pl);
  for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) lfr[3 * r + k] = lfr16[4 * r + k];
  for (long long i = 0; i < n; ++i) { float d2, fo;
    ll::sample_li(type, pl, lfr, cs, ce, p + 3 * i, wi + 3 * i, &d2, &fo);
    const Spec lam = {lam4[4 * i], lam4[4 * i + 1], lam4[4 * i + 2], lam4[4 * i + 3]};
    const Spec I = sample_table(L, lambda_index(lam));
    const float iv[4] = {I.v0, I.v1, I.v2, I.v3};
    for (int k = 0; k < 4; ++k) { I4[4 * i + k] = iv[k]; Li[4 * i + k] = ll::li_channel(type, fo, scale, iv[k], d2); }
    const float d[3] = {pl[0] - p[3 * i], pl[1] - p[3 * i + 1], pl[2] - p[3 * i + 2]};
    dist[i] = ll::length3(d); } }
}
'''
_lib = None
FP = ctypes.POINTER(ctypes.c_float)
IP = ctypes.POINTER(ctypes.c_int)


def _fp(a):
    return a.ctypes.data_as(FP)


def _ip(a):
    return a.ctypes.data_as(IP)


def shim():
    """csrc/avr_local_light.h compiled for the host (g++, -ffp-contract=off, as
    tests/camera_model_cases.py compiles the camera header)."""
    global _lib
    if _lib is None:
        d = tempfile.mkdtemp(prefix="local_lights_")
        src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "shim.so")
        with open(src, "w") as f:
            f.write(_SHIM % dict(csrc=os.path.join(ROOT, "acceleratedvolrenderer_amd", "csrc")))
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__",
                               "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "include"), src, "-o", so])
        L = ctypes.CDLL(so)
        ll, i, fl = ctypes.c_longlong, ctypes.c_int, ctypes.c_float
        L.build.argtypes = [i, IP, FP, FP, FP, FP, FP, FP, FP, IP, IP, IP, IP, FP, IP]
        L.pick.argtypes = [ll, FP, FP, IP, FP]
        L.pmf_infinite.restype = fl
        L.sample.argtypes = [ll, i, FP, FP, fl, fl, fl, FP, FP, FP, FP, FP, FP, FP]
        _lib = L
    return _lib


def hdr_build(scene):
    """The header's tree of a scene's light list, as Context.light_bvh() returns it."""
    types, rfl, _, scale, max_i, cs, ce = light_records(scene)
    phi, w, qcos, qb = np.zeros(15, np.float32), np.zeros((15, 3), np.float32), np.zeros((15, 2), np.int32), np.zeros(
        (15, 2, 3), np.int32)
    link, leaf, allb, ninf = np.zeros(15, np.int32), np.zeros(15, np.int32), np.zeros(6, np.float32), np.zeros(1, np.int32)
    rfl = np.ascontiguousarray(rfl)
    k = shim().build(len(types), _ip(types), _fp(rfl), _fp(scale), _fp(max_i), _fp(cs), _fp(ce), _fp(phi), _fp(w),
                     _ip(qcos), _ip(qb), _ip(link), _ip(leaf), _fp(allb), _ip(ninf))
    return dict(phi=phi[:k], w=w[:k], qcos=qcos[:k], qb=qb[:k], link=link[:k], leaf=leaf[:k].astype(bool),
                all_bounds=allb, n_infinite=int(ninf[0]))


def hdr_pick(scene, p, u):
    """BVHLightSampler::Sample of the header over a scene's list: (index, pmf)."""
    hdr_build(scene)
    p, u = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(u, np.float32)
    idx, pmf = np.zeros(len(u), np.int32), np.zeros(len(u), np.float32)
    shim().pick(len(u), _fp(p), _fp(u), _ip(idx), _fp(pmf))
    return idx, pmf


def hdr_pmf_infinite(scene):
    hdr_build(scene)
    return np.float32(shim().pmf_infinite())


def hdr_sample(scene, index, p, lam):
    """SampleLi of the header for light `index`: (wi, Li, distance, I at the wavelengths)."""
    types, rfl, lfr, scale, _, cs, ce = light_records(scene)
    p, lam = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(lam, np.float32)
    n = len(p)
    L = np.ascontiguousarray(scene.lights[index].L, np.float32)
    wi, Li, dist, I4 = (np.zeros((n, 3), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32),
                        np.zeros((n, 4), np.float32))
    r, f = np.ascontiguousarray(rfl[index]), np.ascontiguousarray(lfr[index])
    shim().sample(n, int(types[index]), _fp(r), _fp(f), float(cs[index]), float(ce[index]), float(scale[index]), _fp(L),
                  _fp(lam), _fp(p), _fp(wi), _fp(Li), _fp(dist), _fp(I4))
    return wi, Li, dist, I4
