"""Scene description for the volumetric path: the subset of pbrt-v4 scene objects
the MI355X integrator consumes, with pbrt's parameter names and defaults.

    GridMedium            media.h:265-352, GridMedium::Create media.cpp:249-330
    DistantLight          lights.h:244-305, DistantLight::Create lights.cpp:246-276
    UniformInfiniteLight  lights.cpp:950-972, creation lights.cpp:1529-1566
    Orthographic/PerspectiveCamera  cameras.h:245-273, cameras.cpp:284-306, 404-427, 365-400, 490-520
    RGBFilm + PixelSensor film.h:95-100, 232-316; film.cpp:212-250, 484-497, 567-585
    CameraTransform       cameras.cpp:27-57 (default rendering space: CameraWorld)

The medium's box `[p0, p1]` doubles as the scene's only geometry: an "interface"
boundary (no BSDF; rays cross it without scattering, interaction.cpp:91-97).
See DESIGN.md "Scene model" for why that is exact for VolPath's sampling.
"""
import math
import warnings

import numpy as np

from . import spectra
from . import transform as xf


class GridMedium:
    """pbrt "uniformgrid" medium (GridMedium::Create, media.cpp:249-330).

    density: float32 array shaped (nz, ny, nx) (x fastest, containers.h:834), or a
    device tensor with `.data_ptr()` (kept alive by the caller) plus `shape`.
    """

    def __init__(self, density, p0=(0.0, 0.0, 0.0), p1=(1.0, 1.0, 1.0), world_from_medium=None, sigma_a=None,
                 sigma_s=None, scale=1.0, g=0.0, Le=None, Lescale=None, majorant_res=(16, 16, 16), temperature=None,
                 temperaturescale=1.0, temperatureoffset=0.0):
        if hasattr(density, "data_ptr"):
            check_device_grid(density, "density", 3)
            self.device_density = density
            self.density = None
            nz, ny, nx = (int(s) for s in density.shape)
        else:
            d = np.ascontiguousarray(np.asarray(density, np.float32))
            if d.ndim != 3:
                raise ValueError("density must be (nz, ny, nx)")
            self.device_density = None
            self.density = d
            nz, ny, nx = d.shape
        self.nx, self.ny, self.nz = nx, ny, nz
        self.p0 = np.asarray(p0, np.float32)
        self.p1 = np.asarray(p1, np.float32)
        self.world_from_medium = np.eye(4) if world_from_medium is None else np.asarray(world_from_medium, np.float64)
        self.g = np.float32(g)
        # DenselySampledSpectrum(sigma).Scale(sigmaScale) (media.cpp:229-231), defaults 1 (media.cpp:313-320)
        self.sigma_a = spectra.scaled(spectra.as_table(sigma_a, 1.0), scale)
        self.sigma_s = spectra.scaled(spectra.as_table(sigma_s, 1.0), scale)
        # Le / LeScale (media.cpp:283-305)
        le_norm = np.float32(1.0)
        if Le is None or float(np.max(spectra.as_table(Le, 0.0))) == 0.0:
            self.Le = None
        else:
            self.Le = spectra.as_table(Le, 0.0)
            le_norm = np.float32(1.0) / spectra.spectrum_to_photometric(self.Le)
        if Lescale is None:
            self.Lescale = np.array([[[le_norm]]], np.float32)
        else:
            ls = np.asarray(Lescale, np.float32)
            if ls.shape != (nz, ny, nx):
                raise ValueError("Lescale must match the density grid shape")
            self.Lescale = (ls * le_norm).astype(np.float32)
        self.majorant_res = tuple(int(r) for r in majorant_res)
        # temperature grid (media.cpp:255-266, 321-326): blackbody emission, exclusive with Le
        self.temperature = None
        if temperature is not None:
            if self.Le is not None:
                raise ValueError('Both "Le" and "temperature" values were provided.')
            t = np.ascontiguousarray(np.asarray(temperature, np.float32))
            if t.shape != (nz, ny, nx):
                raise ValueError("temperature must match the density grid shape")
            self.temperature = t
        self.temperature_scale = np.float32(temperaturescale)
        self.temperature_offset = np.float32(temperatureoffset)

    type_id = 0

    @property
    def bounds(self):
        return np.concatenate([self.p0, self.p1]).astype(np.float32)


class _AnalyticMedium:
    """Shared surface of the media without a density grid (the C-ABI and the oracle see a
    1^3 grid of 1.0 and a 1^3 majorant; the kernels never read them)."""
    device_density = None
    nx = ny = nz = 1
    majorant_res = (1, 1, 1)

    def _box(self, p0, p1, world_from_medium):
        self.p0 = np.asarray(p0, np.float32)
        self.p1 = np.asarray(p1, np.float32)
        self.world_from_medium = np.eye(4) if world_from_medium is None else np.asarray(world_from_medium, np.float64)
        self.density = np.ones((1, 1, 1), np.float32)
        self.Lescale = np.ones((1, 1, 1), np.float32)

    @property
    def bounds(self):
        return np.concatenate([self.p0, self.p1]).astype(np.float32)


class HomogeneousMedium(_AnalyticMedium):
    """pbrt "homogeneous" medium (HomogeneousMedium::Create, media.cpp:166-200): sigma_a,
    sigma_s (default 1) x scale, g, Le (illuminant) x Lescale / photometric(Le). pbrt's
    medium is unbounded; here it fills the interface box [p0, p1] (its majorant segment is
    the box crossing, as the box's interface surfaces would bound it in pbrt)."""
    type_id = 1

    def __init__(self, p0=(0.0, 0.0, 0.0), p1=(1.0, 1.0, 1.0), world_from_medium=None, sigma_a=None, sigma_s=None,
                 scale=1.0, g=0.0, Le=None, Lescale=1.0):
        self._box(p0, p1, world_from_medium)
        self.g = np.float32(g)
        self.sigma_a = spectra.scaled(spectra.as_table(sigma_a, 1.0), scale)
        self.sigma_s = spectra.scaled(spectra.as_table(sigma_s, 1.0), scale)
        if Le is None or float(np.max(spectra.as_table(Le, 0.0))) == 0.0:
            self.Le = None
        else:
            le = spectra.as_table(Le, 0.0)
            self.Le = spectra.scaled(le, np.float32(np.float32(Lescale) / spectra.spectrum_to_photometric(le)))


class CloudMedium(_AnalyticMedium):
    """pbrt "cloud" medium (CloudMedium::Create, media.cpp:463-484): procedural Perlin
    density (density 1, wispiness 1, frequency 5), sigma_a / sigma_s default 1 (no scale
    parameter in pbrt), g, bounds p0/p1."""
    type_id = 2

    def __init__(self, p0=(0.0, 0.0, 0.0), p1=(1.0, 1.0, 1.0), world_from_medium=None, sigma_a=None, sigma_s=None,
                 g=0.0, density=1.0, wispiness=1.0, frequency=5.0):
        self._box(p0, p1, world_from_medium)
        self.g = np.float32(g)
        self.sigma_a = spectra.as_table(sigma_a, 1.0)
        self.sigma_s = spectra.as_table(sigma_s, 1.0)
        self.Le = None
        self.cloud = (np.float32(density), np.float32(wispiness), np.float32(frequency))


class NanoVDBMedium:
    """pbrt "nanovdb" medium (NanoVDBMedium::Create, media.cpp:618-665; ctor 511-616):
    `density` and optional `temperature` are NanoVDBGrid trees (vdb.py) in place of the
    "filename" / "gridname" / "temperaturename" file read. sigma_a / sigma_s default 1,
    x "scale"; "g"; "Lescale" (default 1); "temperatureoffset" (falls back to
    "temperaturecutoff", default 0); "temperaturescale" (default 1). Bounds = the density
    grid's world bbox union the temperature grid's; 64^3 majorant."""
    type_id = 3
    device_density = None
    nx = ny = nz = 1
    majorant_res = (64, 64, 64)
    temperature = None   # (GridMedium's dense temperature grid; this medium's is temperature_grid)

    def __init__(self, density, temperature=None, world_from_medium=None, sigma_a=None, sigma_s=None, scale=1.0,
                 g=0.0, Lescale=1.0, temperatureoffset=None, temperaturecutoff=0.0, temperaturescale=1.0):
        self.grid = density
        self.temperature_grid = temperature
        p0, p1 = density.world_bbox()
        if temperature is not None:
            t0, t1 = temperature.world_bbox()
            p0, p1 = np.minimum(p0, t0), np.maximum(p1, t1)
        self.p0, self.p1 = p0.astype(np.float32), p1.astype(np.float32)
        self.world_from_medium = np.eye(4) if world_from_medium is None else np.asarray(world_from_medium, np.float64)
        self.g = np.float32(g)
        self.sigma_a = spectra.scaled(spectra.as_table(sigma_a, 1.0), scale)
        self.sigma_s = spectra.scaled(spectra.as_table(sigma_s, 1.0), scale)
        self.Le = None
        self.Lescale_value = np.float32(Lescale)
        self.temperature_offset = np.float32(temperaturecutoff if temperatureoffset is None else temperatureoffset)
        self.temperature_scale = np.float32(temperaturescale)
        self.density = None
        self.Lescale = np.ones((1, 1, 1), np.float32)

    @property
    def bounds(self):
        return np.concatenate([self.p0, self.p1]).astype(np.float32)


def check_device_grid(t, name, ndim):
    """A grid handed to the device entry points as a tensor: float32 (the kernels read f32 /
    float4 elements, so a narrower dtype would be read past its end), contiguous, on a GPU."""
    if str(getattr(t, "dtype", "")) != "torch.float32":
        raise ValueError(f"{name} tensor must be float32 (got {getattr(t, 'dtype', None)})")
    if t.dim() != ndim or not t.is_contiguous():
        raise ValueError(f"{name} tensor must be contiguous with {ndim} dimensions")
    if getattr(t.device, "type", None) != "cuda":
        raise ValueError(f"{name} tensor must live on a GPU (got {t.device}); pass a numpy array for host data")


class RGBGridMedium:
    """pbrt "rgbgrid" medium (RGBGridMedium::Create, media.cpp:380-453): per-voxel RGB
    "sigma_a" / "sigma_s" (RGBUnboundedSpectrum) and "Le" (RGBIlluminantSpectrum) arrays
    shaped (nz, ny, nx, 3), converted with `rgb_table` (rgbspectrum.RGBToSpectrumTable of
    the colour space, sRGB by default); or the converted {c0, c1, c2, scale} arrays
    (nz, ny, nx, 4) directly as sigma_a_coeffs / sigma_s_coeffs / Le_coeffs. "p0"/"p1"
    bounds, "scale" (sigmaScale), "g", "Lescale" (default 1). `illuminant`: the colour
    space's illuminant table (default D65 = sRGB's). Coefficient arrays may be device tensors
    (torch, float32 (nz, ny, nx, 4) on the context's GPU): they are then used in place
    (avr_medium_rgbgrid_device) and `on_device` is True."""
    type_id = 4
    on_device = False
    device_density = None
    majorant_res = (16, 16, 16)
    temperature = None
    Le = None

    def __init__(self, sigma_a=None, sigma_s=None, Le=None, p0=(0.0, 0.0, 0.0), p1=(1.0, 1.0, 1.0),
                 world_from_medium=None, scale=1.0, g=0.0, Lescale=1.0, rgb_table=None, illuminant=None,
                 sigma_a_coeffs=None, sigma_s_coeffs=None, Le_coeffs=None):
        def conv(rgb, coeffs, name):
            if coeffs is not None and hasattr(coeffs, "data_ptr"):
                if tuple(coeffs.shape[3:]) != (4,) or coeffs.dim() != 4:
                    raise ValueError(f"{name}_coeffs must be a contiguous (nz, ny, nx, 4) tensor")
                check_device_grid(coeffs, f"{name}_coeffs", 4)
                self.on_device = True
                return coeffs
            if coeffs is not None:
                c = np.ascontiguousarray(np.asarray(coeffs, np.float32))
                if c.ndim != 4 or c.shape[3] != 4:
                    raise ValueError(f"{name}_coeffs must be (nz, ny, nx, 4)")
                return c
            if rgb is None:
                return None
            v = np.asarray(rgb, np.float32)
            if v.ndim != 4 or v.shape[3] != 3:
                raise ValueError(f"{name} must be (nz, ny, nx, 3) RGB")
            if rgb_table is None:
                raise ValueError(f"{name} given as RGB needs rgb_table (rgbspectrum.RGBToSpectrumTable)")
            return np.ascontiguousarray(rgb_table.spectrum_coeffs(v))

        self.rgb_sigma_a = conv(sigma_a, sigma_a_coeffs, "sigma_a")
        self.rgb_sigma_s = conv(sigma_s, sigma_s_coeffs, "sigma_s")
        self.rgb_Le = conv(Le, Le_coeffs, "Le")
        given = [x for x in (self.rgb_sigma_a, self.rgb_sigma_s, self.rgb_Le) if x is not None]
        if self.on_device:
            # the device entry point takes device pointers for every grid: no host arrays mixed in
            if not all(hasattr(x, "data_ptr") for x in given):
                raise ValueError("RGB grids given as device tensors must all be device tensors (got a host array too)")
            if len({(x.device.type, x.device.index) for x in given}) != 1:
                raise ValueError("RGB grids given as device tensors must all live on the same GPU")
        if self.rgb_sigma_a is None and self.rgb_sigma_s is None:
            raise ValueError('RGB grid requires "sigma_a" and/or "sigma_s" parameter values.')
        if self.rgb_Le is not None and self.rgb_sigma_a is None:
            raise ValueError('RGB grid requires "sigma_a" if "Le" value provided.')
        grids = [x for x in (self.rgb_sigma_a, self.rgb_sigma_s, self.rgb_Le) if x is not None]
        if any(x.shape != grids[0].shape for x in grids):
            raise ValueError("sigma_a, sigma_s and Le must have the same number of samples")
        self.nz, self.ny, self.nx = grids[0].shape[:3]
        self.p0 = np.asarray(p0, np.float32)
        self.p1 = np.asarray(p1, np.float32)
        self.world_from_medium = np.eye(4) if world_from_medium is None else np.asarray(world_from_medium, np.float64)
        self.g = np.float32(g)
        self.sigma_scale = np.float32(scale)
        self.Le_scale = np.float32(Lescale)
        self.illuminant = (spectra.TABLES["D65"] if illuminant is None else spectra.as_table(illuminant, 0.0)).astype(np.float32)
        # SampleRay's sigma_t = 1 (media.h:417) through the shared tables
        self.sigma_a = np.ones(spectra.N, np.float32)
        self.sigma_s = np.zeros(spectra.N, np.float32)
        self.density = None
        self.Lescale = np.ones((1, 1, 1), np.float32)

    @property
    def bounds(self):
        return np.concatenate([self.p0, self.p1]).astype(np.float32)


class DistantLight:
    """DistantLight::Create (lights.cpp:246-276). L defaults to the color space illuminant."""
    type_id = 0

    def __init__(self, from_=(0.0, 0.0, 0.0), to=(0.0, 0.0, 1.0), L=None, scale=1.0, illuminance=None,
                 world_from_light=None):
        self.L = spectra.TABLES["D65"].copy() if L is None else spectra.as_table(L, 1.0)
        sc = np.float32(scale) / spectra.spectrum_to_photometric(self.L)
        if illuminance is not None and illuminance > 0:
            sc = np.float32(sc * np.float32(illuminance))
        self.scale = np.float32(sc)
        w = np.asarray(from_, np.float64) - np.asarray(to, np.float64)
        self.w_light = w / np.linalg.norm(w)
        self.world_from_light = np.eye(4) if world_from_light is None else np.asarray(world_from_light, np.float64)

    def render_direction(self, render_from_world):
        """Normalize(renderFromLight(Vector3f(0, 0, 1))) (lights.h:287)."""
        v = (render_from_world @ self.world_from_light)[:3, :3] @ self.w_light
        return (v / np.linalg.norm(v)).astype(np.float32)


class UniformInfiniteLight:
    """"infinite" light with constant L (lights.cpp:1529-1566); scale /= SpectrumToPhotometric, and
    with "illuminance" E_v > 0 scale *= E_v / Pi (the illuminance of a uniform hemisphere)."""
    type_id = 1

    def __init__(self, L=None, scale=1.0, illuminance=None):
        self.L = spectra.TABLES["D65"].copy() if L is None else spectra.as_table(L, 1.0)
        sc = np.float32(np.float32(scale) / spectra.spectrum_to_photometric(self.L))
        if illuminance is not None and illuminance > 0:
            sc = np.float32(sc * np.float32(np.float32(illuminance) / np.float32(math.pi)))
        self.scale = sc

    def render_direction(self, render_from_world):
        return np.zeros(3, np.float32)


class ImageInfiniteLight:
    """"infinite" light with "filename" (ImageInfiniteLight, lights.h:552-640; Create
    lights.cpp:1568-1660): a square equal-area octahedral RGB map. `image` is an (res, res, 3)
    array or `filename` an EXR/PFM; "scale" / SpectrumToPhotometric(illuminant) and the
    optional "illuminance" normalisation as Create computes them. The per-pixel
    RGBIlluminantSpectrum conversion needs the colour space's `rgb_table`
    (rgbspectrum.RGBToSpectrumTable; sRGB by default with the D65 illuminant)."""
    type_id = 2

    def __init__(self, image=None, filename=None, scale=1.0, illuminance=None, world_from_light=None,
                 rgb_table=None, illuminant=None):
        if (image is None) == (filename is None):
            raise ValueError("give exactly one of image / filename")
        if filename is not None:
            from . import imageio
            image = imageio.read_rgb(filename)
        img = np.ascontiguousarray(np.asarray(image, np.float32)[:, :, :3])
        if img.ndim != 3 or img.shape[0] != img.shape[1]:
            raise ValueError("image resolution is non-square: not an equal-area environment map")
        if not np.all(np.isfinite(img)):
            raise ValueError("image has infinite or NaN pixel values and so is not suitable as a light")
        if rgb_table is None:
            raise ValueError("ImageInfiniteLight needs rgb_table (rgbspectrum.RGBToSpectrumTable)")
        self.res = img.shape[0]
        self.image = img
        self.illuminant = (spectra.TABLES["D65"] if illuminant is None else spectra.as_table(illuminant, 0.0)
                           ).astype(np.float32)
        sc = np.float32(np.float32(scale) / spectra.spectrum_to_photometric(self.illuminant))
        if illuminance is not None and illuminance > 0:
            sc = np.float32(sc * np.float32(np.float32(illuminance) / self._illuminance(img)))
        self.scale = sc
        self.L = np.zeros(spectra.N, np.float32)
        self.world_from_light = np.eye(4) if world_from_light is None else np.asarray(world_from_light, np.float64)
        # ImageLe: RGBIlluminantSpectrum(cs, ClampZero(rgb)) per pixel (lights.h:620-627)
        self.coeffs = np.ascontiguousarray(rgb_table.spectrum_coeffs(np.maximum(img, np.float32(0))))
        # Image::GetSamplingDistribution (util/image.h:451-470): ImageChannelValues::Average
        # (float sum in channel order / 3) times dxdA = 1
        avg = ((np.float32(0) + img[:, :, 0]) + img[:, :, 1]) + img[:, :, 2]
        self.distribution = np.ascontiguousarray((avg / np.float32(3)).astype(np.float32))

    @staticmethod
    def _cos_theta(res):
        """cos(theta) = z of EqualAreaSquareToSphere at the pixel centres of a res x res map, float32
        (util/math.cpp: z = copysign(1 - r^2, 1 - (|u| + |v|)))."""
        f32 = np.float32
        c = ((np.arange(res, dtype=np.float32) + f32(0.5)) / f32(res)).astype(np.float32)
        uu, vv = np.meshgrid(f32(2) * c - f32(1), f32(2) * c - f32(1))
        sd = f32(1) - (np.abs(uu) + np.abs(vv))
        r = f32(1) - np.abs(sd)
        return np.copysign(f32(1) - r * r, sd).astype(np.float32)

    @classmethod
    def _illuminance(cls, img):
        """Upper-hemisphere illuminance of the map (lights.cpp:1621-1641) with the colour space's
        LuminanceVector (row Y of XYZFromRGB), in the reference's float order: per pixel (rows y,
        then x) of the upper hemisphere and per channel, illuminance += value * lum * cos(theta),
        then * 2 Pi / res^2."""
        f32 = np.float32
        res = img.shape[0]
        lum = np.linalg.inv(spectra.TABLES["srgb_rgb_from_xyz"].astype(np.float64))[1].astype(np.float32)
        z = cls._cos_theta(res)
        up = z > 0
        terms = ((img[up] * lum).astype(np.float32) * z[up][:, None]).astype(np.float32).reshape(-1)
        total = np.cumsum(terms, dtype=np.float32)[-1] if terms.size else f32(0)   # sequential float sum
        return f32(total * f32(f32(f32(2) * f32(math.pi)) / f32(res * res)))

    def render_direction(self, render_from_world):
        return np.zeros(3, np.float32)


class PointLight:
    """PointLight::Create (lights.cpp:192-213): "scale" / SpectrumToPhotometric(I), times
    power / (4 Pi) for power > 0; renderFromLight = world_from_light * Translate(from). I defaults
    to the colour space illuminant. A delta-position light: Li = scale * I / r^2."""
    type_id = 3
    cos_falloff_start, cos_falloff_end = np.float32(1.0), np.float32(-1.0)   # the whole sphere (not read)

    def __init__(self, from_=(0.0, 0.0, 0.0), I=None, scale=1.0, power=None, world_from_light=None):   # noqa: E741
        f32 = np.float32
        self.L = spectra.TABLES["D65"].copy() if I is None else spectra.as_table(I, 1.0)
        sc = f32(f32(scale) / spectra.spectrum_to_photometric(self.L))
        if power is not None and power > 0:
            k_e = f32(f32(4) * f32(math.pi))
            sc = f32(sc * f32(f32(power) / k_e))
        self.scale = sc
        base = np.eye(4) if world_from_light is None else np.asarray(world_from_light, np.float64)
        self.world_from_light = base @ xf.translate(np.asarray(from_, np.float32).astype(np.float64))

    def render_direction(self, render_from_world):
        return np.zeros(3, np.float32)


def _frame_from_z(z):
    """Frame::FromZ (util/vecmath.h:1868-1872) through CoordinateSystem (util/vecmath.h:1007-1013),
    float32: the rows x, y, z of the frame's matrix."""
    f32 = np.float32
    z = np.asarray(z, f32)
    sign = f32(np.copysign(f32(1), z[2]))
    a = f32(f32(-1) / f32(sign + z[2]))
    b = f32(f32(z[0] * z[1]) * a)
    x = np.array([f32(f32(1) + f32(f32(sign * f32(z[0] * z[0])) * a)), f32(sign * b), f32(f32(-sign) * z[0])], f32)
    y = np.array([b, f32(sign + f32(f32(z[1] * z[1]) * a)), f32(-z[1])], f32)
    return np.stack([x, y, z]).astype(f32)


class SpotLight:
    """SpotLight::Create (lights.cpp:1433-1464): renderFromLight = world_from_light * Translate(from) *
    Inverse(Frame::FromZ(Normalize(to - from))); "scale" / SpectrumToPhotometric(I), times
    power / (2 Pi ((1 - cosStart) + (cosStart - cosEnd) / 2)) for power > 0; cosFalloffEnd =
    cos(Radians(coneangle)), cosFalloffStart = cos(Radians(coneangle - conedeltaangle)), in float.
    Li = SmoothStep(cos theta, cosFalloffEnd, cosFalloffStart) * scale * I / r^2."""
    type_id = 4

    def __init__(self, from_=(0.0, 0.0, 0.0), to=(0.0, 0.0, 1.0), I=None, scale=1.0, power=None, coneangle=30.0,   # noqa: E741
                 conedeltaangle=5.0, world_from_light=None):
        f32 = np.float32
        total, start = f32(coneangle), f32(f32(coneangle) - f32(conedeltaangle))
        if start > total:
            raise ValueError("SpotLight: falloffStart > totalWidth (a negative conedeltaangle)")
        self.L = spectra.TABLES["D65"].copy() if I is None else spectra.as_table(I, 1.0)
        rad = lambda deg: f32(f32(f32(math.pi) / f32(180)) * deg)   # noqa: E731
        self.cos_falloff_end = f32(np.cos(rad(total)))
        self.cos_falloff_start = f32(np.cos(rad(start)))
        sc = f32(f32(scale) / spectra.spectrum_to_photometric(self.L))
        if power is not None and power > 0:
            cs, ce = self.cos_falloff_start, self.cos_falloff_end
            k_e = f32(f32(f32(2) * f32(math.pi)) * f32(f32(f32(1) - cs) + f32(f32(cs - ce) / f32(2))))
            sc = f32(sc * f32(f32(power) / k_e))
        self.scale = sc
        frm, to = np.asarray(from_, f32), np.asarray(to, f32)
        d = (to - frm).astype(f32)
        ln = f32(np.sqrt(f32(f32(f32(d[0] * d[0]) + f32(d[1] * d[1])) + f32(d[2] * d[2]))))
        dir_to_z = np.eye(4)
        dir_to_z[:3, :3] = _frame_from_z((d / ln).astype(f32)).astype(np.float64)
        base = np.eye(4) if world_from_light is None else np.asarray(world_from_light, np.float64)
        self.world_from_light = base @ xf.translate(frm.astype(np.float64)) @ np.linalg.inv(dir_to_z)

    def render_direction(self, render_from_world):
        return np.zeros(3, np.float32)


class _ProjectiveCamera:
    type_id = -1

    def __init__(self, pos=(0, 0, 0), look=(0, 0, 1), up=(0, 1, 0), screenwindow=None, frameaspectratio=None,
                 camera_from_world=None, lensradius=0.0, focaldistance=1e6):
        """lensradius, focaldistance: the thin lens of ProjectiveCamera (cameras.cpp:292-303,
        413-424; Create's defaults, cameras.cpp:368, 494); radius 0 is the pinhole."""
        self.camera_from_world = (xf.look_at(pos, look, up) if camera_from_world is None
                                  else np.asarray(camera_from_world, np.float64))
        self.screenwindow = screenwindow
        self.frameaspectratio = frameaspectratio
        self.lensradius = float(lensradius)
        self.focaldistance = float(focaldistance)
        if not (math.isfinite(self.lensradius) and self.lensradius >= 0):
            raise ValueError("lensradius must be finite and >= 0")
        if not self.focaldistance > 0:
            raise ValueError("focaldistance must be > 0")

    def _screen(self, xres, yres):
        frame = self.frameaspectratio if self.frameaspectratio is not None else xres / yres
        if frame > 1:
            s = [-frame, frame, -1.0, 1.0]
        else:
            s = [-1.0, 1.0, -1.0 / frame, 1.0 / frame]
        if self.screenwindow is not None:
            s = list(self.screenwindow)
        return s

    def camera_from_raster(self, xres, yres):
        """ProjectiveCamera ctor (cameras.h:254-273)."""
        x0, x1, y0, y1 = self._screen(xres, yres)
        ndc_from_screen = xf.scale(1 / (x1 - x0), 1 / (y1 - y0), 1) @ xf.translate([-x0, -y1, 0])
        raster_from_ndc = xf.scale(xres, -yres, 1)
        screen_from_raster = np.linalg.inv(raster_from_ndc @ ndc_from_screen)
        return np.linalg.inv(self.screen_from_camera()) @ screen_from_raster

    def world_from_camera(self):
        return np.linalg.inv(self.camera_from_world)


class OrthographicCamera(_ProjectiveCamera):
    """OrthographicCamera (cameras.h:280-300): screenFromCamera = Orthographic(0, 1)."""
    type_id = 0

    def screen_from_camera(self):
        return xf.orthographic(0.0, 1.0)


class PerspectiveCamera(_ProjectiveCamera):
    """PerspectiveCamera (cameras.h:340-350): screenFromCamera = Perspective(fov, 1e-2, 1000)."""
    type_id = 1

    def __init__(self, fov=90.0, **kw):
        super().__init__(**kw)
        self.fov = float(fov)

    def screen_from_camera(self):
        return xf.perspective(self.fov, 1e-2, 1000.0)


class SphericalCamera(_ProjectiveCamera):
    """SphericalCamera (cameras.h:380-410, cameras.cpp:610-687): the whole sphere of directions
    over the film's full resolution, mapping "equalarea" (the octahedral square of
    ImageInfiniteLight) or "equirectangular". Like pbrt's Create it accepts lensradius,
    focaldistance, screenwindow and frameaspectratio and ignores them."""
    type_id = 2
    MAPPINGS = {"equalarea": 0, "equirectangular": 1}

    def __init__(self, mapping="equalarea", **kw):
        if mapping not in self.MAPPINGS:
            raise ValueError(f'unknown mapping for spherical camera {mapping!r} (must be "equalarea" or "equirectangular")')
        kw.pop("lensradius", None)       # (void)lensradius; (void)focaldistance; cameras.cpp:671-672
        kw.pop("focaldistance", None)
        super().__init__(**kw)
        self.mapping = mapping
        self.mapping_id = self.MAPPINGS[mapping]
        self.lensradius, self.focaldistance = 0.0, 1e6

    def camera_from_raster(self, xres, yres):
        """Unused by the spherical camera (pFilm / FullResolution maps to the sphere directly)."""
        return np.eye(4)


class BoxFilter:
    """BoxFilter (filters.h:48-77; Create filters.cpp: radius default 0.5)."""
    type_id = 0

    def __init__(self, radius=(0.5, 0.5)):
        self.radius = np.asarray(radius, np.float32)
        self.sigma = np.float32(0)


class GaussianFilter:
    """GaussianFilter (filters.h:80-118; Create filters.cpp: radius 1.5, sigma 0.5) — pbrt's
    default filter (scene.cpp:94). Sampled through FilterSampler's tabulated distribution;
    samples carry weight f/pdf."""
    type_id = 1

    def __init__(self, radius=(1.5, 1.5), sigma=0.5):
        self.radius = np.asarray(radius, np.float32)
        self.sigma = np.float32(sigma)
        if not (self.radius > 0).all() or int(32 * self.radius[0]) < 1 or int(32 * self.radius[1]) < 1:
            raise ValueError("gaussian filter radius too small")
        if int(32 * self.radius[0]) > 128 or int(32 * self.radius[1]) > 128:
            raise ValueError("gaussian filter radius above 4 is not supported")


class IndependentSampler:
    """IndependentSampler (samplers.h:442-476): PCG32 stream per (pixel, sampleIndex)."""
    type_id = 0

    def __init__(self, pixelsamples=16, seed=None):
        self.pixelsamples = int(pixelsamples)
        self.seed = seed


class ZSobolSampler:
    """ZSobolSampler (samplers.h:225-330) with FastOwen randomisation — pbrt's default
    sampler (scene.cpp:93). pixelsamples should be a power of two (Warning otherwise)."""
    type_id = 1

    def __init__(self, pixelsamples=16, seed=None, randomization="fastowen"):
        if randomization != "fastowen":
            raise NotImplementedError("only the default FastOwen randomisation is implemented")
        self.pixelsamples = int(pixelsamples)
        self.seed = seed


def crop_to_bounds(xres, yres, crop):
    """FilmBaseParameters' crop window -> pixel bounds (film.cpp:134-137, 162-165):
    ceil(float32(res) * float32(c)) per edge, the product rounded to float32 as pbrt's Float
    arithmetic does (1280 x 0.1 is 128 there; the f64 product is just above 128 and would give
    129). crop = (x0, x1, y0, y1) within [0, 1]. Returns (x0, y0, x1, y1)."""
    f = lambda res, c: int(math.ceil(np.float32(np.float32(res) * np.float32(c))))
    return (f(xres, crop[0]), f(yres, crop[2]), f(xres, crop[1]), f(yres, crop[3]))


def _intersect_bounds(b, xres, yres, what):
    """Intersect(newBounds, image) with pbrt's warning when it clamps (film.cpp:101-104, 115-118)."""
    x0, x1, y0, y1 = (int(v) for v in b)
    c = (max(x0, 0), max(y0, 0), min(x1, xres), min(y1, yres))
    if c != (x0, y0, x1, y1):
        warnings.warn(f"Supplied {what} extend beyond image resolution. Clamping.", stacklevel=4)
    return c


def resolve_pixel_bounds(xres, yres, cropwindow=None, pixelbounds=None, cropwindow_override=None,
                         pixelbounds_override=None):
    """Film::pixelBounds from its four sources, FilmBaseParameters' constructor (film.cpp:97-172):
    the film's "pixelbounds" (x0 x1 y0 y1, intersected with the image, a warning when clamped)
    and "cropwindow" (x0 x1 y0 y1 fractions, each pair sorted and clamped to [0, 1]) and the
    command line's --pixelbounds and --cropwindow (the *_override arguments, same orders). The
    film's cropwindow wins over the film's pixelbounds, a pixel-bounds override over the film's
    cropwindow, a crop-window override over everything. Returns (x0, y0, x1, y1); empty bounds
    raise (ErrorExit "Degenerate pixel bounds", film.cpp:171)."""
    xres, yres = int(xres), int(yres)
    for name, v in (("pixelbounds", pixelbounds), ("cropwindow", cropwindow), ("pixelbounds", pixelbounds_override),
                    ("cropwindow", cropwindow_override)):
        if v is not None and len(v) != 4:
            raise ValueError(f'{len(v)} values supplied for "{name}". Expected 4.')
    b = (0, 0, xres, yres)
    if pixelbounds_override is not None:
        b = _intersect_bounds(pixelbounds_override, xres, yres, "pixel bounds")
        if pixelbounds is not None:
            warnings.warn("Both pixel bounds on the command line and in the film were specified. Using the command line's.",
                          stacklevel=3)
    elif pixelbounds is not None:
        b = _intersect_bounds(pixelbounds, xres, yres, "pixel bounds")
    if cropwindow_override is not None:
        c = [float(v) for v in cropwindow_override]
        k = [min(max(v, 0.0), 1.0) for v in c]
        if k != c:
            warnings.warn(f'Film crop window {c} is not in [0,1] range; did you mean to use "pixelbounds"? '
                          "Clamping to valid range.", stacklevel=3)
        b = crop_to_bounds(xres, yres, k)
        if cropwindow is not None:
            warnings.warn("Crop window supplied on command line will override crop window specified with Film.",
                          stacklevel=3)
        if pixelbounds_override is not None or pixelbounds is not None:
            warnings.warn("Both pixel bounds and crop window were specified. Using the crop window.", stacklevel=3)
    elif cropwindow is not None:
        if pixelbounds_override is not None:
            warnings.warn('Ignoring "cropwindow" since pixel bounds were specified on the command line.', stacklevel=3)
        else:
            if pixelbounds is not None:
                warnings.warn("Both pixel bounds and crop window were specified. Using the crop window.", stacklevel=3)
            c = [np.float32(v) for v in cropwindow]
            k = np.clip([min(c[0], c[1]), max(c[0], c[1]), min(c[2], c[3]), max(c[2], c[3])], np.float32(0),
                        np.float32(1))
            b = crop_to_bounds(xres, yres, k)
    if b[0] >= b[2] or b[1] >= b[3]:
        raise ValueError(f"Degenerate pixel bounds provided to film: [ {b[0]}, {b[1]} ] - [ {b[2]}, {b[3]} ].")
    return tuple(int(v) for v in b)


class RGBFilm:
    """RGBFilm (film.h:232-316) with the cie1931 PixelSensor (film.cpp:212-250) and a box
    (default here) or Gaussian pixel filter.

    width and height are the full resolution (the sampler's and the camera's domain);
    pixel_bounds = (x0, y0, x1, y1), from "cropwindow" / "pixelbounds" (resolve_pixel_bounds), are
    the pixels rendered and stored: sums, images and per-sample records are crop_height x
    crop_width, row-major within the bounds."""

    def __init__(self, xresolution=1280, yresolution=720, filter_radius=(0.5, 0.5), iso=100.0, exposure_time=1.0,
                 maxcomponentvalue=math.inf, filter=None, cropwindow=None, pixelbounds=None):
        self.width = int(xresolution)
        self.height = int(yresolution)
        self.cropwindow = None if cropwindow is None else tuple(float(v) for v in cropwindow)
        self.pixelbounds = None if pixelbounds is None else tuple(int(v) for v in pixelbounds)
        self.pixel_bounds = resolve_pixel_bounds(self.width, self.height, self.cropwindow, self.pixelbounds)
        self.filter = filter if filter is not None else BoxFilter(filter_radius)
        self.filter_radius = self.filter.radius
        self.imaging_ratio = np.float32(np.float32(exposure_time) * np.float32(iso) / np.float32(100))
        self.max_component_value = np.float32(maxcomponentvalue)
        self.sensor = spectra.sensor_cie1931()
        # outputRGBFromSensorRGB = colorSpace->RGBFromXYZ * XYZFromSensorRGB (film.cpp:496), cie1931: I
        self.output_from_sensor = spectra.TABLES["srgb_rgb_from_xyz"].astype(np.float32)

    @property
    def crop_width(self):
        return self.pixel_bounds[2] - self.pixel_bounds[0]

    @property
    def crop_height(self):
        return self.pixel_bounds[3] - self.pixel_bounds[1]

    @property
    def npix(self):
        """Pixels of the bounds: what the film stores."""
        return self.crop_width * self.crop_height

    def apply_overrides(self, pixelbounds_override=None, cropwindow_override=None):
        """pbrt's --pixelbounds / --cropwindow: pixel_bounds resolved again from the film's own
        parameters and the overrides (None, None returns to the film's own). Returns the bounds."""
        self.pixel_bounds = resolve_pixel_bounds(self.width, self.height, self.cropwindow, self.pixelbounds,
                                                 cropwindow_override, pixelbounds_override)
        return self.pixel_bounds

    def crop_slice(self):
        """The bounds as an index into a (height, width, ...) array of the whole film."""
        x0, y0, x1, y1 = self.pixel_bounds
        return (slice(y0, y1), slice(x0, x1))


class SpectralFilm(RGBFilm):
    """SpectralFilm (film.h:401-530, film.cpp:849-1066): the RGB sums of RGBFilm plus
    `nbuckets` (default 16) per-pixel spectral buckets over [lambdamin, lambdamax] (default
    360-830 nm); wavelengths sampled uniformly (SampledWavelengths::SampleUniform). Here the
    range must lie within 360-830 nm (the densely sampled tables' domain)."""
    nbuckets_default = 16

    def __init__(self, xresolution=1280, yresolution=720, nbuckets=16, lambdamin=360.0, lambdamax=830.0, **kw):
        super().__init__(xresolution, yresolution, **kw)
        if int(nbuckets) < 1:
            raise ValueError("nbuckets must be positive")
        if not (360.0 <= float(lambdamin) < float(lambdamax) <= 830.0):
            raise ValueError("SpectralFilm wavelength range must lie within 360..830 nm")
        self.nbuckets = int(nbuckets)
        self.lambdamin = np.float32(lambdamin)
        self.lambdamax = np.float32(lambdamax)

    def bucket_centers(self):
        """Channel wavelengths of GetImage: Lerp((i + 0.5) / nBuckets, min, max) (film.cpp:969)."""
        t = ((np.arange(self.nbuckets, dtype=np.float32) + np.float32(0.5)) / np.float32(self.nbuckets)).astype(
            np.float32)
        return ((np.float32(1) - t) * self.lambdamin + t * self.lambdamax).astype(np.float32)

    def channel_names(self):
        """R, G, B, then S0.<lambda>nm with ',' for '.' (film.cpp:963-973)."""
        return ["R", "G", "B"] + ["S0." + ("%.3fnm" % float(l)).replace(".", ",") for l in self.bucket_centers()]


class GBufferFilm(RGBFilm):
    """GBufferFilm (film.h:319-400, film.cpp:588-800). Its geometric channels (albedo, P,
    dzdx/dzdy, N, Ns, uv) and the RGB variance estimators are fed only by a VisibleSurface,
    which VolPathIntegrator::Li sets at the first intersection whose material has a BSDF
    (cpu/integrators.cpp:1124-1151); the medium boundaries this path renders are interface
    shapes (no BSDF), so those channels stay at their zero initial values and the radiance
    part is RGBFilm's (same AddSample sums: the device film is shared)."""
    CHANNELS = ["R", "G", "B", "Albedo.R", "Albedo.G", "Albedo.B", "P.X", "P.Y", "P.Z", "dzdx", "dzdy", "N.X",
                "N.Y", "N.Z", "Ns.X", "Ns.Y", "Ns.Z", "u", "v", "Variance.R", "Variance.G", "Variance.B",
                "RelativeVariance.R", "RelativeVariance.G", "RelativeVariance.B"]

    def channel_names(self):
        return list(self.CHANNELS)


def _crop_shape(film):
    """(rows, columns) of what a film stores: its pixel bounds (a film object without them: all of it)."""
    return getattr(film, "crop_height", film.height), getattr(film, "crop_width", film.width)


def clamp_fp16(rgb):
    """The fp16 clamp of RGBFilm::GetImage and GBufferFilm::GetImage (film.cpp:543-551, 761-769):
    channels above 65504 become 65504 where std::max({r, g, b}) > 65504. The initializer-list
    maximum is `largest = r; if (largest < g) largest = g; if (largest < b) largest = b`: a NaN r
    stays the maximum and keeps the gate shut (a channel above 65504 beside it is left, and
    becomes inf in the half image), a NaN g or b is skipped."""
    m = rgb[..., 0]
    for c in (1, 2):
        m = np.where(m < rgb[..., c], rgb[..., c], m)
    return np.where((m > 65504)[..., None] & (rgb > 65504), np.float32(65504), rgb)


def gbuffer_image(film, rgb_sum, w_sum, fp16=True):
    """GBufferFilm::GetImage (film.cpp:688-800), no splats and no visible surfaces:
    (H, W, 25) float32 (of the pixel bounds) in GBufferFilm.CHANNELS order."""
    rgb = film_rgb(film, rgb_sum, w_sum)
    if fp16:
        rgb = clamp_fp16(rgb)
    out = np.zeros((*_crop_shape(film), len(GBufferFilm.CHANNELS)), np.float32)
    out[:, :, :3] = rgb
    return out


def spectral_image(film, rgb_sum, w_sum, bucket_sums, weight_sums, fp16=True):
    """SpectralFilm::GetImage (film.cpp:961-1028), no splats: (H, W, 3 + nbuckets) float32."""
    rgb = film_rgb(film, rgb_sum, w_sum)
    if fp16:
        rgb = np.minimum(rgb, np.float32(65504))
    bs = np.asarray(bucket_sums, np.float64).reshape(*_crop_shape(film), film.nbuckets)
    bw = np.asarray(weight_sums, np.float64).reshape(*_crop_shape(film), film.nbuckets)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = np.where(bw > 0, (bs / np.where(bw > 0, bw, 1)).astype(np.float32), np.float32(0))
    if fp16:
        c = np.minimum(c, np.float32(65504))
    return np.concatenate([rgb, c.astype(np.float32)], axis=2)


def convex_mesh_planes(vertices, triangles):
    """Outward face planes {nx, ny, nz, h} (inside: n.p <= h) of a closed convex triangle mesh,
    coplanar faces merged; f64."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    c = v.mean(axis=0)
    out = []
    for a, b, d in t:
        n = np.cross(v[b] - v[a], v[d] - v[a])
        ln = np.linalg.norm(n)
        if ln == 0:
            continue
        n = n / ln
        h = float(n @ v[a])
        if n @ c > h:
            n, h = -n, -h
        if not any(np.allclose(n, q[:3], atol=1e-9) and abs(h - q[3]) < 1e-9 for q in out):
            out.append(np.array([*n, h]))
    if len(out) < 4:
        raise ValueError("interface mesh must be a closed convex polyhedron")
    planes = np.array(out)
    if np.any(v @ planes[:, :3].T > planes[:, 3] + 1e-6 * (1 + np.abs(planes[:, 3]))):
        raise ValueError("interface mesh is not convex")
    return planes


def _bounding_sphere_radius(pmin, pmax):
    """Bounds3::BoundingSphere (vecmath.h:1335-1338) in float32."""
    pmin = pmin.astype(np.float32)
    pmax = pmax.astype(np.float32)
    center = ((pmin + pmax) / np.float32(2)).astype(np.float32)
    inside = bool(np.all(center >= pmin) and np.all(center <= pmax))
    if not inside:
        return np.float32(0)
    d = (pmax - center).astype(np.float32)
    return np.float32(np.sqrt(np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])))


class Scene:
    """Resolved render-space scene (CameraWorld rendering space, cameras.cpp:35-41)."""

    def __init__(self, camera, film, medium, lights, sampler=None, interface_sphere=None, interface_mesh=None):
        """interface_sphere: None (the medium's bounds box is its interface shape) or
        (world-space centre, radius) of a sphere without material whose MediumInterface holds
        the medium inside (pbrt's `AttributeBegin MediumInterface "cloud" "" Shape "sphere"`).
        interface_mesh: (vertices, triangles) of a closed CONVEX triangle mesh in world space
        (e.g. pbrt's `Shape "trianglemesh"` cube around a medium) bounding the medium instead."""
        self.camera, self.film, self.medium, self.lights = camera, film, medium, list(lights)
        self.interface_sphere = interface_sphere
        self.sampler = sampler if sampler is not None else IndependentSampler()
        if len(self.lights) > 8:
            raise ValueError("at most 8 lights")
        wfc = camera.world_from_camera()
        cam_pos = wfc @ np.array([0, 0, 0, 1.0])
        self.render_from_world = xf.translate(-cam_pos[:3])
        self.render_from_camera = xf.f32(self.render_from_world @ wfc)
        self.camera_from_raster = xf.f32(camera.camera_from_raster(film.width, film.height))
        rfm = self.render_from_world @ medium.world_from_medium
        self.render_from_medium = xf.f32(rfm)
        self.medium_from_render = xf.f32(np.linalg.inv(rfm))
        # scene bounds = render-space bounds of the interface box (the only shape)
        c = np.array([[x, y, z, 1.0] for x in (medium.p0[0], medium.p1[0]) for y in (medium.p0[1], medium.p1[1])
                      for z in (medium.p0[2], medium.p1[2])])
        rc = (rfm @ c.T).T[:, :3]
        self.scene_radius = _bounding_sphere_radius(rc.min(axis=0), rc.max(axis=0))
        self.interface_sphere_render = None
        self.interface_planes_render = None
        self.interface_vertices_render = None   # the mesh's vertices, float32 (its bounds: graph.MediumData)
        if interface_mesh is not None:
            verts, tris = interface_mesh
            pw = convex_mesh_planes(verts, tris)
            off = np.asarray(self.render_from_world, np.float64)[:3, 3]   # CameraWorld: a translation
            pr = pw.copy()
            pr[:, 3] = pw[:, 3] + pw[:, :3] @ off
            self.interface_planes_render = pr.astype(np.float32)
            vr = np.asarray(verts, np.float64).reshape(-1, 3) + off
            self.interface_vertices_render = vr.astype(np.float32)
            self.scene_radius = _bounding_sphere_radius(vr.min(axis=0), vr.max(axis=0))
        if interface_sphere is not None:
            cw, r = interface_sphere
            if not float(r) > 0:
                raise ValueError("interface sphere radius must be > 0")
            cr = (self.render_from_world @ np.array([*map(float, cw), 1.0]))[:3].astype(np.float32)
            self.interface_sphere_render = np.array([*cr, np.float32(r)], np.float32)
            # the sphere is then the scene's only shape: Sphere::Bounds (shapes.cpp) -> sceneRadius
            lo = cr.astype(np.float64) - float(r)
            hi = cr.astype(np.float64) + float(r)
            self.scene_radius = _bounding_sphere_radius(lo, hi)
        self.light_types = np.array([l.type_id for l in self.lights], np.int32)
        self.light_w = np.stack([l.render_direction(self.render_from_world) for l in self.lights]).astype(
            np.float32) if self.lights else np.zeros((0, 3), np.float32)
        self.light_L = np.stack([l.L for l in self.lights]).astype(np.float32) if self.lights else np.zeros(
            (0, spectra.N), np.float32)
        self.light_scale = np.array([l.scale for l in self.lights], np.float32)
        # image lights: renderFromLight and its inverse (ImageInfiniteLight's transform)
        # (and the local lights: PointLight / SpotLight's renderFromLight and its inverse)
        self.light_rfl = [xf.f32(self.render_from_world @ l.world_from_light) if l.type_id >= 2 else None
                          for l in self.lights]
        self.light_lfr = [xf.f32(np.linalg.inv(self.render_from_world @ l.world_from_light)) if l.type_id >= 2
                          else None for l in self.lights]


def film_rgb(film, rgb_sum, w_sum):
    """RGBFilm::GetPixelRGB (film.h:258-274) in float32, no splats: returns (H, W, 3) of the
    film's pixel bounds."""
    rgb = np.asarray(rgb_sum, np.float64).reshape(-1, 3).astype(np.float32)
    w = np.asarray(w_sum, np.float64).reshape(-1).astype(np.float32)
    nz = w != 0
    rgb[nz] = (rgb[nz] / w[nz, None]).astype(np.float32)
    m = film.output_from_sensor.astype(np.float32)
    out = np.empty_like(rgb)
    for r in range(3):
        out[:, r] = ((m[r, 0] * rgb[:, 0] + m[r, 1] * rgb[:, 1]).astype(np.float32) + m[r, 2] * rgb[:, 2]).astype(
            np.float32)
    return out.reshape(*_crop_shape(film), 3)
