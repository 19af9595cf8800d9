"""Spectral tables and DenselySampledSpectrum helpers (host side).

Mirrors pbrt-v4 `DenselySampledSpectrum` (util/spectrum.h:374-420): a spectrum is a
471-entry float32 table over 360..830 nm, sampled at `lround(lambda) - 360`.
Tables (data/spectra_f32.bin) were dumped from the reference's own spectrum.cpp /
colorspace.cpp by oracle/ref/gen_golden.py: CIE 1931 x̄ȳz̄, the sRGB illuminant (D65)
as RGBColorSpace::illuminant holds it, sRGB RGBFromXYZ and the D65 photometric scale.
"""
import os

import numpy as np

LAMBDA_MIN, LAMBDA_MAX = 360, 830
N = LAMBDA_MAX - LAMBDA_MIN + 1  # 471
CIE_Y_INTEGRAL = np.float32(106.856895)  # util/spectrum.h:38

_DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "spectra_f32.bin")


def _load():
    raw = np.fromfile(_DATA, dtype="<f4")
    expected = 4 * N + 9 + 2
    if raw.size != expected:
        raise RuntimeError(f"{_DATA}: expected {expected} floats, found {raw.size}")
    t = {
        "X": raw[0:N].copy(),
        "Y": raw[N:2 * N].copy(),
        "Z": raw[2 * N:3 * N].copy(),
        "D65": raw[3 * N:4 * N].copy(),
        "srgb_rgb_from_xyz": raw[4 * N:4 * N + 9].reshape(3, 3).copy(),
        "d65_scale": np.float32(raw[4 * N + 9]),
    }
    return t


TABLES = _load()


def constant(c):
    """ConstantSpectrum(c) densely sampled (spectrum.h:354-372)."""
    return np.full(N, np.float32(c), dtype=np.float32)


def as_table(s, default=1.0):
    """Accept None (-> constant `default`), a scalar (ConstantSpectrum) or a 471 table."""
    if s is None:
        return constant(default)
    a = np.asarray(s, dtype=np.float32)
    if a.ndim == 0:
        return constant(float(a))
    if a.shape != (N,):
        raise ValueError(f"spectrum table must have {N} entries (360..830 nm), got {a.shape}")
    return a.copy()


def scaled(table, s):
    """DenselySampledSpectrum::Scale — per-entry float32 multiply (spectrum.h:410-413)."""
    return (np.asarray(table, np.float32) * np.float32(s)).astype(np.float32)


def inner_product_y(table):
    """InnerProduct(&Spectra::Y(), s) with pbrt's float accumulation order (spectrum.cpp)."""
    acc = np.float32(0.0)
    y = TABLES["Y"]
    t = np.asarray(table, np.float32)
    for i in range(N):
        acc = np.float32(acc + np.float32(y[i] * t[i]))
    return acc


def spectrum_to_photometric(table):
    """SpectrumToPhotometric (spectrum.cpp:37-47) for a densely sampled, non-RGB spectrum."""
    return inner_product_y(table)


def _fast_exp(x):
    """FastExp (util/math.h:450-471) on a float32 array: 2^floor(x') times a cubic in the fraction,
    the exponent set in the float's bits. The fused multiply-adds are evaluated in float64 (their
    products are exact there) and rounded once."""
    f32 = np.float32
    xp = (np.asarray(x, np.float32) * f32(1.442695041)).astype(np.float32)
    fxp = np.floor(xp)
    f = (xp - fxp).astype(np.float32)
    fma = lambda a, b, c: (a.astype(np.float64) * np.asarray(b, np.float64) + np.float64(c)).astype(np.float32)
    two_f = fma(f, fma(f, fma(f, f32(0.0781455737), f32(0.226173572)), f32(0.695556856)), f32(1))
    bits = two_f.view(np.uint32)
    exponent = (bits >> np.uint32(23)).astype(np.int64) - 127 + fxp.astype(np.int64)
    out = ((bits & np.uint32(0x807FFFFF)) | (np.clip(exponent + 127, 0, 255).astype(np.uint32) << np.uint32(23))).view(
        np.float32)
    return np.where(exponent < -126, f32(0), np.where(exponent > 127, f32(np.inf), out)).astype(np.float32)


def _blackbody_f32(lambda_nm, T):
    """Blackbody(lambda, T) (util/spectrum.h:69-80) in the reference's float order, FastExp included:
    its emission, and with it SpectrumToPhotometric of a blackbody L, differs from the exact Planck
    law by up to 1e-4."""
    f32 = np.float32
    c, h, kb = f32(299792458.0), f32(6.62606957e-34), f32(1.3806488e-23)
    l = (np.asarray(lambda_nm, np.float32) * f32(1e-9)).astype(np.float32)
    l2 = l * l
    l5 = (l2 * l2) * l
    e = _fast_exp((h * c) / ((l * kb) * f32(T)))
    return (((f32(2) * h) * c) * c) / (l5 * (e - f32(1)))


def blackbody(T):
    """BlackbodySpectrum(T) densely sampled (spectrum.h:500-530): Blackbody(lambda, T) times
    1 / Blackbody(lambdaMax, T), lambdaMax = 2.8977721e-3 / T (Wien), in the reference's floats."""
    if not T > 0:
        return np.zeros(N, np.float32)
    lam = np.arange(LAMBDA_MIN, LAMBDA_MAX + 1, dtype=np.float32)
    lambda_max = np.float32(2.8977721e-3) / np.float32(T)
    norm = np.float32(1) / _blackbody_f32(np.array([lambda_max * np.float32(1e9)], np.float32), T)[0]
    return (_blackbody_f32(lam, T) * norm).astype(np.float32)


def sensor_cie1931():
    """cie1931 PixelSensor response (film.h:220-231): r̄ḡb̄ = X, Y, Z; XYZFromSensorRGB = I."""
    return np.stack([TABLES["X"], TABLES["Y"], TABLES["Z"]]).astype(np.float32)
