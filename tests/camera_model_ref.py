"""pbrt's thin lens and SphericalCamera restated in numpy from the cited lines (not from
csrc/avr_camera.h), evaluated in the dtype of the caller's choice — TEST INFRASTRUCTURE, no device.

  concentric_disk      SampleUniformDiskConcentric, util/sampling.h:325-341
  thin_lens            "Modify ray for depth of field", cameras.cpp:292-303 and 413-424
  wrap_equal_area      WrapEqualAreaSquare, util/math.cpp:363-379 (also returns the branch taken)
  square_to_sphere     EqualAreaSquareToSphere, util/math.cpp:292-315
  spherical_dir        SphericalCamera::GenerateRay, cameras.cpp:610-630

tests/test_camera_models.py evaluates each in float32 and in float64 on the same float32 inputs:
the largest difference between the two is the formulas' own rounding, and four times that is what
the header may differ from the float64 values."""
import numpy as np


def concentric_disk(u, dt):
    u = np.asarray(u, np.float32).astype(dt)
    ox, oy = dt(2) * u[:, 0] - dt(1), dt(2) * u[:, 1] - dt(1)
    first = np.abs(ox) > np.abs(oy)
    pi4, pi2 = dt(np.pi / 4), dt(np.pi / 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, ox, oy)
        theta = np.where(first, pi4 * (oy / ox), pi2 - pi4 * (ox / oy))
    x, y = r * np.cos(theta), r * np.sin(theta)
    zero = (ox == 0) & (oy == 0)
    return np.stack([np.where(zero, dt(0), x), np.where(zero, dt(0), y)], 1).astype(dt)


def thin_lens(radius, focal, u, o, d, dt):
    """(o', d') of the camera-space pinhole rays (o, d) through a lens; radius, focal: (n,)."""
    radius, focal = np.asarray(radius, np.float32).astype(dt), np.asarray(focal, np.float32).astype(dt)
    o, d = np.asarray(o, np.float32).astype(dt), np.asarray(d, np.float32).astype(dt)
    p_lens = radius[:, None] * concentric_disk(u, dt)
    ft = focal / d[:, 2]
    p_focus = o + d * ft[:, None]
    o2 = np.stack([p_lens[:, 0], p_lens[:, 1], np.zeros(len(o), dt)], 1)
    v = p_focus - o2
    d2 = v / np.sqrt((v * v).sum(axis=1))[:, None]
    return o2.astype(dt), d2.astype(dt)


def wrap_equal_area(u, v):
    """(u', v', branches): branches (n, 4) bool — u < 0, u > 1, v < 0, v > 1 as the code takes them."""
    u, v = np.array(u), np.array(v)
    one, two = u.dtype.type(1), u.dtype.type(2)
    b0 = u < 0
    u, v = np.where(b0, -u, u), np.where(b0, one - v, v)
    b1 = ~b0 & (u > 1)
    u, v = np.where(b1, two - u, u), np.where(b1, one - v, v)
    b2 = v < 0
    u, v = np.where(b2, one - u, u), np.where(b2, -v, v)
    b3 = ~b2 & (v > 1)
    u, v = np.where(b3, one - u, u), np.where(b3, two - v, v)
    return u, v, np.stack([b0, b1, b2, b3], 1)


def square_to_sphere(p, q, dt):
    u, v = dt(2) * p - dt(1), dt(2) * q - dt(1)
    up, vp = np.abs(u), np.abs(v)
    sd = dt(1) - (up + vp)
    r = dt(1) - np.abs(sd)
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(r == 0, dt(1), (vp - up) / r + dt(1)) * dt(np.pi) / dt(4)
    z = np.copysign(dt(1) - r * r, sd)
    k = r * np.sqrt(np.maximum(dt(2) - r * r, dt(0)))
    return np.stack([np.copysign(np.cos(phi), u) * k, np.copysign(np.sin(phi), v) * k, z], 1).astype(dt)


def spherical_dir(mapping, p_film, res, dt):
    """Camera-space directions at raster points p_film (n, 2) of a film of full resolution res."""
    pf = np.asarray(p_film, np.float32).astype(dt)
    u, v = pf[:, 0] / dt(res[0]), pf[:, 1] / dt(res[1])
    if mapping == "equirectangular":
        theta, phi = dt(np.pi) * v, dt(2) * dt(np.pi) * u
        st, ct = np.clip(np.sin(theta), -1, 1), np.clip(np.cos(theta), -1, 1)
        d = np.stack([st * np.cos(phi), st * np.sin(phi), ct], 1)
    else:
        u, v, _ = wrap_equal_area(u, v)
        d = square_to_sphere(u, v, dt)
    return d[:, [0, 2, 1]].astype(dt)


def wrap_branches(p_film, res):
    """Which of WrapEqualAreaSquare's four branches each float32 raster point takes."""
    pf = np.asarray(p_film, np.float32)
    return wrap_equal_area(pf[:, 0] / np.float32(res[0]), pf[:, 1] / np.float32(res[1]))[2]
