// Camera models beyond the pinholes, shared by the device kernels and the host-compiled tests:
// the thin lens of the projective cameras (cameras.cpp:292-303, 413-424) with
// SampleUniformDiskConcentric (util/sampling.h:325-341), and SphericalCamera's directions
// (cameras.cpp:610-630) with WrapEqualAreaSquare (util/math.cpp:363-379). Standalone (no HIP
// headers); pbrt's float operation order; sin/cos follow the canonical convention of avr_canon.h.
#pragma once

#include "avr_canon.h"
#include "avr_envmap.h"

namespace avr {
namespace cam {

// DevCamera::type
constexpr int kOrthographic = 0, kPerspective = 1, kSpherical = 2;
// DevCamera::mapping (SphericalCamera::Mapping)
constexpr int kEqualArea = 0, kEquiRectangular = 1;

// SampleUniformDiskConcentric (util/sampling.h:325-341)
AVR_HD void concentric_disk(float u0, float u1, float *x, float *y) {
    const float ox = 2 * u0 - 1, oy = 2 * u1 - 1;
    if (ox == 0 && oy == 0) {
        *x = 0;
        *y = 0;
        return;
    }
    float theta, r;
    if (__builtin_fabsf(ox) > __builtin_fabsf(oy)) {
        r = ox;
        theta = 0.78539816339744830961f * (oy / ox);
    } else {
        r = oy;
        theta = 1.57079632679489661923f - 0.78539816339744830961f * (ox / oy);
    }
    float s, c;
    canon::sincos_f(theta, &s, &c);
    *x = r * c;
    *y = r * s;
}

// "Modify ray for depth of field" of Orthographic/PerspectiveCamera::GenerateRay
// (cameras.cpp:292-303, 413-424) on the camera-space pinhole ray (o, d), for lensRadius > 0
AVR_HD void thin_lens(float lensRadius, float focalDistance, float u0, float u1, float o[3], float d[3]) {
    float lx, ly;
    concentric_disk(u0, u1, &lx, &ly);
    lx = lensRadius * lx;
    ly = lensRadius * ly;
    const float ft = focalDistance / d[2];
    const float fx = o[0] + d[0] * ft, fy = o[1] + d[1] * ft, fz = o[2] + d[2] * ft;   // pFocus = ray(ft)
    o[0] = lx;
    o[1] = ly;
    o[2] = 0;
    const float vx = fx - o[0], vy = fy - o[1], vz = fz - o[2];
    const float len = __builtin_sqrtf(vx * vx + vy * vy + vz * vz);
    d[0] = vx / len;
    d[1] = vy / len;
    d[2] = vz / len;
}

// WrapEqualAreaSquare (util/math.cpp:363-379)
AVR_HD void wrap_equal_area_square(float *u, float *v) {
    if (*u < 0) {
        *u = -*u;
        *v = 1 - *v;
    } else if (*u > 1) {
        *u = 2 - *u;
        *v = 1 - *v;
    }
    if (*v < 0) {
        *u = 1 - *u;
        *v = -*v;
    } else if (*v > 1) {
        *u = 1 - *u;
        *v = 2 - *v;
    }
}

// SphericalCamera::GenerateRay's camera-space direction (cameras.cpp:610-630); resx, resy: the
// film's full resolution. The origin is (0, 0, 0) and the ray's weight 1.
AVR_HD void spherical_dir(int mapping, float pFilmX, float pFilmY, int resx, int resy, float d[3]) {
    float u = pFilmX / resx, v = pFilmY / resy;
    float x, y, z;
    if (mapping == kEquiRectangular) {
        const float kPi_ = 3.14159265358979323846f;
        const float theta = kPi_ * v, phi = 2 * kPi_ * u;
        float st, ct, sp, cp;
        canon::sincos_f(theta, &st, &ct);
        canon::sincos_f(phi, &sp, &cp);
        // SphericalDirection (util/vecmath.h:1666-1673)
        st = st < -1 ? -1 : (st > 1 ? 1 : st);
        ct = ct < -1 ? -1 : (ct > 1 ? 1 : ct);
        x = st * cp;
        y = st * sp;
        z = ct;
    } else {
        wrap_equal_area_square(&u, &v);
        env::square_to_sphere(u, v, &x, &y, &z);
    }
    d[0] = x;   // pstd::swap(dir.y, dir.z)
    d[1] = z;
    d[2] = y;
}

}  // namespace cam
}  // namespace avr
