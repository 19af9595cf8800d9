// Local (delta-position) lights and the half of BVHLightSampler that handles lights with bounds,
// shared by the device kernels, the host (the BVH build) and the host-compiled tests:
// PointLight::SampleLi (lights.h:223-230), SpotLight::SampleLi / I (lights.h:779-791,
// lights.cpp:1360-1363) with SmoothStep (util/math.h:268-274), CompactLightBounds
// (lightsamplers.h:101-228) with OctahedralVector (util/vecmath.h:1734-1783) and
// BoundSubtendedDirections (util/vecmath.h:1816-1829), BVHLightSampler::Sample / PMF
// (lightsamplers.h:266-327) with SampleDiscrete (util/sampling.h:79-113), and on the host the
// lights' Bounds() (lights.cpp:168-173, 1370-1380), Union(LightBounds) (lights.h:137-153) with
// DirectionCone's union (util/vecmath.cpp:56-83), EvaluateCost (lightsamplers.h:383-396) and
// buildBVH (lightsamplers.cpp:109-238). Standalone (no HIP headers); pbrt's float operation
// order. What the device runs uses + - * / and sqrt alone, so device and host agree bit for bit;
// the build's acos / cos / sin / asin are the host's libm, as they are pbrt's.
#pragma once

#include <algorithm>
#include <limits>
#include <utility>
#include <vector>

#include "avr_canon.h"

namespace avr {
namespace ll {

// DevLight::type of the local lights
constexpr int kPoint = 3, kSpot = 4;
constexpr int kMaxTreeLights = 8;
constexpr int kMaxNodes = 2 * kMaxTreeLights - 1;
constexpr float kPi_ = 3.14159265358979323846f;
constexpr float kOneMinusEps = 0x1.fffffep-1f;

// LightBVHNode (32 bytes): CompactLightBounds {OctahedralVector w, phi, qCosTheta_o : 15,
// qCosTheta_e : 15, twoSided : 1, qb[2][3]} and {childOrLightIndex : 31, isLeaf : 1}
struct Node {
    uint16_t wx, wy;
    float phi;
    uint32_t bits;
    uint16_t qb[2][3];
    uint32_t link;
    uint32_t pad_;
    AVR_HD uint32_t q_cos_o() const { return bits & 0x7fffu; }
    AVR_HD uint32_t q_cos_e() const { return (bits >> 15) & 0x7fffu; }
    AVR_HD bool two_sided() const { return (bits >> 30) & 1u; }
    AVR_HD uint32_t index() const { return link & 0x7fffffffu; }
    AVR_HD bool leaf() const { return link >> 31; }
};
static_assert(sizeof(Node) == 32, "LightBVHNode is 32 bytes");

// BVHLightSampler's members for at most kMaxTreeLights lights: allLightBounds, the nodes, and the
// infinite lights as indices into the light list (infiniteLights[j] == list[inf[j]])
struct Tree {
    float allb[6];                    // allLightBounds pMin, pMax
    int nNodes, nInf;
    int inf[kMaxTreeLights];
    Node nodes[kMaxNodes];
};

AVR_HD float sqr(float x) { return x * x; }
AVR_HD float safe_sqrt(float x) { return __builtin_sqrtf(x > 0.f ? x : 0.f); }   // sqrt(max(0, x))
AVR_HD float clampf(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }
AVR_HD float lerp(float x, float a, float b) { return (1 - x) * a + x * b; }
AVR_HD float length3(const float v[3]) { return __builtin_sqrtf(sqr(v[0]) + sqr(v[1]) + sqr(v[2])); }
AVR_HD void normalize3(float v[3]) {
    const float l = length3(v);
    v[0] = v[0] / l;
    v[1] = v[1] / l;
    v[2] = v[2] / l;
}

// SmoothStep (util/math.h:268-274), with its a == b branch
AVR_HD float smooth_step(float x, float a, float b) {
    if (a == b) return x < a ? 0.f : 1.f;
    const float t = clampf((x - a) / (b - a), 0.f, 1.f);
    return t * t * (3 - 2 * t);
}

// renderFromLight(Point3f(0, 0, 0)) (Transform::operator()(Point3), util/transform.h) of a 4x4
AVR_HD void light_position(const float m[16], float p[3]) {
    const float x = 0.f, y = 0.f, z = 0.f;
    float xp = m[0] * x + m[1] * y + m[2] * z + m[3];
    float yp = m[4] * x + m[5] * y + m[6] * z + m[7];
    float zp = m[8] * x + m[9] * y + m[10] * z + m[11];
    const float wp = m[12] * x + m[13] * y + m[14] * z + m[15];
    if (wp != 1) {
        xp = xp / wp;
        yp = yp / wp;
        zp = zp / wp;
    }
    p[0] = xp;
    p[1] = yp;
    p[2] = zp;
}

// PointLight / SpotLight::SampleLi at the reference point p: wi = Normalize(pLight - p), the
// squared distance, and the factor on scale * I(lambda) in front of 1 / DistanceSquared: 1 for the
// point light, SmoothStep(CosTheta(Normalize(lightFromRender(-wi))), cosEnd, cosStart) for the
// spot light (lfr: lightFromRender's 3x3, row-major). Li = falloff * scale * I / dist2; pdf 1.
AVR_HD void sample_li(int type, const float pLight[3], const float lfr[9], float cosStart, float cosEnd,
                      const float p[3], float wi[3], float *dist2, float *falloff) {
    wi[0] = pLight[0] - p[0];
    wi[1] = pLight[1] - p[1];
    wi[2] = pLight[2] - p[2];
    *dist2 = sqr(wi[0]) + sqr(wi[1]) + sqr(wi[2]);   // DistanceSquared(p, ctx.p): the same differences
    normalize3(wi);
    if (type != kSpot) {
        *falloff = 1.f;
        return;
    }
    const float nx = -wi[0], ny = -wi[1], nz = -wi[2];
    float wl[3] = {lfr[0] * nx + lfr[1] * ny + lfr[2] * nz, lfr[3] * nx + lfr[4] * ny + lfr[5] * nz,
                   lfr[6] * nx + lfr[7] * ny + lfr[8] * nz};
    normalize3(wl);
    *falloff = smooth_step(wl[2], cosEnd, cosStart);
}

// One wavelength of Li from sample_li's values: PointLight scale * I / r^2 (lights.h:228),
// SpotLight SmoothStep * scale * I / r^2 (lights.cpp:1361-1362, lights.h:786)
AVR_HD float li_channel(int type, float falloff, float scale, float I, float dist2) {
    return type == kSpot ? falloff * scale * I / dist2 : scale * I / dist2;
}

// OctahedralVector -> Vector3f (util/vecmath.h:1752-1765)
AVR_HD void oct_decode(uint16_t ox, uint16_t oy, float v[3]) {
    v[0] = -1 + 2 * (ox / 65535.f);
    v[1] = -1 + 2 * (oy / 65535.f);
    v[2] = 1 - (__builtin_fabsf(v[0]) + __builtin_fabsf(v[1]));
    if (v[2] < 0) {
        const float xo = v[0];
        v[0] = (1 - __builtin_fabsf(v[1])) * __builtin_copysignf(1.f, xo);
        v[1] = (1 - __builtin_fabsf(xo)) * __builtin_copysignf(1.f, v[1]);
    }
    normalize3(v);
}

AVR_HD float node_cos_o(const Node &n) { return 2 * (n.q_cos_o() / 32767.f) - 1; }
AVR_HD float node_cos_e(const Node &n) { return 2 * (n.q_cos_e() / 32767.f) - 1; }

// CompactLightBounds::Bounds (lightsamplers.h:134-141): b = {pMin, pMax}
AVR_HD void node_bounds(const Node &n, const float allb[6], float b[6]) {
    for (int s = 0; s < 2; ++s)
        for (int c = 0; c < 3; ++c) b[3 * s + c] = lerp(n.qb[s][c] / 65535.f, allb[c], allb[3 + c]);
}

AVR_HD float cos_sub_clamped(float sinTheta_a, float cosTheta_a, float sinTheta_b, float cosTheta_b) {
    if (cosTheta_a > cosTheta_b) return 1;
    return cosTheta_a * cosTheta_b + sinTheta_a * sinTheta_b;
}
AVR_HD float sin_sub_clamped(float sinTheta_a, float cosTheta_a, float sinTheta_b, float cosTheta_b) {
    if (cosTheta_a > cosTheta_b) return 0;
    return sinTheta_a * cosTheta_b - cosTheta_a * sinTheta_b;
}

// The importance of (decoded) light bounds at p for n = (0, 0, 0): CompactLightBounds::Importance
// (lightsamplers.h:144-201) after its Bounds() and cosines
AVR_HD float bounds_importance(const float b[6], const float w[3], float phi, float cosTheta_o, float cosTheta_e,
                               bool twoSided, const float p[3]) {
    const float pc[3] = {(b[0] + b[3]) / 2, (b[1] + b[4]) / 2, (b[2] + b[5]) / 2};
    float wi[3] = {p[0] - pc[0], p[1] - pc[1], p[2] - pc[2]};
    float d2 = sqr(wi[0]) + sqr(wi[1]) + sqr(wi[2]);
    const float diag[3] = {b[3] - b[0], b[4] - b[1], b[5] - b[2]};
    const float hl = length3(diag) / 2;
    d2 = d2 < hl ? hl : d2;   // std::max(d2, Length(Diagonal()) / 2)
    normalize3(wi);
    float cosTheta_w = w[0] * wi[0] + w[1] * wi[1] + w[2] * wi[2];
    if (twoSided) cosTheta_w = __builtin_fabsf(cosTheta_w);
    const float sinTheta_w = safe_sqrt(1 - sqr(cosTheta_w));
    // BoundSubtendedDirections(bounds, p).cosTheta (util/vecmath.h:1816-1829)
    float cosTheta_b;
    {
        const bool inside = pc[0] >= b[0] && pc[0] <= b[3] && pc[1] >= b[1] && pc[1] <= b[4] && pc[2] >= b[2] &&
                            pc[2] <= b[5];
        const float r3[3] = {pc[0] - b[3], pc[1] - b[4], pc[2] - b[5]};
        const float radius = inside ? length3(r3) : 0.f;
        const float dc[3] = {p[0] - pc[0], p[1] - pc[1], p[2] - pc[2]};
        const float dist2 = sqr(dc[0]) + sqr(dc[1]) + sqr(dc[2]);
        if (dist2 < sqr(radius)) {
            cosTheta_b = -1.f;   // EntireSphere
        } else {
            const float cd[3] = {pc[0] - p[0], pc[1] - p[1], pc[2] - p[2]};
            const float sin2ThetaMax = sqr(radius) / (sqr(cd[0]) + sqr(cd[1]) + sqr(cd[2]));
            cosTheta_b = safe_sqrt(1 - sin2ThetaMax);
        }
    }
    const float sinTheta_b = safe_sqrt(1 - sqr(cosTheta_b));
    const float sinTheta_o = safe_sqrt(1 - sqr(cosTheta_o));
    const float cosTheta_x = cos_sub_clamped(sinTheta_w, cosTheta_w, sinTheta_o, cosTheta_o);
    const float sinTheta_x = sin_sub_clamped(sinTheta_w, cosTheta_w, sinTheta_o, cosTheta_o);
    const float cosThetap = cos_sub_clamped(sinTheta_x, cosTheta_x, sinTheta_b, cosTheta_b);
    if (cosThetap <= cosTheta_e) return 0;
    float importance = phi * cosThetap / d2;
    importance = importance < 0.f ? 0.f : importance;   // std::max<Float>(importance, 0): a NaN stays
    return importance;
}

AVR_HD float node_importance(const Node &n, const float allb[6], const float p[3]) {
    float b[6], w[3];
    node_bounds(n, allb, b);
    oct_decode(n.wx, n.wy, w);
    return bounds_importance(b, w, n.phi, node_cos_o(n), node_cos_e(n), n.two_sided(), p);
}

// NextFloatDown of a finite float (util/float.h:181-194)
AVR_HD float next_float_down(float v) {
    if (v == 0.f) v = -0.f;
    uint32_t ui;
    memcpy(&ui, &v, 4);
    if (v > 0) --ui;
    else ++ui;
    memcpy(&v, &ui, 4);
    return v;
}

// SampleDiscrete over two weights (util/sampling.h:79-113): the offset, its PMF and the remapped u
AVR_HD int sample_discrete2(const float w[2], float u, float *pmf, float *uRemapped) {
    float sumWeights = 0;
    sumWeights += w[0];
    sumWeights += w[1];
    float up = u * sumWeights;
    if (up == sumWeights) up = next_float_down(up);
    int offset = 0;
    float sum = 0;
    while (sum + w[offset] <= up) sum += w[offset++];
    *pmf = w[offset] / sumWeights;
    const float r = (up - sum) / w[offset];
    *uRemapped = kOneMinusEps < r ? kOneMinusEps : r;   // std::min(r, OneMinusEpsilon)
    return offset;
}

// BVHLightSampler::Sample(ctx, u) (lightsamplers.h:266-320) for a medium interaction (n = 0): the
// index of the sampled light in the light list, or -1 for "no light"; *pmf its probability
AVR_HD int bvh_sample(const Tree &t, const float p[3], float u, float *pmf) {
    const int nInf = t.nInf;
    const float pInfinite = float(nInf) / float(nInf + (t.nNodes == 0 ? 0 : 1));
    if (u < pInfinite) {
        u /= pInfinite;
        int index = (int)(u * nInf);
        index = index < nInf - 1 ? index : nInf - 1;
        *pmf = pInfinite / nInf;
        return t.inf[index];
    }
    if (t.nNodes == 0) return -1;
    const float uu = (u - pInfinite) / (1 - pInfinite);
    u = kOneMinusEps < uu ? kOneMinusEps : uu;
    int nodeIndex = 0;
    float pm = 1 - pInfinite;
    while (true) {
        const Node &node = t.nodes[nodeIndex];
        if (!node.leaf()) {
            const int second = (int)node.index();
            const float ci[2] = {node_importance(t.nodes[nodeIndex + 1], t.allb, p),
                                 node_importance(t.nodes[second], t.allb, p)};
            if (ci[0] == 0 && ci[1] == 0) return -1;
            float nodePMF;
            const int child = sample_discrete2(ci, u, &nodePMF, &u);
            pm *= nodePMF;
            nodeIndex = child == 0 ? nodeIndex + 1 : second;
        } else {
            if (nodeIndex > 0 || node_importance(node, t.allb, p) > 0) {
                *pmf = pm;
                return (int)node.index();
            }
            return -1;
        }
    }
}

// BVHLightSampler::PMF(ctx, light) of an infinite light (lightsamplers.h:325-326)
AVR_HD float bvh_pmf_infinite(const Tree &t) { return 1.f / (t.nInf + (t.nNodes == 0 ? 0 : 1)); }

// ---------------------------------------------------------------------------------------------
// Host: the lights' bounds and the BVH build

struct LightBounds {
    float b[6] = {std::numeric_limits<float>::max(), std::numeric_limits<float>::max(), std::numeric_limits<float>::max(),
                  std::numeric_limits<float>::lowest(), std::numeric_limits<float>::lowest(),
                  std::numeric_limits<float>::lowest()};
    float phi = 0;
    float w[3] = {0, 0, 0};
    float cosTheta_o = 0, cosTheta_e = 0;
    bool twoSided = false;
};

// PointLight::Bounds / SpotLight::Bounds (lights.cpp:168-173, 1370-1380); rfl: renderFromLight
// (4x4), maxI: I->MaxValue()
inline LightBounds light_bounds(int type, const float rfl[16], float scale, float maxI, float cosStart, float cosEnd) {
    LightBounds lb;
    float p[3];
    light_position(rfl, p);
    for (int c = 0; c < 3; ++c) lb.b[c] = lb.b[3 + c] = p[c];
    if (type == kSpot) {
        float w[3] = {rfl[0] * 0.f + rfl[1] * 0.f + rfl[2] * 1.f, rfl[4] * 0.f + rfl[5] * 0.f + rfl[6] * 1.f,
                      rfl[8] * 0.f + rfl[9] * 0.f + rfl[10] * 1.f};
        normalize3(w);
        lb.phi = scale * maxI * 4 * kPi_;
        float cosTheta_e = std::cos(std::acos(cosEnd) - std::acos(cosStart));
        if (cosTheta_e == 1 && cosEnd != cosStart) cosTheta_e = 0.999f;
        lb.cosTheta_o = cosStart;
        lb.cosTheta_e = cosTheta_e;
        for (int c = 0; c < 3; ++c) lb.w[c] = w[c];
        normalize3(lb.w);   // LightBounds' constructor normalises again
    } else {
        lb.phi = 4 * kPi_ * scale * maxI;
        lb.w[0] = 0.f;
        lb.w[1] = 0.f;
        lb.w[2] = 1.f;
        normalize3(lb.w);
        lb.cosTheta_o = std::cos(kPi_);
        lb.cosTheta_e = std::cos(kPi_ / 2);
    }
    lb.twoSided = false;
    return lb;
}

struct Cone {
    float w[3] = {0, 0, 0};
    float cosTheta = std::numeric_limits<float>::infinity();
};
inline Cone entire_sphere() {
    Cone c;
    c.w[2] = 1.f;
    c.cosTheta = -1.f;
    return c;
}
inline float safe_asin(float x) { return std::asin(clampf(x, -1.f, 1.f)); }
inline float safe_acos(float x) { return std::acos(clampf(x, -1.f, 1.f)); }
// AngleBetween (util/vecmath.h:972-977)
inline float angle_between(const float a[3], const float b[3]) {
    if (a[0] * b[0] + a[1] * b[1] + a[2] * b[2] < 0) {
        const float s[3] = {a[0] + b[0], a[1] + b[1], a[2] + b[2]};
        return kPi_ - 2 * safe_asin(length3(s) / 2);
    }
    const float d[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
    return 2 * safe_asin(length3(d) / 2);
}
// Union(DirectionCone, DirectionCone) (util/vecmath.cpp:56-83) with Rotate(theta, axis)
// (util/transform.h:224-251) applied to a.w
inline Cone cone_union(const Cone &a, const Cone &b) {
    const float inf = std::numeric_limits<float>::infinity();
    if (a.cosTheta == inf) return b;
    if (b.cosTheta == inf) return a;
    const float theta_a = safe_acos(a.cosTheta), theta_b = safe_acos(b.cosTheta);
    const float theta_d = angle_between(a.w, b.w);
    if (std::min(theta_d + theta_b, kPi_) <= theta_a) return a;
    if (std::min(theta_d + theta_a, kPi_) <= theta_b) return b;
    const float theta_o = (theta_a + theta_d + theta_b) / 2;
    if (theta_o >= kPi_) return entire_sphere();
    const float theta_r = theta_o - theta_a;
    float wr[3];
    {   // Cross (util/vecmath.h: DifferenceOfProducts, exact to one rounding through fma)
        auto dop = [](float p, float q, float r, float s) {
            const float rs = r * s;
            const float diff = std::fma(p, q, -rs);
            const float err = std::fma(-r, s, rs);
            return diff + err;
        };
        wr[0] = dop(a.w[1], b.w[2], a.w[2], b.w[1]);
        wr[1] = dop(a.w[2], b.w[0], a.w[0], b.w[2]);
        wr[2] = dop(a.w[0], b.w[1], a.w[1], b.w[0]);
    }
    if (sqr(wr[0]) + sqr(wr[1]) + sqr(wr[2]) == 0) return entire_sphere();
    const float deg = (180 / kPi_) * theta_r;
    const float rad = (kPi_ / 180) * deg;
    const float sinTheta = std::sin(rad), cosTheta = std::cos(rad);
    float ax[3] = {wr[0], wr[1], wr[2]};
    normalize3(ax);
    float m[3][3];
    m[0][0] = ax[0] * ax[0] + (1 - ax[0] * ax[0]) * cosTheta;
    m[0][1] = ax[0] * ax[1] * (1 - cosTheta) - ax[2] * sinTheta;
    m[0][2] = ax[0] * ax[2] * (1 - cosTheta) + ax[1] * sinTheta;
    m[1][0] = ax[0] * ax[1] * (1 - cosTheta) + ax[2] * sinTheta;
    m[1][1] = ax[1] * ax[1] + (1 - ax[1] * ax[1]) * cosTheta;
    m[1][2] = ax[1] * ax[2] * (1 - cosTheta) - ax[0] * sinTheta;
    m[2][0] = ax[0] * ax[2] * (1 - cosTheta) - ax[1] * sinTheta;
    m[2][1] = ax[1] * ax[2] * (1 - cosTheta) + ax[0] * sinTheta;
    m[2][2] = ax[2] * ax[2] + (1 - ax[2] * ax[2]) * cosTheta;
    Cone c;
    for (int r = 0; r < 3; ++r) c.w[r] = m[r][0] * a.w[0] + m[r][1] * a.w[1] + m[r][2] * a.w[2];
    normalize3(c.w);   // DirectionCone's constructor
    c.cosTheta = std::cos(theta_o);
    return c;
}

inline void bounds_union(const float a[6], const float b[6], float out[6]) {
    for (int c = 0; c < 3; ++c) {
        out[c] = std::min(a[c], b[c]);
        out[3 + c] = std::max(a[3 + c], b[3 + c]);
    }
}

// Union(LightBounds, LightBounds) (lights.h:137-153)
inline LightBounds lb_union(const LightBounds &a, const LightBounds &b) {
    if (a.phi == 0) return b;
    if (b.phi == 0) return a;
    Cone ca, cb;
    for (int c = 0; c < 3; ++c) ca.w[c] = a.w[c], cb.w[c] = b.w[c];
    normalize3(ca.w);   // DirectionCone's constructor
    normalize3(cb.w);
    ca.cosTheta = a.cosTheta_o;
    cb.cosTheta = b.cosTheta_o;
    const Cone cone = cone_union(ca, cb);
    LightBounds r;
    bounds_union(a.b, b.b, r.b);
    for (int c = 0; c < 3; ++c) r.w[c] = cone.w[c];
    normalize3(r.w);    // LightBounds' constructor
    r.phi = a.phi + b.phi;
    r.cosTheta_o = cone.cosTheta;
    r.cosTheta_e = std::min(a.cosTheta_e, b.cosTheta_e);
    r.twoSided = a.twoSided | b.twoSided;
    return r;
}

// CompactLightBounds(lb, allb) (lightsamplers.h:108-121, 206-217) into a node
inline void compact(const LightBounds &lb, const float allb[6], Node *n) {
    float v[3] = {lb.w[0], lb.w[1], lb.w[2]};
    normalize3(v);
    {   // OctahedralVector(v) (util/vecmath.h:1739-1749)
        const float s = std::abs(v[0]) + std::abs(v[1]) + std::abs(v[2]);
        v[0] /= s;
        v[1] /= s;
        v[2] /= s;
        auto encode = [](float f) { return (uint16_t)std::round(clampf((f + 1) / 2, 0.f, 1.f) * 65535.f); };
        if (v[2] >= 0) {
            n->wx = encode(v[0]);
            n->wy = encode(v[1]);
        } else {
            n->wx = encode((1 - std::abs(v[1])) * std::copysign(1.f, v[0]));
            n->wy = encode((1 - std::abs(v[0])) * std::copysign(1.f, v[1]));
        }
    }
    n->phi = lb.phi;
    auto qcos = [](float c) { return (uint32_t)std::floor(32767.f * ((c + 1) / 2)) & 0x7fffu; };
    n->bits = qcos(lb.cosTheta_o) | (qcos(lb.cosTheta_e) << 15) | ((lb.twoSided ? 1u : 0u) << 30);
    auto qbound = [](float c, float mn, float mx) {
        if (mn == mx) return 0.f;
        return 65535.f * clampf((c - mn) / (mx - mn), 0.f, 1.f);
    };
    for (int c = 0; c < 3; ++c) {
        n->qb[0][c] = (uint16_t)std::floor(qbound(lb.b[c], allb[c], allb[3 + c]));
        n->qb[1][c] = (uint16_t)std::ceil(qbound(lb.b[3 + c], allb[c], allb[3 + c]));
    }
    n->pad_ = 0;
}

// EvaluateCost (lightsamplers.h:383-396)
inline float evaluate_cost(const LightBounds &b, const float bounds[6], int dim) {
    const float theta_o = std::acos(b.cosTheta_o), theta_e = std::acos(b.cosTheta_e);
    const float theta_w = std::min(theta_o + theta_e, kPi_);
    const float sinTheta_o = safe_sqrt(1 - sqr(b.cosTheta_o));
    const float M_omega = 2 * kPi_ * (1 - b.cosTheta_o) +
                          kPi_ / 2 * (2 * theta_w * sinTheta_o - std::cos(theta_o - 2 * theta_w) -
                                      2 * theta_o * sinTheta_o + b.cosTheta_o);
    const float d[3] = {bounds[3] - bounds[0], bounds[4] - bounds[1], bounds[5] - bounds[2]};
    const float Kr = std::max({d[0], d[1], d[2]}) / d[dim];
    const float e[3] = {b.b[3] - b.b[0], b.b[4] - b.b[1], b.b[5] - b.b[2]};
    const float area = 2 * (e[0] * e[1] + e[0] * e[2] + e[1] * e[2]);
    return b.phi * M_omega * Kr * area;
}

struct Builder {
    Tree *t;
    using Item = std::pair<int, LightBounds>;

    static void centroid(const LightBounds &lb, float c[3]) {
        for (int k = 0; k < 3; ++k) c[k] = (lb.b[k] + lb.b[3 + k]) / 2;
    }
    // Bounds3::Offset(p)[dim] (util/vecmath.h:1323-1332)
    static float offset(const float cb[6], const float p[3], int dim) {
        float o = p[dim] - cb[dim];
        if (cb[3 + dim] > cb[dim]) o /= cb[3 + dim] - cb[dim];
        return o;
    }

    // buildBVH (lightsamplers.cpp:135-238); returns {node index, bounds}
    std::pair<int, LightBounds> build(std::vector<Item> &lights, int start, int end) {
        constexpr float fmax = std::numeric_limits<float>::max(), flow = std::numeric_limits<float>::lowest();
        if (end - start == 1) {
            const int nodeIndex = t->nNodes++;
            Node &n = t->nodes[nodeIndex];
            compact(lights[start].second, t->allb, &n);
            n.link = (uint32_t)lights[start].first | (1u << 31);
            return {nodeIndex, lights[start].second};
        }
        float bounds[6] = {fmax, fmax, fmax, flow, flow, flow}, cb[6] = {fmax, fmax, fmax, flow, flow, flow};
        for (int i = start; i < end; ++i) {
            const LightBounds &lb = lights[i].second;
            bounds_union(bounds, lb.b, bounds);
            float c[3];
            centroid(lb, c);
            for (int k = 0; k < 3; ++k) {
                cb[k] = std::min(cb[k], c[k]);
                cb[3 + k] = std::max(cb[3 + k], c[k]);
            }
        }
        float minCost = std::numeric_limits<float>::infinity();
        int minCostSplitBucket = -1, minCostSplitDim = -1;
        constexpr int nBuckets = 12;
        for (int dim = 0; dim < 3; ++dim) {
            if (cb[3 + dim] == cb[dim]) continue;
            LightBounds bucket[nBuckets];
            for (int i = start; i < end; ++i) {
                float pc[3];
                centroid(lights[i].second, pc);
                int b = (int)(nBuckets * offset(cb, pc, dim));
                if (b == nBuckets) b = nBuckets - 1;
                bucket[b] = lb_union(bucket[b], lights[i].second);
            }
            float cost[nBuckets - 1];
            for (int i = 0; i < nBuckets - 1; ++i) {
                LightBounds b0, b1;
                for (int j = 0; j <= i; ++j) b0 = lb_union(b0, bucket[j]);
                for (int j = i + 1; j < nBuckets; ++j) b1 = lb_union(b1, bucket[j]);
                cost[i] = evaluate_cost(b0, bounds, dim) + evaluate_cost(b1, bounds, dim);
            }
            for (int i = 1; i < nBuckets - 1; ++i)
                if (cost[i] > 0 && cost[i] < minCost) {
                    minCost = cost[i];
                    minCostSplitBucket = i;
                    minCostSplitDim = dim;
                }
        }
        int mid;
        if (minCostSplitDim == -1) {
            mid = (start + end) / 2;
        } else {
            const Item *pmid = std::partition(&lights[start], &lights[end - 1] + 1, [=](const Item &l) {
                float pc[3];
                centroid(l.second, pc);
                int b = (int)(nBuckets * offset(cb, pc, minCostSplitDim));
                if (b == nBuckets) b = nBuckets - 1;
                return b <= minCostSplitBucket;
            });
            mid = (int)(pmid - &lights[0]);
            if (mid == start || mid == end) mid = (start + end) / 2;
        }
        const int nodeIndex = t->nNodes++;
        const auto child0 = build(lights, start, mid);
        const auto child1 = build(lights, mid, end);
        (void)child0.first;
        const LightBounds lb = lb_union(child0.second, child1.second);
        Node &n = t->nodes[nodeIndex];
        compact(lb, t->allb, &n);
        n.link = (uint32_t)child1.first;
        return {nodeIndex, lb};
    }
};

// BVHLightSampler's constructor (lightsamplers.cpp:109-133) over a light list: bounded[i] says
// whether light i has bounds (a local light), lb[i] holds them. Lights without bounds become the
// infinite lights; bounded ones with phi > 0 enter the tree.
inline void build_tree(int n, const bool *bounded, const LightBounds *lb, Tree *t) {
    *t = Tree{};
    constexpr float fmax = std::numeric_limits<float>::max(), flow = std::numeric_limits<float>::lowest();
    for (int c = 0; c < 3; ++c) t->allb[c] = fmax, t->allb[3 + c] = flow;
    std::vector<Builder::Item> bvh;
    for (int i = 0; i < n && i < kMaxTreeLights; ++i) {
        if (!bounded[i]) t->inf[t->nInf++] = i;
        else if (lb[i].phi > 0) {
            bvh.push_back({i, lb[i]});
            bounds_union(t->allb, lb[i].b, t->allb);
        }
    }
    if (!bvh.empty()) {
        Builder b{t};
        b.build(bvh, 0, (int)bvh.size());
    }
}

}  // namespace ll
}  // namespace avr
