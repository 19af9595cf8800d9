// avr_graph_uniform.h — the uniform (voxel) lighting graph: UniformGraph (graph/graph.h:195,
// graph.cpp:545-577), FitToGraph (graph/util.h:302-311), FreeGraph::ToUniform's vertex part
// (graph.cpp:597-604) and what GraphIntegrator's uniform branch asks of it
// (graph_integrator.cpp:89-178): the vertex of a point's voxel, and, for --graph-debug
// (:104-131), the lit voxel a ray enters first. One set of routines, compiled for the host
// (avr_graph_uniform_*) and for the device (k_graph_uniform_lookup, k_graph_uniform_trace,
// k_graph_render_uniform): the semantics below are the contract of both.
//
// Coordinates: per axis q = p / spacing (a float division), r = roundf(q) (half away from
// zero, std::round), valid iff |r| < 2^20 (NaN is not), c = (int)r. The reference casts any
// value; the range is limited here so that the three coordinates pack into one 64-bit key,
// (cx + 2^20) | (cy + 2^20) << 21 | (cz + 2^20) << 42. The vertex's point is (float)c * spacing
// per axis (coors * spacing, graph.cpp:555).
//
// Table: open addressing with linear probing over 16-B entries {key, id, light}; capacity the
// smallest power of two >= 2 m, at least 16; slot = MixBits(key) & (capacity - 1); the empty
// key is all ones (no valid key: bit 63 is never set). It also carries the coordinate bounds of
// its vertices. This is the only lookup structure.
//
// First lit voxel (uniform_first_lit): among the vertices with light != 0, the one whose box
// [mid - spacing / 2, mid + spacing / 2] (floats, as Initialize builds voxelBounds) the ray
// enters first, with hit0 and hit1 of Bounds3::IntersectP(o, d, Infinity, &hit0, &hit1) in
// intersect_box's arithmetic (t0 from 0, tFar widened by 1 + 2 gamma(3)). The reference loops
// over every lit voxel and keeps the smallest hit0 with a strict <, in unordered-map order;
// here equal hit0 go to the lower vertex id. The search is a 3-D DDA in double over the lattice
// cells (faces at (k +- 1/2) spacing) from where the ray enters the coordinate bounds: one
// table lookup per cell, the exact IntersectP on each lit candidate, at most (sum of the
// bounds' extents + 3) steps. Once a candidate hits, the walk goes on while the next cell's
// entry is not beyond that hit0 (cells that meet at an edge or corner), keeping the smallest
// (hit0, id). It gives the brute-force answer whenever that answer is unambiguous: the two
// smallest hit0 differ, and the winner's chord hit1 - hit0 is more than rounding.
#pragma once

#include <cmath>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#ifndef AVR_HD
#define AVR_HD inline
#endif

namespace avr {
namespace graph {

constexpr int kUniformCoorLimit = 1 << 20;
constexpr uint64_t kUniformEmpty = ~0ull;

struct alignas(16) UniformEntry {
    uint64_t key;
    int id;
    float light;
};

// What a query reads: the host table, or its device copy
struct UniformView {
    const UniformEntry *tab;
    uint32_t mask;       // capacity - 1
    int lo[3], hi[3];    // coordinate bounds of the vertices
    float spacing;
};

// MixBits (util/hash.h)
AVR_HD uint64_t uniform_mix(uint64_t v) {
    v ^= (v >> 31);
    v *= 0x7fb5d329728ea185ull;
    v ^= (v >> 27);
    v *= 0x81dadef4bc2dd44dull;
    v ^= (v >> 33);
    return v;
}

// FitToGraph for one axis; false: outside +-2^20 or NaN
AVR_HD bool uniform_coor(float p, float spacing, int *c) {
    const float q = p / spacing;
    const float r = __builtin_roundf(q);
    if (!(__builtin_fabsf(r) < (float)kUniformCoorLimit)) return false;
    *c = (int)r;
    return true;
}

AVR_HD bool uniform_coors(float x, float y, float z, float spacing, int c[3]) {
    return uniform_coor(x, spacing, &c[0]) && uniform_coor(y, spacing, &c[1]) && uniform_coor(z, spacing, &c[2]);
}

AVR_HD bool uniform_coor_valid(int c) { return c > -kUniformCoorLimit && c < kUniformCoorLimit; }

AVR_HD uint64_t uniform_key(int cx, int cy, int cz) {
    return (uint64_t)(cx + kUniformCoorLimit) | ((uint64_t)(cy + kUniformCoorLimit) << 21) |
           ((uint64_t)(cz + kUniformCoorLimit) << 42);
}

// The entry of `key`, or null
AVR_HD const UniformEntry *uniform_find(const UniformView &u, uint64_t key) {
    uint32_t slot = (uint32_t)uniform_mix(key) & u.mask;
    for (uint32_t probe = 0; probe <= u.mask; ++probe) {
        const UniformEntry *e = u.tab + slot;
        const uint64_t k = e->key;
        if (k == key) return e;
        if (k == kUniformEmpty) return nullptr;
        slot = (slot + 1) & u.mask;
    }
    return nullptr;
}

// UniformGraph::GetVertexConst(p): the id of the vertex in p's voxel, or -1 (also for an
// invalid coordinate); *light = its lightScalar, 0 without a vertex
AVR_HD int uniform_lookup(const UniformView &u, float x, float y, float z, float *light) {
    *light = 0.f;
    int c[3];
    if (!uniform_coors(x, y, z, u.spacing, c)) return -1;
    const UniformEntry *e = uniform_find(u, uniform_key(c[0], c[1], c[2]));
    if (!e) return -1;
    *light = e->light;
    return e->id;
}

// Bounds3::IntersectP(o, d, Infinity, &hit0, &hit1) of the voxel box around coordinate c
AVR_HD bool uniform_voxel_hit(const int c[3], float spacing, const float o[3], const float d[3], float *hit0, float *hit1) {
    const float half = spacing / 2;
    const float gamma3 = (3 * 5.96046448e-08f) / (1 - 3 * 5.96046448e-08f);
    const float widen = 1 + 2 * gamma3;
    float t0 = 0, t1 = INFINITY;
    for (int i = 0; i < 3; ++i) {
        const float mid = (float)c[i] * spacing;
        const float lo = mid - half, hi = mid + half;
        const float inv = 1 / d[i];
        float tNear = (lo - o[i]) * inv;
        float tFar = (hi - o[i]) * inv;
        if (tNear > tFar) {
            const float tt = tNear;
            tNear = tFar;
            tFar = tt;
        }
        tFar *= widen;
        t0 = tNear > t0 ? tNear : t0;
        t1 = tFar < t1 ? tFar : t1;
        if (t0 > t1) return false;
    }
    *hit0 = t0;
    *hit1 = t1;
    return true;
}

// The lit voxel the ray o + t d, t >= 0, enters first: its vertex id (or -1) and IntersectP's
// hit0, hit1 for its box (0 without a hit)
AVR_HD int uniform_first_lit(const UniformView &u, const float o[3], const float d[3], float *hit0, float *hit1) {
    *hit0 = 0.f;
    *hit1 = 0.f;
    const double s = (double)u.spacing;
    // the ray's stretch inside the slabs [(lo - 1/2) s, (hi + 1/2) s] of the coordinate bounds
    double tIn = 0.0, tOut = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const double oa = (double)o[a], da = (double)d[a];
        const double fLo = ((double)u.lo[a] - 0.5) * s, fHi = ((double)u.hi[a] + 0.5) * s;
        if (!(oa == oa) || !(da == da)) return -1;
        if (da == 0.0) {
            if (oa < fLo || oa > fHi) return -1;
            continue;
        }
        double tn = (fLo - oa) / da, tf = (fHi - oa) / da;
        if (tn > tf) {
            const double tt = tn;
            tn = tf;
            tf = tt;
        }
        tIn = tn > tIn ? tn : tIn;
        tOut = tf < tOut ? tf : tOut;
    }
    if (!(tIn <= tOut)) return -1;
    int c[3], step[3];
    double tNext[3];   // where the ray leaves the current cell along each axis
    long long steps = 3;
    for (int a = 0; a < 3; ++a) {
        const double oa = (double)o[a], da = (double)d[a];
        double k = std::floor((oa + da * tIn) / s + 0.5);
        if (!(k >= (double)u.lo[a])) k = (double)u.lo[a];   // also a NaN from 0 * inf
        if (k > (double)u.hi[a]) k = (double)u.hi[a];
        c[a] = (int)k;
        step[a] = da > 0.0 ? 1 : (da < 0.0 ? -1 : 0);
        tNext[a] = step[a] ? (((double)c[a] + 0.5 * step[a]) * s - oa) / da : INFINITY;
        steps += (long long)u.hi[a] - u.lo[a];
    }
    int best = -1;
    float best0 = 0.f, best1 = 0.f;
    double tCell = tIn;   // where the ray enters the current cell
    for (long long n = 0; n < steps; ++n) {
        if (best >= 0 && tCell > (double)best0) break;
        const UniformEntry *e = uniform_find(u, uniform_key(c[0], c[1], c[2]));
        if (e && e->light != 0.f) {
            float h0, h1;
            // hit0 < minHit0 from Infinity (graph_integrator.cpp:108-119): an infinite hit0 is no hit
            if (uniform_voxel_hit(c, u.spacing, o, d, &h0, &h1) && h0 < INFINITY &&
                (best < 0 || h0 < best0 || (h0 == best0 && e->id < best))) {
                best = e->id;
                best0 = h0;
                best1 = h1;
            }
        }
        int a = 0;
        double tMin = tNext[0];
        if (tNext[1] < tMin) {
            tMin = tNext[1];
            a = 1;
        }
        if (tNext[2] < tMin) {
            tMin = tNext[2];
            a = 2;
        }
        if (!(tMin < INFINITY)) break;   // no axis moves
        tCell = tMin;
        // c[a] += step[a] and its next face, without indexing the arrays at run time
        if (a == 0) {
            c[0] += step[0];
            tNext[0] = (((double)c[0] + 0.5 * step[0]) * s - (double)o[0]) / (double)d[0];
        } else if (a == 1) {
            c[1] += step[1];
            tNext[1] = (((double)c[1] + 0.5 * step[1]) * s - (double)o[1]) / (double)d[1];
        } else {
            c[2] += step[2];
            tNext[2] = (((double)c[2] + 0.5 * step[2]) * s - (double)o[2]) / (double)d[2];
        }
        if (c[0] < u.lo[0] || c[0] > u.hi[0] || c[1] < u.lo[1] || c[1] > u.hi[1] || c[2] < u.lo[2] || c[2] > u.hi[2]) break;
    }
    if (best >= 0) {
        *hit0 = best0;
        *hit1 = best1;
    }
    return best;
}

// The host graph (avr_graph_uniform_*). Create / FromPoints return a message on a bad
// argument, else an empty string.
class Uniform {
  public:
    std::string Create(long long m, const int *coors, const float *light, float spacing) {
        if (!(spacing > 0) || !std::isfinite(spacing)) return "graph uniform: spacing must be positive and finite";
        if (m < 1 || m > 0x3fffffff || !coors || !light) return "graph uniform: at least one vertex required";
        spacing_ = spacing;
        coors_.assign(coors, coors + 3 * m);
        light_.assign(light, light + m);
        size_t cap = 16;
        while (cap < 2 * (size_t)m) cap *= 2;
        tab_.assign(cap, UniformEntry{kUniformEmpty, -1, 0.f});
        for (int a = 0; a < 3; ++a) lo_[a] = hi_[a] = coors[a];
        for (long long v = 0; v < m; ++v) {
            const int *c = coors + 3 * v;
            if (!uniform_coor_valid(c[0]) || !uniform_coor_valid(c[1]) || !uniform_coor_valid(c[2]))
                return "graph uniform: vertex " + std::to_string(v) + ": coordinate outside +-2^20";
            if (light[v] != light[v]) return "graph uniform: vertex " + std::to_string(v) + ": NaN light";
            if (!uniform_insert(tab_, uniform_key(c[0], c[1], c[2]), (int)v, light[v]))
                return "graph uniform: vertex " + std::to_string(v) + ": repeated coordinate";
            for (int a = 0; a < 3; ++a) {
                lo_[a] = c[a] < lo_[a] ? c[a] : lo_[a];
                hi_[a] = c[a] > hi_[a] ? c[a] : hi_[a];
            }
        }
        return "";
    }

    // FreeGraph::ToUniform's vertices: points in ascending id, a new vertex at the first
    // appearance of a voxel; reduce 0 keeps the first point's light (AddVertex returns the
    // existing vertex), reduce 1 the float sum of the voxel's lights in ascending id over
    // (float)count. vertex_of (n, may be null): point -> vertex.
    std::string FromPoints(long long n, const float *xyz, const float *light, float spacing, int reduce, int *vertex_of) {
        if (!(spacing > 0) || !std::isfinite(spacing)) return "graph uniform: spacing must be positive and finite";
        if (n < 1 || n > 0x3fffffff || !xyz || !light) return "graph uniform: at least one vertex required";
        if (reduce != 0 && reduce != 1) return "graph uniform: reduce must be 0 (first) or 1 (mean)";
        std::unordered_map<uint64_t, int> seen;
        std::vector<int> coors, count;
        std::vector<float> sum;
        for (long long v = 0; v < n; ++v) {
            int c[3];
            if (!uniform_coors(xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], spacing, c))
                return "graph uniform: vertex " + std::to_string(v) + ": coordinate outside +-2^20";
            if (light[v] != light[v]) return "graph uniform: vertex " + std::to_string(v) + ": NaN light";
            const auto it = seen.emplace(uniform_key(c[0], c[1], c[2]), (int)count.size());
            const int id = it.first->second;
            if (it.second) {
                coors.insert(coors.end(), c, c + 3);
                count.push_back(0);
                sum.push_back(reduce == 0 ? light[v] : 0.f);
            }
            if (reduce == 1) sum[(size_t)id] += light[v];
            ++count[(size_t)id];
            if (vertex_of) vertex_of[v] = id;
        }
        if (reduce == 1)
            for (size_t i = 0; i < sum.size(); ++i) sum[i] = sum[i] / (float)count[i];
        return Create((long long)count.size(), coors.data(), sum.data(), spacing);
    }

    UniformView View() const {
        UniformView v{};
        v.tab = tab_.data();
        v.mask = (uint32_t)(tab_.size() - 1);
        for (int a = 0; a < 3; ++a) {
            v.lo[a] = lo_[a];
            v.hi[a] = hi_[a];
        }
        v.spacing = spacing_;
        return v;
    }

    void Lookup(long long n, const float *points, int *id, float *light) const {
        const UniformView v = View();
        for (long long i = 0; i < n; ++i) {
            float l = 0.f;
            const int k = uniform_lookup(v, points[3 * i], points[3 * i + 1], points[3 * i + 2], &l);
            if (id) id[i] = k;
            if (light) light[i] = l;
        }
    }

    void Trace(long long n, const float *o, const float *d, int *id, float *hit0, float *hit1) const {
        const UniformView v = View();
        for (long long i = 0; i < n; ++i) {
            float h0 = 0.f, h1 = 0.f;
            const int k = uniform_first_lit(v, o + 3 * i, d + 3 * i, &h0, &h1);
            if (id) id[i] = k;
            if (hit0) hit0[i] = h0;
            if (hit1) hit1[i] = h1;
        }
    }

    size_t NumVertices() const { return light_.size(); }
    size_t Capacity() const { return tab_.size(); }
    float Spacing() const { return spacing_; }
    const int *Coors() const { return coors_.data(); }
    const float *Light() const { return light_.data(); }

  private:
    // false: the key is already there
    static bool uniform_insert(std::vector<UniformEntry> &tab, uint64_t key, int id, float light) {
        const uint32_t mask = (uint32_t)(tab.size() - 1);
        uint32_t slot = (uint32_t)uniform_mix(key) & mask;
        while (tab[slot].key != kUniformEmpty) {
            if (tab[slot].key == key) return false;
            slot = (slot + 1) & mask;
        }
        tab[slot] = UniformEntry{key, id, light};
        return true;
    }

    std::vector<UniformEntry> tab_;
    std::vector<int> coors_;
    std::vector<float> light_;
    int lo_[3] = {0, 0, 0}, hi_[3] = {0, 0, 0};
    float spacing_ = 1;
};

}  // namespace graph
}  // namespace avr
