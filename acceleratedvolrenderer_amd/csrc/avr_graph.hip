// avr_graph.hip — device kernels of the lighting-graph precompute (src/graph/ of the
// reference: the fork's own SampleT_maj callers), included by
// avr_capi.hip after avr_kernels.hip.
//
//  k_graph_walks   FreeGraphBuilder::TracePath (free/free_graph_builder.cpp:19-141), the
//                  medium part: one lane per light path, delta tracking segment by segment,
//                  scatter points written out; the order-dependent vertex merging stays on the
//                  host (avr_graph_add_walks), because a walk never depends on the graph.
//  k_graph_disk    LightingCalculator::GetLightVector (lighting_calculator.cpp:84-155): one
//                  lane per vertex enumerates its disk points (graph/util.h:179-204) and the
//                  ray/box/sphere crossings (util.h:419-503).
//  k_graph_tr      ComputeRaysToSphere (util.h:814-840) + SampleTransmittance (util.h:344-366):
//                  one lane per (vertex, disk point, iteration) ratio-tracking estimate.
//  k_graph_average the two Averager::GetAverage levels (util.h:545-565) and Inv4Pi.
//  k_graph_spmv    ComputeFinalLight's transport product (lighting_calculator.cpp:23-59):
//                  CSR row per lane, terms summed in ascending column order (Eigen's
//                  column-major sparse x sparse-vector order), NaN/Inf flag per bounce; the
//                  previous bounce's vector is added to the total in the same pass.
//  k_graph_connect GraphIntegrator::ConnectToGraph (graph_integrator.cpp:249-280) for a batch
//                  of graph-space points: index_connect (avr_graph_index.h), one lane per point.
//  k_graph_knn     FreeGraphBuilder::ComputeSearchRanges (free_graph_builder.cpp:473-548):
//  k_graph_range_average  index_knn per vertex (one lane per sorted slot) with the first
//                  Averager level, then the second level over each vertex's neighbours.
//  k_graph_render  GraphIntegrator::Li, free-graph branch (graph_integrator.cpp:180-247): one
//                  lane per camera record of the pass; delta tracking to the first real
//                  scatter, then the same index_connect.
//  k_graph_render_uniform  GraphIntegrator::Li, uniform-graph branch (:89-178): the same walk to
//  k_graph_uniform_lookup  the first real scatter (graph_first_scatter), then one hashed lookup
//  k_graph_uniform_trace   of the point's voxel (avr_graph_uniform.h); --graph-debug's voxel
//                  view (:104-131) as its kView 1; the lookup and the first-lit-voxel search
//                  for batches of points and rays.
//  k_graph_coverage  IntegrationAnalyzer's Analyze (analysis/integration_analyzer.cpp:56-83)
//                  for a batch of graph-space points: index_coverage, one lane per point.
//  k_graph_analyze IntegrationAnalyzer::AnalyzeRay (:55-163): one lane per camera record walks
//  k_graph_analyze_reduce  on as k_graph_walks does and analyses up to maxDepth scatters;
//                  then one lane per pixel adds the pass's records to the pixel's sums.
//  k_graph_start_rays  BuildGraph's ray grid (free_graph_builder.cpp:143-199): one lane per
//                  grid ray, its crossing of the primitive and SkipIntersection.
//  k_graph_merge_round  the vertex merge of TracePath (:71-93) in rounds (avr_graph_merge.h):
//  k_graph_merge_flags  one lane per unfinalised scatter point runs merge_step; then the
//  k_graph_merge_scan   id scan over the final states (new-vertex flags per wave, their
//  k_graph_merge_ids    prefix sums, vertex_of_point).
//  k_graph_capture  VoxelBoundary::CaptureBoundary's ray bundles (voxels/voxel_boundary.cpp:13-62):
//                  one lane per ray, the primitive's crossing, then the majorant DDA up to the
//                  first non-empty cell.
//  k_graph_uniform_insert  FreeGraph::ToUniform's vertex part for points on the device: one lane
//  k_graph_uniform_first   per point inserts its voxel key into an open-addressing set (64-bit
//                  compare-and-swap) and keeps the key's lowest point index (atomic min); the
//                  ids then come from k_graph_merge_flags / _scan / _ids.
//  k_graph_voxels_level  one level of the voxel boundary's floods (avr_graph_voxels.h): one lane
//                  per frontier cell, the next level appended with one atomic per wave.
//
// Geometry model (shared with the oracle): the medium's boundary primitive is
// its bounds box (medium-space slab test, ray mapped without error offsets), kGeom 0, or, on
// request (avr_graph_set_geometry, kGeom 1), the medium's interface: the sphere or the convex
// polyhedron of avr_medium_boundary_*, solved once from the ray's own origin. Spheres solve
// Sphere::BasicIntersect's interval quadric once for both roots. The geometry is a template
// parameter: the kGeom 0 instantiations are the box-only kernels' code.
#include "avr_graph_index.h"
#include "avr_graph_merge.h"
#include "avr_graph_uniform.h"
#include "avr_graph_voxels.h"

namespace avr {
namespace graph {

// ray / sphere crossings and the hit kinds: avr_boundary.h (shared with the path kernels)
using namespace ::avr::shape;

// GetHits(primitive) in the model (util.h:419-458): slab test in medium space
__device__ __forceinline__ Hits box_hits(const DevMedium &m, V3 o, V3 d) {
    const V3 om = xf_point_lr(m.medium_from_render, o), dm = xf_vector(m.medium_from_render, d);
    float t0, t1;
    if (!intersect_box(m.bmin, m.bmax, om, dm, kInf, &t0, &t1)) return {kOutsideZeroHits, 0.f, 0.f};
    if (t0 > 0) return {kOutsideTwoHits, t0, t1};
    return {kInsideOneHit, t1, 0.f};
}

// GetHits(primitive) of the graph geometry kGeom: 0 the bounds box; 1 the medium's interface
// (the sphere for boundary 1, the convex polyhedron for boundary 2, the box without one).
// One solve from o, no surface offset: OutsideTwoHits {t0, t1}, InsideOneHit {exit}.
template <int kGeom>
__device__ __forceinline__ Hits primitive_hits(const DevMedium &m, V3 o, V3 d) {
    if constexpr (kGeom != 0) {
        if (m.boundary == 1) return sphere_hits(V3{m.sph[0], m.sph[1], m.sph[2]}, m.sph[3], o, d);
        if (m.boundary == 2) return convex_hits(m.planes, m.n_planes, o, d);
    }
    return box_hits(m, o, d);
}

__device__ __forceinline__ void coordinate_system(V3 v1, V3 *v2, V3 *v3) {   // vecmath.h:1007-1013
    const float sign = __builtin_copysignf(1.f, v1.z);
    const float a = -1 / (sign + v1.z);
    const float b = v1.x * v1.y * a;
    *v2 = {1 + sign * sqr(v1.x) * a, sign * b, -sign * v1.x};
    *v3 = {b, sign + sqr(v1.y) * a, -v1.y};
}

// Sampling index -> pixel (util.h:816-817)
__device__ __forceinline__ void index_pixel(unsigned long long index, int resX, int *px, int *py) {
    *py = (int)(index / (unsigned long long)resX);
    *px = (int)(index - (unsigned long long)*py * (unsigned long long)resX);
}

// One disk point's ray after the crossings (k_graph_disk -> k_graph_tr)
struct DiskRec {
    float4 o_start;      // ray origin at the medium entry (SkipIntersection), startScatterT
    float dist;          // distInSphere (endScatterT - startScatterT)
    int valid;           // crossed both the box and the sphere inside the medium
};

}  // namespace graph

// The medium walk of FreeGraphBuilder::TracePath (free_graph_builder.cpp:19-141), which
// IntegrationAnalyzer::AnalyzeRay (integration_analyzer.cpp:85-162) repeats for a camera ray:
// per segment RNG(Hash(Get1D()), Hash(Get1D())), SampleT_maj with the next Get1D and the
// 3-way event choice on channel 0; the first segment ends at tFirst, a later one where the
// ray from the scatter point leaves the primitive (primitive_hits). Every real scatter point goes to
// onScatter(k, p), up to maxDepth of them; between two the direction comes from the HG
// Sample_p(-d, Get2D()). Absorption, leaving the medium and the maxDepth-th scatter end the
// walk (draws after that scatter cannot reach a result). Returns the scatters seen.
template <int kGeom, typename Sampler, typename F>
__device__ __forceinline__ int graph_walk(const Params &P, const float *maj, Sampler &smp, V3 ro, V3 rd, float tFirst,
                                          int maxDepth, const Spec &sig_a, const Spec &sig_s, const Spec &lam,
                                          unsigned long long &nLookup, unsigned long long &nSteps, F onScatter) {
    bool usedTHit = false;
    int k = 0;
    while (k < maxDepth) {
        const float h0 = smp.get1d(P);
        const float h1 = smp.get1d(P);
        Pcg32 rng;
        rng.set_sequence(hash_u32(f2u(h0)), hash_u32(f2u(h1)));
        float tMax;
        if (!usedTHit) {
            tMax = tFirst;
            usedTHit = true;
        } else {
            const graph::Hits h = graph::primitive_hits<kGeom>(P.med, ro, rd);
            if (h.type == graph::kOutsideZeroHits) break;
            tMax = h.t0;
        }
        bool scattered = false;
        V3 pS = {0.f, 0.f, 0.f};
        const float u = smp.get1d(P);
        auto cb = [&](V3 p, const MediumSample &ms, const Spec &sigma_maj, const Spec &) -> bool {
            const float pAbsorb = ms.sigma_a.v0 / sigma_maj.v0;
            const float pScat = ms.sigma_s.v0 / sigma_maj.v0;
            const float pNull = fmaxf_(0.f, 1 - pAbsorb - pScat);
            const int mode = sample_discrete3(pAbsorb, pScat, pNull, rng.uniform());
            if (mode == 0) return false;
            if (mode == 1) {
                scattered = true;
                pS = p;
                return false;
            }
            return true;
        };
        sample_t_maj(P.med, maj, Ray{ro, rd}, tMax, u, rng, sig_a, sig_s, Spec::c(0.f), lam, nLookup, nSteps, cb);
        if (!scattered) break;
        onScatter(k, pS);
        ++k;
        if (k == maxDepth) break;
        float u0, u1, pdf;
        smp.get2d(P, &u0, &u1);
        const V3 wi = hg_sample(-rd, P.med.g, u0, u1, &pdf);
        ro = pS;
        rd = wi;
    }
    return k;
}

// skipDims: sampler dimensions already drawn after StartPixelSample before TracePath (the
// reinforcement rays' phase sample, free_graph_builder.cpp:448-451)
template <bool kZSobol, int kGeom>
__global__ void __launch_bounds__(256) k_graph_walks(Params P, long long nPaths, int iterations, const float *__restrict__ o,
                                                     const float *__restrict__ d, const float *__restrict__ tFirst,
                                                     const long long *__restrict__ index0, int sampleIndex, int skipDims,
                                                     int resX, int maxDepth, float *__restrict__ points,
                                                     int *__restrict__ counts) {
    __shared__ float s_maj[4096];
    const float *maj = stage_majorant(P.med, s_maj);
    const Lambda lw = sample_visible(0.f);   // mediumData.defaultLambda = film.SampleWavelengths(0)
    const Spec lam = lw.l;
    const LambdaIdx li = lambda_index(lam);
    const Spec sig_a = sample_table(P.med.sigma_a, li), sig_s = sample_table(P.med.sigma_s, li);
    unsigned long long nLookup = 0, nSteps = 0, nIn = 0;
    for (long long path = blockIdx.x * (long long)blockDim.x + threadIdx.x; path < nPaths;
         path += (long long)gridDim.x * blockDim.x) {
        ++nIn;
        const long long r = path / iterations, i = path - r * iterations;
        int px, py;
        graph::index_pixel((unsigned long long)(index0[r] + i), resX, &px, &py);
        PathSampler<kZSobol> smp;
        smp.start(P, px, py, sampleIndex);
        for (int k = 0; k < skipDims; ++k) (void)smp.get1d(P);
        const V3 ro = {o[3 * r], o[3 * r + 1], o[3 * r + 2]}, rd = {d[3 * r], d[3 * r + 1], d[3 * r + 2]};
        counts[path] = graph_walk<kGeom>(P, maj, smp, ro, rd, tFirst[r], maxDepth, sig_a, sig_s, lam, nLookup, nSteps,
                                  [&](int k, V3 pS) {
                                      float *dst = points + 3 * (path * maxDepth + k);
                                      dst[0] = pS.x;
                                      dst[1] = pS.y;
                                      dst[2] = pS.z;
                                  });
    }
    flush_stat(P.stats, 3, nLookup);
    flush_stat(P.stats, 4, nIn);
    flush_stat(P.stats, 6, nSteps);
}

// FreeGraphBuilder::ReinforceSparseVertices' rays (free_graph_builder.cpp:434-475), one lane
// per listed vertex: StartPixelSample({0, 0}, cycle) on a copy of the sampler, then
// GetSphereVolumePointsRandom (util.h:238-252: rejection sampling in the cube; the three
// Get1D of one Point3f are GCC-evaluated right to left, so the first draw is z; the
// arithmetic is (double(u) - 0.5) * 2 * radius), then per point StartPixelSample(pixel(id *
// nRays + point), cycle), the medium's HG Sample_p((1, 0, 0), Get2D()), GetHits(primitive) and
// SkipIntersection. valid = RayEntersVolume (OutsideTwoHits or InsideOneHit).
template <bool kZSobol, int kGeom>
__global__ void __launch_bounds__(256) k_graph_reinforce_rays(Params P, int n, const int *__restrict__ ids,
                                                              const float *__restrict__ pts, float radius, int nRays,
                                                              int cycle, int resX, float *__restrict__ o,
                                                              float *__restrict__ d, float *__restrict__ tFirst,
                                                              int *__restrict__ valid) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const V3 c = {pts[3 * v], pts[3 * v + 1], pts[3 * v + 2]};
    PathSampler<kZSobol> cube;
    cube.start(P, 0, 0, cycle);
    const double r = (double)radius;
    for (int k = 0; k < nRays;) {
        const float pz = (float)(((double)cube.get1d(P) - 0.5) * 2 * r);
        const float py = (float)(((double)cube.get1d(P) - 0.5) * 2 * r);
        const float px = (float)(((double)cube.get1d(P) - 0.5) * 2 * r);
        const V3 q = {px, py, pz};
        if (!(length(q) < radius)) continue;
        const long long ray = (long long)v * nRays + k;
        const V3 sp = q + c;
        int pxl, pyl;
        graph::index_pixel((unsigned long long)ids[v] * (unsigned long long)nRays + (unsigned long long)k, resX, &pxl,
                           &pyl);
        PathSampler<kZSobol> smp;
        smp.start(P, pxl, pyl, cycle);
        float u0, u1, pdf;
        smp.get2d(P, &u0, &u1);
        const V3 dir = hg_sample(V3{1.f, 0.f, 0.f}, P.med.g, u0, u1, &pdf);
        const graph::Hits h = graph::primitive_hits<kGeom>(P.med, sp, dir);
        V3 og = sp;
        float t = 0.f;
        int ok = 0;
        if (h.type == graph::kOutsideTwoHits) {
            og = sp + dir * h.t0;
            t = h.t1 - h.t0;
            ok = 1;
        } else if (h.type == graph::kInsideOneHit) {
            t = h.t0;
            ok = 1;
        }
        o[3 * ray] = og.x; o[3 * ray + 1] = og.y; o[3 * ray + 2] = og.z;
        d[3 * ray] = dir.x; d[3 * ray + 1] = dir.y; d[3 * ray + 2] = dir.z;
        tFirst[ray] = t;
        valid[ray] = ok;
        ++k;
    }
}

// BuildGraph's ray grid (free_graph_builder.cpp:143-199), one lane per grid ray (x, y) of the
// steps x steps grid, x outer (ray = (x - 1) * steps + (y - 1)): the grid's corner is center -
// inDir * maxDist * 2 - (xv + yv) * maxDist with (xv, yv) = CoordinateSystem(inDir), its step
// maxDist * 2 / (steps + 1); ray (x, y) starts at (corner + xv * step * x) + yv * step * y, then
// GetHits(primitive) and SkipIntersection (no offset). type = the hit kind, o the origin after
// the skip (the grid point itself without a hit), tFirst the first segment's tMax (0 without).
template <int kGeom>
__global__ void __launch_bounds__(256) k_graph_start_rays(DevMedium m, V3 center, float maxDist, V3 dir, int steps,
                                                          int *__restrict__ type, float *__restrict__ o,
                                                          float *__restrict__ tFirst) {
    const long long n = (long long)steps * steps;
    for (long long ray = blockIdx.x * (long long)blockDim.x + threadIdx.x; ray < n;
         ray += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(ray / steps) + 1, y = (int)(ray - (long long)(x - 1) * steps) + 1;
        V3 xv, yv;
        graph::coordinate_system(dir, &xv, &yv);
        V3 origin = center - (dir * maxDist) * 2.f;
        origin = origin - (xv + yv) * maxDist;
        const float step = (maxDist * 2.f) / (float)(steps + 1);
        xv = xv * step;
        yv = yv * step;
        V3 p = (origin + xv * (float)x) + yv * (float)y;
        const graph::Hits h = graph::primitive_hits<kGeom>(m, p, dir);
        float t = 0.f;
        if (h.type == graph::kOutsideTwoHits) {
            p = p + dir * h.t0;
            t = h.t1 - h.t0;
        } else if (h.type == graph::kInsideOneHit) {
            t = h.t0;
        }
        type[ray] = h.type;
        o[3 * ray] = p.x; o[3 * ray + 1] = p.y; o[3 * ray + 2] = p.z;
        tFirst[ray] = t;
    }
}

// Per vertex: disk points around vertex - inDir * maxDistToCenter * 2 (GetDiskPoints, util.h:179-204,
// grid order x then y), the primitive and vertex-sphere crossings of the ray along inDir from each,
// GetStartEndT (util.h:484-503), SkipIntersection to the medium entry and SkipForward.
template <int kGeom>
__global__ void __launch_bounds__(256) k_graph_disk(DevMedium m, int nv, const float *__restrict__ verts, V3 dir,
                                                    float radius, int n, float maxDist, int maxPts,
                                                    graph::DiskRec *__restrict__ rec, int *__restrict__ npts) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nv) return;
    const V3 c = {verts[3 * v], verts[3 * v + 1], verts[3 * v + 2]};
    const V3 origin = c - (dir * maxDist) * 2.f;
    V3 xv, yv;
    graph::coordinate_system(dir, &xv, &yv);
    const float step = radius / (float)(n + 1);
    xv = xv * step;
    yv = yv * step;
    int k = 0;
    for (int x = -n; x <= n; ++x)
        for (int y = -n; y <= n; ++y) {
            V3 p = (n == 0) ? origin : (origin + (float)x * xv) + (float)y * yv;
            if (n != 0 && length(p - origin) > radius) continue;
            graph::DiskRec r;
            r.valid = 0;
            r.dist = 0.f;
            r.o_start = make_float4(0.f, 0.f, 0.f, 0.f);
            const graph::Hits mh = graph::primitive_hits<kGeom>(m, p, dir), sh = graph::sphere_hits(c, radius, p, dir);
            if (mh.type == graph::kOutsideTwoHits && sh.type == graph::kOutsideTwoHits) {
                const float startT = mh.t0, endT = graph::smin(mh.t1, sh.t1), startScatterT = graph::smax(mh.t0, sh.t0);
                const float endScatterT = endT;
                if (!(endT < startScatterT || endScatterT < startT)) {
                    const V3 os = p + dir * startT;
                    r.o_start = make_float4(os.x, os.y, os.z, startScatterT - startT);
                    r.dist = (endScatterT - startT) - (startScatterT - startT);
                    r.valid = 1;
                }
            }
            if (k < maxPts) rec[(long long)v * maxPts + k] = r;
            ++k;
        }
    npts[v] = k;
}

// One ratio-tracking estimate per lane: (vertex v0 + j / (maxPts * iterations), point, iteration).
template <bool kZSobol>
__global__ void __launch_bounds__(256) k_graph_tr(Params P, int v0, int nvChunk, int maxPts, int iterations, V3 dir,
                                                  int resX, const graph::DiskRec *__restrict__ rec,
                                                  const int *__restrict__ npts, float *__restrict__ tr) {
    __shared__ float s_maj[4096];
    const float *maj = stage_majorant(P.med, s_maj);
    const Lambda lw = sample_visible(0.f);
    const Spec lam = lw.l;
    const LambdaIdx li = lambda_index(lam);
    const Spec sig_a = sample_table(P.med.sigma_a, li), sig_s = sample_table(P.med.sigma_s, li);
    unsigned long long nLookup = 0, nSteps = 0, nIn = 0;
    const long long total = (long long)nvChunk * maxPts * iterations;
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < total;
         j += (long long)gridDim.x * blockDim.x) {
        const int i = (int)(j % iterations);
        const long long vk = j / iterations;
        const int k = (int)(vk % maxPts);
        const int v = v0 + (int)(vk / maxPts);
        const int np = npts[v];
        if (k >= np) continue;
        const graph::DiskRec r = rec[(long long)v * maxPts + k];
        if (!r.valid) continue;
        ++nIn;
        int px, py;
        graph::index_pixel((unsigned long long)v * (unsigned long long)np + (unsigned long long)k, resX, &px, &py);
        PathSampler<kZSobol> smp;
        smp.start(P, px, py, i);
        const float curDist = r.dist * smp.get1d(P);
        const float curT = r.o_start.w + curDist;
        // RNG rng(Hash(Get1D()), Hash(Get1D())) (util.h:346): GCC evaluates the two arguments
        // right to left, so the first draw is the offset and the second the sequence index
        const float uOff = smp.get1d(P);
        const float uSeq = smp.get1d(P);
        Pcg32 rng;
        rng.set_sequence(hash_u32(f2u(uSeq)), hash_u32(f2u(uOff)));
        float Tr = 1.f;
        const float u = smp.get1d(P);
        auto cb = [&](V3, const MediumSample &ms, const Spec &sigma_maj, const Spec &) -> bool {
            const float sigma_n = fmaxf_(0.f, (sigma_maj.v0 - ms.sigma_a.v0) - ms.sigma_s.v0);
            Tr *= sigma_n / sigma_maj.v0;
            return Tr != 0;
        };
        sample_t_maj(P.med, maj, Ray{{r.o_start.x, r.o_start.y, r.o_start.z}, dir}, curT, u, rng, sig_a, sig_s,
                     Spec::c(0.f), lam, nLookup, nSteps, cb);
        tr[j] = Tr;
    }
    flush_stat(P.stats, 3, nLookup);
    flush_stat(P.stats, 4, nIn);
    flush_stat(P.stats, 6, nSteps);
}

// Averager::GetAverage (util.h:545-565, unit weights) over the iterations of each valid disk
// point, then over the points; light = average * Inv4Pi (lighting_calculator.cpp:151-152).
__global__ void __launch_bounds__(256) k_graph_average(int v0, int nvChunk, int maxPts, int iterations,
                                                       const graph::DiskRec *__restrict__ rec,
                                                       const int *__restrict__ npts, const float *__restrict__ tr,
                                                       float *__restrict__ light) {
    const int vc = blockIdx.x * blockDim.x + threadIdx.x;
    if (vc >= nvChunk) return;
    const int v = v0 + vc;
    const int np = npts[v] < maxPts ? npts[v] : maxPts;
    float avg = 0.f, w = 0.f;
    for (int k = 0; k < np; ++k) {
        if (!rec[(long long)v * maxPts + k].valid) continue;
        const float *t = tr + ((long long)vc * maxPts + k) * iterations;
        float a = 0.f, wi = 0.f;
        for (int i = 0; i < iterations; ++i) {
            a += t[i] * 1.f;
            wi += 1.f;
        }
        a = wi == 0 ? 0.f : a / wi;
        avg += a * 1.f;
        w += 1.f;
    }
    light[v] = (w == 0 ? 0.f : avg / w) * kInv4Pi;
}

// One bounce of ComputeFinalLight: next = T * cur by CSR rows (terms in ascending column order,
// the first product starting the sum), flag[it] |= NaN/Inf in next; and, unless an earlier
// bounce was flagged, total += cur for it >= 1 (the previous bounce's product).
__global__ void __launch_bounds__(256) k_graph_spmv(int n, const int *__restrict__ rowptr, const int *__restrict__ col,
                                                    const float *__restrict__ val, const float *__restrict__ cur,
                                                    float *__restrict__ next, float *__restrict__ total,
                                                    int *__restrict__ flags, int it) {
    bool stopped = false;
    if (it >= 1)
        for (int j = 0; j < it; ++j) stopped |= flags[j] != 0;
    bool bad = false;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gridDim.x * blockDim.x) {
        const int e0 = rowptr[row], e1 = rowptr[row + 1];
        float acc = 0.f;
        if (e0 < e1) {
            acc = val[e0] * cur[col[e0]];
            for (int e = e0 + 1; e < e1; ++e) acc = acc + val[e] * cur[col[e]];
        }
        next[row] = acc;
        bad |= __builtin_isnan(acc) || __builtin_isinf(acc);
        if (it >= 1 && !stopped) total[row] += cur[row];
    }
    if (__ballot(bad) != 0 && __lane_id() == 0) atomicOr(flags + it, 1);
}

// The last bounce's product added unless a flag stopped the iteration (also the first-order
// copy total = light happens on the host side of the stream, hipMemcpyAsync).
__global__ void __launch_bounds__(256) k_graph_accumulate(int n, const float *__restrict__ cur, float *__restrict__ total,
                                                          const int *__restrict__ flags, int it) {
    for (int j = 0; j < it; ++j)
        if (flags[j]) return;
    for (int row = blockIdx.x * blockDim.x + threadIdx.x; row < n; row += gridDim.x * blockDim.x) total[row] += cur[row];
}

// index_connect's sorted keys in LDS: entry i of this lane at [i * 256] (consecutive lanes in
// consecutive banks), 2 x 16 KiB per block; the buffer is indexed at run time, so registers
// would turn into scratch
struct ConnectBufLds {
    float *d;
    int *s;
    __device__ __forceinline__ float &d2(int i) { return d[i * 256]; }
    __device__ __forceinline__ int &slot(int i) { return s[i * 256]; }
};

// ConnectToGraph for n points already in graph space (avr_graph_connect)
__global__ void __launch_bounds__(256) k_graph_connect(graph::IndexView ix, long long n, const float *__restrict__ pts,
                                                       float *__restrict__ light, int *__restrict__ count) {
    __shared__ float s_d2[graph::kConnectBuf * 256];
    __shared__ int s_slot[graph::kConnectBuf * 256];
    ConnectBufLds buf{s_d2 + threadIdx.x, s_slot + threadIdx.x};
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int cnt = 0, stage = 0;
        light[i] = graph::index_connect(ix, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], buf, &cnt, &stage);
        count[i] = cnt;
    }
}

// GetNClosest for every vertex (avr_graph_knn, avr_graph_search_ranges): index_knn, one lane
// per sorted slot, so that the lanes of a wave scan the same cells; row id[slot] of ids / d2
// (k each) gets the result, and avg[id[slot]] (when given) the first Averager level over the
// row this lane has just written. The sorted buffer is index_connect's, in LDS.
__global__ void __launch_bounds__(256) k_graph_knn(graph::IndexView ix, int n, int k, int *__restrict__ ids,
                                                   float *__restrict__ d2, float *__restrict__ avg) {
    __shared__ float s_d2[graph::kConnectBuf * 256];
    __shared__ int s_slot[graph::kConnectBuf * 256];
    ConnectBufLds buf{s_d2 + threadIdx.x, s_slot + threadIdx.x};
    for (long long s = blockIdx.x * (long long)blockDim.x + threadIdx.x; s < n; s += (long long)gridDim.x * blockDim.x) {
        const int id = ix.id[s];
        float *row = d2 + (size_t)id * (size_t)k;
        (void)graph::index_knn(ix, (int)s, k, buf, ids + (size_t)id * (size_t)k, row);
        if (avg) avg[id] = graph::index_knn_average(row, k);
    }
}

// ComputeSearchRanges' second Averager level: one lane per vertex gathers its neighbours' avg
__global__ void __launch_bounds__(256) k_graph_range_average(int n, int k, const int *__restrict__ ids,
                                                             const float *__restrict__ avg, float *__restrict__ range) {
    for (long long v = blockIdx.x * (long long)blockDim.x + threadIdx.x; v < n; v += (long long)gridDim.x * blockDim.x)
        range[v] = graph::index_range_average(avg, (int)v, ids + (size_t)v * (size_t)k, k);
}

// Where a camera record's ray starts in the graph geometry's primitive (primitive_hits): a ray
// from outside at its entry point with tMax = t1 - t0, a camera inside at its origin with the
// exit as tMax; false on a miss.
template <int kGeom>
__device__ __forceinline__ bool graph_camera_start(const DevMedium &m, V3 o, V3 d, V3 *ro, float *tMax) {
    const graph::Hits h = graph::primitive_hits<kGeom>(m, o, d);
    if (h.type == graph::kOutsideZeroHits) return false;
    *ro = o;
    *tMax = h.t0;
    if (h.type == graph::kOutsideTwoHits) {
        *ro = o + d * h.t0;
        *tMax = h.t1 - h.t0;
    }
    return true;
}

// GraphIntegrator::Li up to the first real scatter, the same for the free and the uniform
// graph (graph_integrator.cpp:134-170, :205-243): graph_camera_start (a miss draws nothing),
// hash0 and hash1 seed the RNG, SampleT_maj with the next Get1D, the medium's coefficients at
// the sample's own wavelengths and the 3-way event choice on channel 0. The scatter point goes
// to pS, and onScatter(li) runs after a real scatter, with the wavelengths' table offsets;
// absorption or leaving the primitive leave pS alone and call nothing.
template <int kGeom, typename Sampler, typename F>
__device__ __forceinline__ void graph_first_scatter(const Params &P, const float *maj, Sampler &smp, V3 o, V3 d,
                                                    const Spec &lam, V3 &pS, unsigned long long &nLookup,
                                                    unsigned long long &nSteps, F onScatter) {
    V3 ro;
    float tMax;
    if (graph_camera_start<kGeom>(P.med, o, d, &ro, &tMax)) {
        const LambdaIdx li = lambda_index(lam);
        const Spec sig_a = sample_table(P.med.sigma_a, li), sig_s = sample_table(P.med.sigma_s, li);
        const float h0 = smp.get1d(P);
        const float h1 = smp.get1d(P);
        Pcg32 rng;
        rng.set_sequence(hash_u32(f2u(h0)), hash_u32(f2u(h1)));
        const float u = smp.get1d(P);
        bool scattered = false;
        auto cb = [&](V3 p, const MediumSample &ms, const Spec &sigma_maj, const Spec &) -> bool {
            const float pAbsorb = ms.sigma_a.v0 / sigma_maj.v0;
            const float pScat = ms.sigma_s.v0 / sigma_maj.v0;
            const float pNull = fmaxf_(0.f, 1 - pAbsorb - pScat);
            const int mode = sample_discrete3(pAbsorb, pScat, pNull, rng.uniform());
            if (mode == 0) return false;
            if (mode == 1) {
                scattered = true;
                pS = p;
                return false;
            }
            return true;
        };
        sample_t_maj(P.med, maj, Ray{ro, d}, tMax, u, rng, sig_a, sig_s, Spec::c(0.f), lam, nLookup, nSteps, cb);
        if (scattered) onScatter(li);
    }
}

// UniformGraph::GetVertexConst for n points already in graph space (avr_graph_uniform_lookup_device)
__global__ void __launch_bounds__(256) k_graph_uniform_lookup(graph::UniformView uv, long long n,
                                                              const float *__restrict__ pts, int *__restrict__ id,
                                                              float *__restrict__ light) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        float l = 0.f;
        id[i] = graph::uniform_lookup(uv, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], &l);
        light[i] = l;
    }
}

// The first lit voxel of n graph-space rays (avr_graph_uniform_trace_device)
__global__ void __launch_bounds__(256) k_graph_uniform_trace(graph::UniformView uv, long long n, const float *__restrict__ o,
                                                             const float *__restrict__ d, int *__restrict__ id,
                                                             float *__restrict__ hit0, float *__restrict__ hit1) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float ro[3] = {o[3 * i], o[3 * i + 1], o[3 * i + 2]}, rd[3] = {d[3 * i], d[3 * i + 1], d[3 * i + 2]};
        float h0 = 0.f, h1 = 0.f;
        id[i] = graph::uniform_first_lit(uv, ro, rd, &h0, &h1);
        hit0[i] = h0;
        hit1[i] = h1;
    }
}

// GraphIntegrator::Li, uniform graph (graph_integrator.cpp:89-178), after k_camera, one lane
// per camera record. kView 0, the render: graph_first_scatter as k_graph_render, then the
// vertex of the scatter point's voxel, L = (lightSpectrum.Sample(lambda) * lightScalar) *
// lightFactor (the reference's Inv4Pi) or 0 without a vertex; side[id] = {p (render space),
// count}: 1 vertex found, 0 scattered without one, -1 no scatter. kView 1, --graph-debug
// (:104-131): no draw and no tracking; the ray from graph_camera_start, mapped to graph space,
// finds its first lit voxel (uniform_first_lit), middle = o' + d' * ((hit0 + hit1) / 2), L =
// lightSpectrum.Sample(lambda) * lightScalar of the vertex at middle; side[id] = {middle
// (graph space), count}: 1 / 0 a lit voxel was hit and middle has / has no vertex, -1 else.
template <bool kZSobol, int kGeom, int kView>
__global__ void __launch_bounds__(256) k_graph_render_uniform(Params P, graph::UniformView uv, Xf graphFromRender,
                                                              float lightFactor, float4 *__restrict__ side) {
    [[maybe_unused]] const float *maj = nullptr;
    if constexpr (kView == 0) {   // the voxel view tracks nothing: no majorant staging
        __shared__ float s_maj[4096];
        maj = stage_majorant(P.med, s_maj);
    }
    const float *lightL = P.lights.list[0].L;   // DistantLight::GetLEmit: scale * Lemit (lights.h:293-297)
    const float lightScale = P.lights.list[0].scale;
    unsigned long long nLookup = 0, nSteps = 0, nIn = 0;
    const int n = P.pass_pixels * P.pass_samples;
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < n; id += gridDim.x * blockDim.x) {
        ++nIn;
        const V3 o = from4(P.ps.o[id]), d = from4(P.ps.d[id]);
        const Spec lam = spec4(P.ps.lambda[id]);
        Spec L = Spec::c(0.f);
        int count = -1;
        V3 pS = {0.f, 0.f, 0.f};
        if constexpr (kView == 0) {
            PathSampler<kZSobol> smp;
            smp.load(P, id);
            graph_first_scatter<kGeom>(P, maj, smp, o, d, lam, pS, nLookup, nSteps, [&](const LambdaIdx &li) {
                const V3 q = xf_point_lr(graphFromRender, pS);
                float light = 0.f;
                count = graph::uniform_lookup(uv, q.x, q.y, q.z, &light) >= 0 ? 1 : 0;
                if (count) L = ((sample_table(lightL, li) * lightScale) * light) * lightFactor;
            });
        } else {
            V3 ro;
            float tMax;
            if (graph_camera_start<kGeom>(P.med, o, d, &ro, &tMax)) {
                const V3 og = xf_point_lr(graphFromRender, ro), dg = xf_vector(graphFromRender, d);
                const float oa[3] = {og.x, og.y, og.z}, da[3] = {dg.x, dg.y, dg.z};
                float hit0, hit1;
                if (graph::uniform_first_lit(uv, oa, da, &hit0, &hit1) >= 0) {
                    pS = og + dg * ((hit0 + hit1) / 2);
                    float light = 0.f;
                    count = graph::uniform_lookup(uv, pS.x, pS.y, pS.z, &light) >= 0 ? 1 : 0;
                    if (count) L = (sample_table(lightL, lambda_index(lam)) * lightScale) * light;
                }
            }
        }
        P.ps.L[id] = to4(L);
        side[id] = make_float4(pS.x, pS.y, pS.z, __int_as_float(count));
    }
    flush_stat(P.stats, 3, nLookup);
    flush_stat(P.stats, 4, nIn);
    flush_stat(P.stats, 6, nSteps);
}

// GraphIntegrator::Li, free graph (graph_integrator.cpp:180-247), after k_camera: the camera
// record's ray crosses the primitive of the graph tools' geometry model (primitive_hits;
// a ray from outside starts at its entry point, as FreeGraphBuilder's rays do; a camera
// inside it, which the reference leaves commented out, tracks from its origin), hash0 and
// hash1 seed the RNG, SampleT_maj runs with the medium's coefficients at the sample's own
// wavelengths and the 3-way event choice on channel 0; the first real scatter p gives
// L = lightSpectrum.Sample(lambda) * ConnectToGraph(graphFromRender(p)), absorption or
// leaving the primitive L = 0. L goes where k_film reads it; side[id] = {p, count} (render space;
// count -1 without a scatter).
template <bool kZSobol, int kGeom>
__global__ void __launch_bounds__(256) k_graph_render(Params P, graph::IndexView ix, Xf graphFromRender,
                                                      float4 *__restrict__ side) {
    __shared__ float s_maj[4096];
    const float *maj = stage_majorant(P.med, s_maj);
    __shared__ float s_d2[graph::kConnectBuf * 256];
    __shared__ int s_slot[graph::kConnectBuf * 256];
    ConnectBufLds buf{s_d2 + threadIdx.x, s_slot + threadIdx.x};
    const float *lightL = P.lights.list[0].L;   // DistantLight::GetLEmit: scale * Lemit (lights.h:293-297)
    const float lightScale = P.lights.list[0].scale;
    unsigned long long nLookup = 0, nSteps = 0, nIn = 0;
    const int n = P.pass_pixels * P.pass_samples;
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < n; id += gridDim.x * blockDim.x) {
        ++nIn;
        const V3 o = from4(P.ps.o[id]), d = from4(P.ps.d[id]);
        const Spec lam = spec4(P.ps.lambda[id]);
        PathSampler<kZSobol> smp;
        smp.load(P, id);
        Spec L = Spec::c(0.f);
        int count = -1;
        V3 pS = {0.f, 0.f, 0.f};
        graph_first_scatter<kGeom>(P, maj, smp, o, d, lam, pS, nLookup, nSteps, [&](const LambdaIdx &li) {
            const V3 q = xf_point_lr(graphFromRender, pS);
            int stage = 0;
            const float conn = graph::index_connect(ix, q.x, q.y, q.z, buf, &count, &stage);
            L = (sample_table(lightL, li) * lightScale) * conn;
        });
        P.ps.L[id] = to4(L);
        side[id] = make_float4(pS.x, pS.y, pS.z, __int_as_float(count));
    }
    flush_stat(P.stats, 3, nLookup);
    flush_stat(P.stats, 4, nIn);
    flush_stat(P.stats, 6, nSteps);
}

// IntegrationAnalyzer's Analyze for n points already in graph space (avr_graph_coverage)
__global__ void __launch_bounds__(256) k_graph_coverage(graph::IndexView ix, long long n, const float *__restrict__ pts,
                                                        int *__restrict__ node, int *__restrict__ inRange,
                                                        float *__restrict__ rangeSum) {
    __shared__ float s_d2[graph::kConnectBuf * 256];
    __shared__ int s_slot[graph::kConnectBuf * 256];
    ConnectBufLds buf{s_d2 + threadIdx.x, s_slot + threadIdx.x};
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        int nd = 0;
        float sum = 0.f;
        inRange[i] = graph::index_coverage(ix, pts[3 * i], pts[3 * i + 1], pts[3 * i + 2], buf, &nd, &sum);
        node[i] = nd;
        rangeSum[i] = sum;
    }
}

namespace graph {

// One sample of the analysis: scatters analysed, those with a vertex within the vertex radius,
// those with a vertex in its search range, the vertices in range and the sum over the scatters,
// in order, of (double)range_sum
struct AnalyzeRec {
    int total, node, search, in_range;
    double range;
};
// One analysed scatter (avr_graph_analyze_last_pass): the point in render space, index_coverage's answer
struct AnalyzeDetail {
    float x, y, z;
    int node, in_range;
    float range_sum;
};
// One pixel's sums over every sample analysed since the last clear
struct AnalyzeAcc {
    unsigned long long total, node, search, in_range;
    double range;
};

}  // namespace graph

// IntegrationAnalyzer::AnalyzeRay (integration_analyzer.cpp:55-163) after k_camera, one lane
// per camera record: the ray starts as k_graph_render's does (primitive_hits; a miss analyses
// nothing) and continues as k_graph_walks' (graph_walk), with the medium's coefficients at the
// sample's own wavelengths; each of at most maxDepth real scatters p is analysed by
// index_coverage(graphFromRender(p)). rec[id] gets the sample's record, detail (when given)
// entry id * maxDepth + k for scatter k.
template <bool kZSobol, int kGeom>
__global__ void __launch_bounds__(256) k_graph_analyze(Params P, graph::IndexView ix, Xf graphFromRender, int maxDepth,
                                                       graph::AnalyzeRec *__restrict__ rec,
                                                       graph::AnalyzeDetail *__restrict__ detail) {
    __shared__ float s_maj[4096];
    const float *maj = stage_majorant(P.med, s_maj);
    __shared__ float s_d2[graph::kConnectBuf * 256];
    __shared__ int s_slot[graph::kConnectBuf * 256];
    ConnectBufLds buf{s_d2 + threadIdx.x, s_slot + threadIdx.x};
    unsigned long long nLookup = 0, nSteps = 0, nIn = 0;
    const int n = P.pass_pixels * P.pass_samples;
    for (int id = blockIdx.x * blockDim.x + threadIdx.x; id < n; id += gridDim.x * blockDim.x) {
        ++nIn;
        const V3 o = from4(P.ps.o[id]), d = from4(P.ps.d[id]);
        const Spec lam = spec4(P.ps.lambda[id]);
        PathSampler<kZSobol> smp;
        smp.load(P, id);
        graph::AnalyzeRec r = {0, 0, 0, 0, 0.0};
        const graph::Hits h = graph::primitive_hits<kGeom>(P.med, o, d);
        if (h.type != graph::kOutsideZeroHits) {
            V3 ro = o;
            float tMax = h.t0;
            if (h.type == graph::kOutsideTwoHits) {
                ro = o + d * h.t0;
                tMax = h.t1 - h.t0;
            }
            const LambdaIdx li = lambda_index(lam);
            const Spec sig_a = sample_table(P.med.sigma_a, li), sig_s = sample_table(P.med.sigma_s, li);
            r.total = graph_walk<kGeom>(P, maj, smp, ro, d, tMax, maxDepth, sig_a, sig_s, lam, nLookup, nSteps, [&](int k, V3 pS) {
                const V3 q = xf_point_lr(graphFromRender, pS);
                int node = 0;
                float sum = 0.f;
                const int inRange = graph::index_coverage(ix, q.x, q.y, q.z, buf, &node, &sum);
                r.node += node;
                r.search += inRange > 0 ? 1 : 0;
                r.in_range += inRange;
                r.range = r.range + (double)sum;
                if (detail) detail[(size_t)id * (size_t)maxDepth + (size_t)k] = {pS.x, pS.y, pS.z, node, inRange, sum};
            });
        }
        rec[id] = r;
    }
    flush_stat(P.stats, 3, nLookup);
    flush_stat(P.stats, 4, nIn);
    flush_stat(P.stats, 6, nSteps);
}

// The pass's records added to the per-pixel sums, one lane per pixel, in sample-index order:
// a sample range split into passes or calls gives the same bits
__global__ void __launch_bounds__(256) k_graph_analyze_reduce(int pixels, int samples,
                                                              const graph::AnalyzeRec *__restrict__ rec,
                                                              graph::AnalyzeAcc *__restrict__ acc) {
    for (int pix = blockIdx.x * blockDim.x + threadIdx.x; pix < pixels; pix += gridDim.x * blockDim.x) {
        graph::AnalyzeAcc a = acc[pix];
        for (int s = 0; s < samples; ++s) {
            const graph::AnalyzeRec r = rec[(size_t)s * (size_t)pixels + (size_t)pix];
            a.total += (unsigned long long)r.total;
            a.node += (unsigned long long)r.node;
            a.search += (unsigned long long)r.search;
            a.in_range += (unsigned long long)r.in_range;
            a.range = a.range + r.range;
        }
        acc[pix] = a;
    }
}

// merge_step's states in device memory: relaxed atomics at agent scope, so that a sweep sees
// what other lanes of the same launch have already decided (a stale read only costs a round)
struct MergeStateDev {
    int *s;
    __device__ __forceinline__ int load(int i) const {
        return __hip_atomic_load(s + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void store(int i, int v) {
        __hip_atomic_store(s + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// One round of the vertex merge (avr_graph_merge.h): one lane per unfinalised point, work[0 ..
// nwork) in cell order, AVR_MERGE_SWEEPS steps at most per point (a fixed number: later steps
// see what the wave's own lanes and its neighbours decided in the earlier ones). No lane
// waits: a point that cannot be finalised yet goes to next[], appended with one atomic per
// wave on *nleft, which is also the count the host reads. Measured with 4 steps
// (tools/graph_merge_profile.py, radius modifier 20): 93 rounds for 166, 63.0 ms for 64.9 ms
// of rounds: the time is the early rounds' scans, not the number of rounds, so 1 stays.
#ifndef AVR_MERGE_SWEEPS
#define AVR_MERGE_SWEEPS 1
#endif
__global__ void __launch_bounds__(256) k_graph_merge_round(graph::MergeView mv, int *state, const int *__restrict__ work,
                                                           int nwork, int *__restrict__ next, int *__restrict__ nleft) {
    MergeStateDev st{state};
    for (long long base = blockIdx.x * 256ll; base < nwork; base += gridDim.x * 256ll) {
        const long long idx = base + threadIdx.x;
        const int i = idx < nwork ? work[idx] : -1;
        bool left = i >= 0;
        for (int sweep = 0; sweep < AVR_MERGE_SWEEPS && left; ++sweep) left = !graph::merge_step(mv, i, st);
        const unsigned long long m = __ballot(left);
        if (m == 0) continue;
        const int lane = __lane_id(), leader = __ffsll(m) - 1;
        int b = 0;
        if (lane == leader) b = atomicAdd(nleft, __popcll(m));
        b = __shfl(b, leader);
        if (left) next[b + __popcll(m & ((1ull << lane) - 1ull))] = i;
    }
}

// The same round with one wave per point, for the rounds with few points left, where a round
// lasts as long as one lane's scan: the wave's lanes share the scan (consecutive records,
// coalesced), join their parts by butterfly, and lane 0 decides and appends.
__global__ void __launch_bounds__(256) k_graph_merge_round_wave(graph::MergeView mv, int *state,
                                                                const int *__restrict__ work, int nwork,
                                                                int *__restrict__ next, int *__restrict__ nleft) {
    MergeStateDev st{state};
    const int lane = __lane_id();
    for (long long w = (blockIdx.x * 256ll + threadIdx.x) >> 6; w < nwork; w += (gridDim.x * 256ll) >> 6) {
        const int i = work[w];
        const int cur = __shfl(st.load(i), 0);   // one value for the wave
        if (cur >= 0) continue;
        const graph::MergeRec q = mv.ent[mv.v0 + i];
        graph::MergeScan r = graph::merge_scan(mv, mv.v0 + i, q, st, lane, 64);
        for (int off = 32; off > 0; off >>= 1) {
            graph::MergeScan o;
            o.best = __shfl_xor(r.best, off);
            o.open = __shfl_xor(r.open, off);
            o.bestD = __shfl_xor(r.bestD, off);
            o.openD = __shfl_xor(r.openD, off);
            graph::merge_scan_join(&r, o);
        }
        if (lane == 0 && !graph::merge_decide(mv, i, cur, q, r, st)) next[atomicAdd(nleft, 1)] = i;
    }
}

// The id scan over the final states, 64 points per wave: mask[w] = which of them are new
// vertices (state == own seq), cnt[w] = how many ...
__global__ void __launch_bounds__(256) k_graph_merge_flags(int v0, int n, const int *__restrict__ state,
                                                           unsigned long long *__restrict__ mask, int *__restrict__ cnt) {
    const long long lanes = ((long long)n + 63) / 64 * 64;
    for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < lanes; idx += gridDim.x * 256ll) {
        const bool isNew = idx < n && state[idx] == v0 + (int)idx;
        const unsigned long long m = __ballot(isNew);
        if (__lane_id() == 0) {
            mask[idx >> 6] = m;
            cnt[idx >> 6] = __popcll(m);
        }
    }
}

// ... cnt[] to its exclusive prefix sum in place (one block: a run of waves per lane, the 256
// run sums scanned in LDS), *total = the new vertices ...
__global__ void __launch_bounds__(256) k_graph_merge_scan(int nw, int *__restrict__ cnt, int *__restrict__ total) {
    __shared__ int s_part[256];
    const int per = (nw + 255) / 256, t = threadIdx.x;
    const int a = min(t * per, nw), b = min(a + per, nw);
    int sum = 0;
    for (int j = a; j < b; ++j) sum += cnt[j];
    s_part[t] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = t >= off ? s_part[t - off] : 0;
        __syncthreads();
        s_part[t] += v;
        __syncthreads();
    }
    int run = s_part[t] - sum;
    for (int j = a; j < b; ++j) {
        const int c = cnt[j];
        cnt[j] = run;
        run += c;
    }
    if (t == 255) *total = s_part[255];
}

// ... and vertex_of_point: an existing vertex's id as it is, a new point's V0 + its rank
__global__ void __launch_bounds__(256) k_graph_merge_ids(int v0, int n, const int *__restrict__ state,
                                                         const unsigned long long *__restrict__ mask,
                                                         const int *__restrict__ woff, int *__restrict__ ids) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        int t = state[i];
        if (t >= v0) {
            const int j = t - v0;
            t = v0 + woff[j >> 6] + __popcll(mask[j >> 6] & ((1ull << (j & 63)) - 1ull));
        }
        ids[i] = t;
    }
}

// VoxelBoundary::CaptureBoundary (voxels/voxel_boundary.cpp:13-62), one lane per ray: ray r of
// bundle b is (i, j) in [-S, S]^2, i outer; p = (origin_b + xv_b * (float)i) + yv_b * (float)j;
// GetHits(primitive) along dir_b: a miss captures nothing, and neither does a start inside the
// primitive (the reference skips to the exit hit, beyond which no medium lies); a ray from
// outside moves to its entry (SkipIntersection, no offset). Then GridMedium::SampleRay with the
// direction as given (not normalised: the segment bounds are in its units) and tMax = Infinity;
// the first segment with sigma_t[0] * majorant != 0 (sigma at sample_visible(0), k_graph_walks'
// defaultLambda) gives out[ray] = {p + dir_b * segMin, 1}; {0, 0, 0, 0} without one.
template <int kGeom>
__global__ void __launch_bounds__(256) k_graph_capture(DevMedium m, long long nRays, int S, const float *__restrict__ origin,
                                                       const float *__restrict__ dir, const float *__restrict__ xvec,
                                                       const float *__restrict__ yvec, float4 *__restrict__ out,
                                                       int *__restrict__ nCaptured) {
    __shared__ float s_maj[4096];
    const float *maj = stage_majorant(m, s_maj);
    const LambdaIdx li = lambda_index(sample_visible(0.f).l);
    const float sigma_t0 = (sample_table(m.sigma_a, li) + sample_table(m.sigma_s, li)).v0;
    const int side = 2 * S + 1;
    const long long per = (long long)side * side;
    const long long lanes = (nRays + 63) / 64 * 64;   // whole waves reach the ballot
    for (long long ray = blockIdx.x * (long long)blockDim.x + threadIdx.x; ray < lanes;
         ray += (long long)gridDim.x * blockDim.x) {
        bool captured = false;
        if (ray < nRays) {
            const long long b = ray / per;
            const int r = (int)(ray - b * per), i = r / side - S, j = r - (r / side) * side - S;
            const V3 o = {origin[3 * b], origin[3 * b + 1], origin[3 * b + 2]}, d = {dir[3 * b], dir[3 * b + 1], dir[3 * b + 2]};
            const V3 xv = {xvec[3 * b], xvec[3 * b + 1], xvec[3 * b + 2]}, yv = {yvec[3 * b], yvec[3 * b + 1], yvec[3 * b + 2]};
            V3 p = (o + xv * (float)i) + yv * (float)j;
            float4 res = make_float4(0.f, 0.f, 0.f, 0.f);
            const graph::Hits h = graph::primitive_hits<kGeom>(m, p, d);
            if (h.type == graph::kOutsideTwoHits) p = p + d * h.t0;
            // a grid point or an entry that overflowed captures nothing (the host checks the bundle)
            const bool finite = __builtin_isfinite(p.x) && __builtin_isfinite(p.y) && __builtin_isfinite(p.z);
            if (h.type == graph::kOutsideTwoHits && finite) {
                Dda it;
                dda_init(it, m, Ray{p, d}, kInf);
                float segMin, segMax, mv;
                while (dda_next(it, maj, m.mres, &segMin, &segMax, &mv)) {
                    if (sigma_t0 * mv != 0) {
                        const V3 q = p + d * segMin;
                        res = make_float4(q.x, q.y, q.z, 1.f);
                        captured = true;
                        break;
                    }
                }
            }
            out[ray] = res;
        }
        const unsigned long long mask = __ballot(captured);
        if (mask != 0 && __lane_id() == 0) atomicAdd(nCaptured, __popcll(mask));
    }
}

// FreeGraph::ToUniform's vertices (Uniform::FromPoints, reduce 0) for n points on the device,
// first pass: the point's voxel key goes into the set keys[0 .. mask] (empty = all ones, slot =
// MixBits(key) & mask, linear probing; capacity at least 2 n, so a free slot exists), and
// first[slot] keeps the lowest index of the key's points, which makes the result independent
// of scheduling. slot_of[i] = the key's slot; *bad = the lowest index with an invalid coordinate.
__global__ void __launch_bounds__(256) k_graph_uniform_insert(long long n, const float *__restrict__ xyz, float spacing,
                                                              unsigned long long *keys, uint32_t mask, int *first,
                                                              int *__restrict__ slot_of, int *bad) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += gridDim.x * 256ll) {
        int c[3];
        if (!graph::uniform_coors(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], spacing, c)) {
            atomicMin(bad, (int)i);
            slot_of[i] = -1;
            continue;
        }
        const unsigned long long key = graph::uniform_key(c[0], c[1], c[2]);
        uint32_t slot = (uint32_t)graph::uniform_mix(key) & mask;
        int found = -1;
        for (uint32_t probe = 0; probe <= mask; ++probe) {
            const unsigned long long old = atomicCAS(keys + slot, graph::kUniformEmpty, key);
            if (old == graph::kUniformEmpty || old == key) {
                found = (int)slot;
                break;
            }
            slot = (slot + 1) & mask;
        }
        if (found >= 0) atomicMin(first + found, (int)i);
        slot_of[i] = found;
    }
}

// Second pass: state[i] = the first point of i's voxel (i itself: a new vertex; the form
// k_graph_merge_flags / _ids read with v0 = 0), *count += the new vertices
__global__ void __launch_bounds__(256) k_graph_uniform_first(long long n, const int *__restrict__ first,
                                                             const int *__restrict__ slot_of, int *__restrict__ state,
                                                             int *count) {
    const long long lanes = (n + 63) / 64 * 64;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < lanes; i += gridDim.x * 256ll) {
        bool isNew = false;
        if (i < n) {
            const int s = slot_of[i];
            const int f = s >= 0 ? first[s] : -1;
            state[i] = f;
            isNew = f == (int)i;
        }
        const unsigned long long m = __ballot(isNew);
        if (m != 0 && __lane_id() == 0) atomicAdd(count, __popcll(m));
    }
}

// The floods' state in device memory: four cells per 32-bit word, bits ored in with relaxed
// atomics at agent scope (a stale read only costs an atomic; the or's old value decides)
struct VoxelStateDev {
    unsigned *w;
    __device__ __forceinline__ unsigned bits(int cell) const {
        return (__hip_atomic_load(w + (cell >> 2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> ((cell & 3) * 8)) & 0xffu;
    }
    __device__ __forceinline__ bool set(int cell, unsigned bit) {
        const unsigned m = bit << ((cell & 3) * 8);
        return !(atomicOr(w + (cell >> 2), m) & m);
    }
};

// One level of a flood (avr_graph_voxels.h), kFill 0 the single layer's, 1 the fill's: one lane
// per cell of frontier[0 .. nFront); a neighbour joins next[] once, where its bit was first set
// (each cell at most once over the whole flood, so next[] holds at most `cells` entries); one
// atomic per wave and neighbour direction on *nNext, which the host reads to launch the next level.
template <int kFill>
__global__ void __launch_bounds__(256) k_graph_voxels_level(graph::VoxelDims d, unsigned *state,
                                                            const int *__restrict__ frontier, int nFront,
                                                            int *__restrict__ next, int *nNext) {
    VoxelStateDev st{state};
    for (long long idx = blockIdx.x * 256ll + threadIdx.x; idx < nFront; idx += gridDim.x * 256ll) {
        const int cell = frontier[idx];
        auto push = [&](int nb, bool fresh) {
            const int slot = wave_push(nNext, fresh);
            if (fresh) next[slot] = nb;
        };
        if constexpr (kFill == 0) graph::voxel_visit_outside(d, st, cell, push);
        else graph::voxel_visit_fill(d, st, cell, push);
    }
}

}  // namespace avr
