// avr_graph_capi.hip — C-ABI of the lighting-graph precompute, the graph render and the analyzer
// (include/avr.h, "Lighting graph"), included at the end of avr_capi.hip (shares avr_context,
// fail(), HIP_TRY, the render calls' sampler setup and path state).
#include "avr_graph_host.h"

#include <atomic>
#include <chrono>

namespace {

// Params for the graph kernels: the context's medium plus the graph's sampler
int graph_params(avr_context *c, const avr_graph_sampling *s, unsigned long long maxIndex, int maxSampleIndex,
                 avr::Params *p) {
    if (!s) return fail(AVR_ERR_ARG, "null sampling");
    if (s->sampler != 0 && s->sampler != 1) return fail(AVR_ERR_ARG, "sampler must be 0 (independent) or 1 (zsobol)");
    if (s->resolution_x <= 0) return fail(AVR_ERR_ARG, "resolution_x must be positive");
    *p = avr::Params{};
    p->med = c->med;
    p->stats = c->d_stats.get();
    p->seed = s->seed;
    p->sampler_kind = s->sampler;
    if (s->sampler == 1) {
        if (s->samples_per_pixel <= 0 || s->film_width <= 0 || s->film_height <= 0)
            return fail(AVR_ERR_ARG, "zsobol: samples_per_pixel and film resolution required");
        avr::smp::ZSobolParams zs = avr::smp::zsobol_params(s->samples_per_pixel, s->film_width, s->film_height, s->seed);
        if (zs.nBase4Digits > 16) return fail(AVR_ERR_ARG, "zsobol: film resolution x spp beyond 2^32 sample indices");
        // (Morton(pixel) << log2(spp)) | sampleIndex must fit 32 bits (the device's ZSobol index)
        const unsigned long long yMax = maxIndex / (unsigned long long)s->resolution_x;
        const unsigned long long xMax = std::min<unsigned long long>(maxIndex, (unsigned long long)s->resolution_x - 1);
        int bits = 0;
        while ((1ull << bits) <= std::max(xMax, yMax)) ++bits;
        int sbits = 0;
        while ((1ll << sbits) <= (long long)maxSampleIndex) ++sbits;
        if (2 * bits + std::max(zs.log2spp, sbits) > 32)
            return fail(AVR_ERR_ARG, "zsobol: graph sampling indices beyond the 2^32 Sobol' index range");
        p->zs = zs;
    }
    return AVR_OK;
}

// The kernels' geometry instantiation (avr_graph_set_geometry): the interface one only for a
// context that has an interface; without one geometry 1 is the bounds box, geometry 0's code
bool graph_interface(const avr_context *c) { return c->graph_geometry == 1 && c->med.boundary != 0; }

// kernel<zsobol, geometry> / kernel<geometry> on the context's stream, 256 lanes per block
#define AVR_GRAPH_LAUNCH_ZG(kernel, zs, geom, blocks, ...)                                                        \
    do {                                                                                                           \
        if (zs) {                                                                                                  \
            if (geom) hipLaunchKernelGGL((kernel<true, 1>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);   \
            else hipLaunchKernelGGL((kernel<true, 0>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);        \
        } else {                                                                                                   \
            if (geom) hipLaunchKernelGGL((kernel<false, 1>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);  \
            else hipLaunchKernelGGL((kernel<false, 0>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);       \
        }                                                                                                          \
    } while (0)
// kernel<zsobol, geometry, view> with a constant view
#define AVR_GRAPH_LAUNCH_ZGV(kernel, zs, geom, view, blocks, ...)                                                      \
    do {                                                                                                                \
        if (zs) {                                                                                                       \
            if (geom) hipLaunchKernelGGL((kernel<true, 1, view>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);  \
            else hipLaunchKernelGGL((kernel<true, 0, view>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);       \
        } else {                                                                                                        \
            if (geom) hipLaunchKernelGGL((kernel<false, 1, view>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__); \
            else hipLaunchKernelGGL((kernel<false, 0, view>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);      \
        }                                                                                                               \
    } while (0)
#define AVR_GRAPH_LAUNCH_G(kernel, geom, blocks, ...)                                                     \
    do {                                                                                                   \
        if (geom) hipLaunchKernelGGL((kernel<1>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);     \
        else hipLaunchKernelGGL((kernel<0>), dim3(blocks), dim3(256), 0, c->stream, __VA_ARGS__);          \
    } while (0)

}  // namespace

// The host vertex index (avr_graph_index.h) and the id its device copies are cached under
struct avr_graph_index {
    avr::graph::Index ix;
    unsigned long long uid = 0;
};

namespace {

std::atomic<unsigned long long> g_index_uid{0};

// The context's device copy of `idx` (c->gidx), uploaded on first use and replaced when
// another index is used: records | ids | cell offsets | squared ranges in one allocation.
int ensure_graph_index(avr_context *c, const avr_graph_index *idx) {
    if (c->gidx_uid == idx->uid) return AVR_OK;
    // queued kernels may still read the previous copy
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_gidx.reset();
    c->gidx_uid = 0;
    const avr::graph::IndexView h = idx->ix.View();
    const size_t n = idx->ix.NumVertices(), cells = idx->ix.NumCells();
    auto pad = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t szRec = pad(n * sizeof(avr::graph::IndexRec)), szId = pad(n * sizeof(int));
    const size_t szStart = pad((cells + 1) * sizeof(int)), szRange = h.range2 ? pad(n * sizeof(float)) : 0;
    Buffer<char> buf;   // the context's only once every part is there
    HIP_TRY(buf.alloc(szRec + szId + szStart + szRange));
    char *d = buf.get();
    HIP_TRY(hipMemcpy(d, h.rec, n * sizeof(avr::graph::IndexRec), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + szRec, h.id, n * sizeof(int), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d + szRec + szId, h.cell_start, (cells + 1) * sizeof(int), hipMemcpyHostToDevice));
    if (h.range2) HIP_TRY(hipMemcpy(d + szRec + szId + szStart, h.range2, n * sizeof(float), hipMemcpyHostToDevice));
    c->d_gidx = std::move(buf);
    c->gidx = h;
    c->gidx.rec = (const avr::graph::IndexRec *)d;
    c->gidx.id = (const int *)(d + szRec);
    c->gidx.cell_start = (const int *)(d + szRec + szId);
    c->gidx.range2 = h.range2 ? (const float *)(d + szRec + szId + szStart) : nullptr;
    c->gidx_uid = idx->uid;
    return AVR_OK;
}

}  // namespace

// The host uniform graph (avr_graph_uniform.h) and the id its device copy is cached under
struct avr_graph_uniform {
    avr::graph::Uniform u;
    unsigned long long uid = 0;
};

namespace {

// The context's device copy of `u`'s table (c->guni), uploaded on first use and replaced when
// another uniform graph is used; the ids come from the counter the vertex indices use
int ensure_graph_uniform(avr_context *c, const avr_graph_uniform *u) {
    if (c->guni_uid == u->uid) return AVR_OK;
    // queued kernels may still read the previous copy
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->d_guni.reset();
    c->guni_uid = 0;
    const avr::graph::UniformView h = u->u.View();
    const size_t cap = u->u.Capacity();
    Buffer<avr::graph::UniformEntry> tab;   // the context's only once it is filled
    HIP_TRY(tab.alloc(cap));
    HIP_TRY(hipMemcpy(tab.get(), h.tab, cap * sizeof(avr::graph::UniformEntry), hipMemcpyHostToDevice));
    c->d_guni = std::move(tab);
    c->guni = h;
    c->guni.tab = c->d_guni.get();
    c->guni_uid = u->uid;
    return AVR_OK;
}

}  // namespace

extern "C" {

int avr_graph_set_geometry(avr_context *c, int geometry) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    if (geometry != 0 && geometry != 1) return fail(AVR_ERR_ARG, "graph geometry must be 0 (bounds box) or 1 (interface)");
    c->graph_geometry = geometry;
    return AVR_OK;
}

int avr_graph_start_rays(avr_context *c, const float bounds_center[3], float max_dist_to_center, const float in_dir[3],
                         int steps, int *type, float *o, float *t_first) {
    if (!c || steps < 0 || steps > 32768) return fail(AVR_ERR_ARG, "bad start ray arguments");
    if (!c->has_medium) return fail(AVR_ERR_STATE, "medium required");
    if (steps == 0) return AVR_OK;
    if (!bounds_center || !in_dir || !type || !o || !t_first) return fail(AVR_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    const long long n = (long long)steps * steps;
    Arena<> scratch(c->stream);
    const auto rTy = scratch.reserve<int>((size_t)n);
    const auto rT = scratch.reserve<float>((size_t)n), rO = scratch.reserve<float>(3 * (size_t)n);
    HIP_TRY(scratch.commit());
    int *dTy = scratch.get(rTy);
    float *dT = scratch.get(rT), *dO = scratch.get(rO);
    const avr::V3 ctr = {bounds_center[0], bounds_center[1], bounds_center[2]}, dir = {in_dir[0], in_dir[1], in_dir[2]};
    AVR_GRAPH_LAUNCH_G(avr::k_graph_start_rays, graph_interface(c), blocks_for(n, 256, 256 * 64), c->med, ctr,
                       max_dist_to_center, dir, steps, dTy, dO, dT);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(type, dTy, rTy.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(o, dO, rO.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(t_first, dT, rT.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_walks(avr_context *c, const avr_graph_sampling *s, long long n_rays, const float *o, const float *d,
                    const float *t_first, const long long *index0, int iterations, int sample_index, int max_depth,
                    float *points, int *counts) {
    return avr_graph_walks_from(c, s, n_rays, o, d, t_first, index0, iterations, sample_index, 0, max_depth, points,
                                counts);
}

int avr_graph_walks_from(avr_context *c, const avr_graph_sampling *s, long long n_rays, const float *o, const float *d,
                         const float *t_first, const long long *index0, int iterations, int sample_index,
                         int skip_dims, int max_depth, float *points, int *counts) {
    if (!c || n_rays < 0 || iterations < 0 || max_depth < 0 || skip_dims < 0)
        return fail(AVR_ERR_ARG, "bad walk arguments");
    if (!c->has_medium) return fail(AVR_ERR_STATE, "medium required");
    const long long nPaths = n_rays * (long long)iterations;
    if (nPaths == 0) return AVR_OK;
    if (!o || !d || !t_first || !index0 || !counts || (max_depth > 0 && !points)) return fail(AVR_ERR_ARG, "null buffer");
    long long maxIdx = 0;
    for (long long r = 0; r < n_rays; ++r) {
        if (index0[r] < 0) return fail(AVR_ERR_ARG, "negative sampling index");
        maxIdx = std::max(maxIdx, index0[r] + iterations - 1);
    }
    avr::Params p;
    int rc = graph_params(c, s, (unsigned long long)maxIdx, sample_index, &p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const int md = std::max(max_depth, 1);
    const size_t nR = (size_t)n_rays, nP = (size_t)nPaths;
    Arena<> scratch(c->stream);
    const auto rO = scratch.reserve<float>(3 * nR), rD = scratch.reserve<float>(3 * nR), rT = scratch.reserve<float>(nR);
    const auto rI = scratch.reserve<long long>(nR);
    const auto rP = scratch.reserve<float>(nP * md * 3);
    const auto rC = scratch.reserve<int>(nP);
    HIP_TRY(scratch.commit());
    float *dO = scratch.get(rO), *dD = scratch.get(rD), *dT = scratch.get(rT), *dP = scratch.get(rP);
    long long *dI = scratch.get(rI);
    int *dC = scratch.get(rC);
    HIP_TRY(hipMemcpyAsync(dO, o, rO.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dD, d, rD.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dT, t_first, rT.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dI, index0, rI.bytes(), hipMemcpyHostToDevice, c->stream));
    const int blocks = blocks_for(nPaths, 256, 256 * 64);
    AVR_GRAPH_LAUNCH_ZG(avr::k_graph_walks, p.sampler_kind == 1, graph_interface(c), blocks, p, nPaths, iterations, dO, dD,
                        dT, dI, sample_index, skip_dims, s->resolution_x, max_depth, dP, dC);
    HIP_TRY(hipGetLastError());
    if (max_depth > 0) HIP_TRY(hipMemcpyAsync(points, dP, rP.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(counts, dC, rC.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_reinforce_rays(avr_context *c, const avr_graph_sampling *s, int n, const int *vertex_ids,
                             const float *points, float vertex_radius, int n_rays, int cycle, float *o, float *d,
                             float *t_first, int *valid) {
    if (!c || n < 0 || n_rays < 0 || cycle < 0 || !(vertex_radius > 0)) return fail(AVR_ERR_ARG, "bad reinforce arguments");
    if (!c->has_medium) return fail(AVR_ERR_STATE, "medium required");
    const long long nr = (long long)n * n_rays;
    if (nr == 0) return AVR_OK;
    if (!vertex_ids || !points || !o || !d || !t_first || !valid) return fail(AVR_ERR_ARG, "null buffer");
    long long maxId = 0;
    for (int i = 0; i < n; ++i) {
        if (vertex_ids[i] < 0) return fail(AVR_ERR_ARG, "negative vertex id");
        maxId = std::max<long long>(maxId, vertex_ids[i]);
    }
    avr::Params p;
    int rc = graph_params(c, s, (unsigned long long)(maxId + 1) * (unsigned long long)n_rays, cycle, &p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    Arena<> scratch(c->stream);
    const auto rId = scratch.reserve<int>((size_t)n);
    const auto rPt = scratch.reserve<float>(3 * (size_t)n);
    const auto rO = scratch.reserve<float>(3 * (size_t)nr), rD = scratch.reserve<float>(3 * (size_t)nr);
    const auto rT = scratch.reserve<float>((size_t)nr);
    const auto rV = scratch.reserve<int>((size_t)nr);
    HIP_TRY(scratch.commit());
    int *dId = scratch.get(rId), *dV = scratch.get(rV);
    float *dPt = scratch.get(rPt), *dO = scratch.get(rO), *dD = scratch.get(rD), *dT = scratch.get(rT);
    HIP_TRY(hipMemcpyAsync(dId, vertex_ids, rId.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dPt, points, rPt.bytes(), hipMemcpyHostToDevice, c->stream));
    AVR_GRAPH_LAUNCH_ZG(avr::k_graph_reinforce_rays, p.sampler_kind == 1, graph_interface(c), (n + 255) / 256, p, n, dId,
                        dPt, vertex_radius, n_rays, cycle, s->resolution_x, dO, dD, dT, dV);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o, dO, rO.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(d, dD, rD.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(t_first, dT, rT.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(valid, dV, rV.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_light(avr_context *c, const avr_graph_sampling *s, int n_vertices, const float *vertices,
                    const float in_dir[3], float sphere_radius, int points_on_radius, int iterations,
                    float max_dist_to_center, float *light) {
    if (!c || n_vertices < 0 || points_on_radius < 0 || iterations < 0) return fail(AVR_ERR_ARG, "bad light arguments");
    if (!c->has_medium) return fail(AVR_ERR_STATE, "medium required");
    if (n_vertices == 0) return AVR_OK;
    if (!vertices || !in_dir || !light) return fail(AVR_ERR_ARG, "null buffer");
    if (iterations < 1) return fail(AVR_ERR_ARG, "Must have at least one light ray iteration");   // :10-11
    const int maxPts = (2 * points_on_radius + 1) * (2 * points_on_radius + 1);
    avr::Params p;
    int rc = graph_params(c, s, (unsigned long long)n_vertices * (unsigned long long)maxPts, iterations - 1, &p);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // tr scratch: at most 2^28 estimates per chunk of vertices (1 GiB)
    const long long perV = (long long)maxPts * iterations;
    const int chunk = (int)std::max<long long>(1, std::min<long long>(n_vertices, (1ll << 28) / perV));
    Arena<> scratch(c->stream);
    const auto rV = scratch.reserve<float>((size_t)n_vertices * 3), rL = scratch.reserve<float>((size_t)n_vertices);
    const auto rRec = scratch.reserve<avr::graph::DiskRec>((size_t)n_vertices * maxPts);
    const auto rN = scratch.reserve<int>((size_t)n_vertices);
    const auto rTr = scratch.reserve<float>((size_t)chunk * perV);
    HIP_TRY(scratch.commit());
    float *dV = scratch.get(rV), *dL = scratch.get(rL), *dTr = scratch.get(rTr);
    avr::graph::DiskRec *dRec = scratch.get(rRec);
    int *dN = scratch.get(rN);
    HIP_TRY(hipMemcpyAsync(dV, vertices, rV.bytes(), hipMemcpyHostToDevice, c->stream));
    const avr::V3 dir = {in_dir[0], in_dir[1], in_dir[2]};
    AVR_GRAPH_LAUNCH_G(avr::k_graph_disk, graph_interface(c), (n_vertices + 255) / 256, c->med, n_vertices, dV, dir,
                       sphere_radius, points_on_radius, max_dist_to_center, maxPts, dRec, dN);
    HIP_TRY(hipGetLastError());
    for (int v0 = 0; v0 < n_vertices; v0 += chunk) {
        const int nv = std::min(chunk, n_vertices - v0);
        const long long n = (long long)nv * perV;
        const int blocks = blocks_for(n, 256, 256 * 64);
        if (p.sampler_kind == 1)
            hipLaunchKernelGGL(avr::k_graph_tr<true>, dim3(blocks), dim3(256), 0, c->stream, p, v0, nv, maxPts, iterations,
                               dir, s->resolution_x, dRec, dN, dTr);
        else
            hipLaunchKernelGGL(avr::k_graph_tr<false>, dim3(blocks), dim3(256), 0, c->stream, p, v0, nv, maxPts, iterations,
                               dir, s->resolution_x, dRec, dN, dTr);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(avr::k_graph_average, dim3((nv + 255) / 256), dim3(256), 0, c->stream, v0, nv, maxPts,
                           iterations, dRec, dN, dTr, dL);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(light, dL, rL.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_propagate_device(avr_context *c, int n, long long nnz, const int *row_ptr, const int *col,
                               const float *val, const float *light, int bounces, float *total, int *iterations) {
    if (!c || n < 0 || nnz < 0 || bounces < 0) return fail(AVR_ERR_ARG, "bad propagate arguments");
    if (n == 0) { if (iterations) *iterations = bounces; return AVR_OK; }
    if (!row_ptr || !light || !total || (nnz > 0 && (!col || !val))) return fail(AVR_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    // (the scratch is freed after the stream drains: the caller's `total` is complete then)
    Arena<> scratch(c->stream);
    const auto rCur = scratch.reserve<float>((size_t)n), rNext = scratch.reserve<float>((size_t)n);
    const auto rFlags = scratch.reserve<int>((size_t)std::max(bounces, 1));
    HIP_TRY(scratch.commit());
    float *cur = scratch.get(rCur), *next = scratch.get(rNext);
    int *flags = scratch.get(rFlags);
    HIP_TRY(hipMemsetAsync(flags, 0, sizeof(int) * std::max(bounces, 1), c->stream));
    HIP_TRY(hipMemcpyAsync(total, light, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(cur, light, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    const int blocks = blocks_for(n, 256, 256 * 64);
    for (int it = 0; it < bounces; ++it) {
        hipLaunchKernelGGL(avr::k_graph_spmv, dim3(blocks), dim3(256), 0, c->stream, n, row_ptr, col, val, cur, next,
                           total, flags, it);
        HIP_TRY(hipGetLastError());
        std::swap(cur, next);
    }
    if (bounces > 0) {
        hipLaunchKernelGGL(avr::k_graph_accumulate, dim3(blocks), dim3(256), 0, c->stream, n, cur, total, flags, bounces);
        HIP_TRY(hipGetLastError());
    }
    if (iterations) {
        std::vector<int> h(std::max(bounces, 1));
        HIP_TRY(hipMemcpyAsync(h.data(), flags, sizeof(int) * h.size(), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        int done = bounces;
        for (int j = 0; j < bounces; ++j)
            if (h[j]) { done = j; break; }
        *iterations = done;
    }
    return AVR_OK;
}

int avr_graph_propagate(avr_context *c, int n, const int *row_ptr, const int *col, const float *val,
                        const float *light, int bounces, float *total, int *iterations) {
    if (!c || n < 0 || bounces < 0) return fail(AVR_ERR_ARG, "bad propagate arguments");
    if (n == 0) { if (iterations) *iterations = bounces; return AVR_OK; }
    if (!row_ptr || !light || !total) return fail(AVR_ERR_ARG, "null buffer");
    const long long nnz = row_ptr[n];
    if (nnz < 0 || row_ptr[0] != 0) return fail(AVR_ERR_ARG, "bad row_ptr");
    for (int i = 0; i < n; ++i) {
        if (row_ptr[i + 1] < row_ptr[i]) return fail(AVR_ERR_ARG, "row_ptr not monotone");
        for (int k = row_ptr[i]; k < row_ptr[i + 1]; ++k) {
            if (col[k] < 0 || col[k] >= n) return fail(AVR_ERR_ARG, "column out of range");
            if (k > row_ptr[i] && col[k] <= col[k - 1]) return fail(AVR_ERR_ARG, "columns must ascend within a row");
        }
    }
    HIP_TRY(hipSetDevice(c->device));
    Arena<> scratch(c->stream);
    const auto rR = scratch.reserve<int>((size_t)n + 1), rC = scratch.reserve<int>((size_t)nnz);
    const auto rVal = scratch.reserve<float>((size_t)nnz), rL = scratch.reserve<float>((size_t)n);
    const auto rT = scratch.reserve<float>((size_t)n);
    HIP_TRY(scratch.commit());
    int *dR = scratch.get(rR), *dC = scratch.get(rC);
    float *dVal = scratch.get(rVal), *dL = scratch.get(rL), *dT = scratch.get(rT);
    HIP_TRY(hipMemcpyAsync(dR, row_ptr, rR.bytes(), hipMemcpyHostToDevice, c->stream));
    if (nnz) HIP_TRY(hipMemcpyAsync(dC, col, rC.bytes(), hipMemcpyHostToDevice, c->stream));
    if (nnz) HIP_TRY(hipMemcpyAsync(dVal, val, rVal.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dL, light, rL.bytes(), hipMemcpyHostToDevice, c->stream));
    const int rc = avr_graph_propagate_device(c, n, nnz, dR, dC, dVal, dL, bounces, dT, iterations);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(total, dT, rT.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

struct avr_graph {
    avr::graph::Builder b;
    explicit avr_graph(float r) : b(r) {}
};

int avr_graph_create(float vertex_radius, avr_graph **out) {
    if (!out || !(vertex_radius > 0)) return fail(AVR_ERR_ARG, "vertex radius must be positive");
    *out = new avr_graph(vertex_radius);
    return AVR_OK;
}
int avr_graph_destroy(avr_graph *g) {
    delete g;
    return AVR_OK;
}
int avr_graph_add_walks(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts) {
    if (!g || n_walks < 0 || max_depth < 0) return fail(AVR_ERR_ARG, "bad walks");
    if (n_walks > 0 && (!counts || (max_depth > 0 && !points))) return fail(AVR_ERR_ARG, "null buffer");
    for (long long w = 0; w < n_walks; ++w) {
        const int k = counts[w];
        if (k < 0 || k > max_depth) return fail(AVR_ERR_ARG, "walk count out of range");
        g->b.AddWalk(points + (size_t)w * max_depth * 3, k, k == max_depth);
    }
    return AVR_OK;
}
int avr_graph_add_walks_from(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                             const int *start_vertex) {
    if (!g || n_walks < 0 || max_depth < 0) return fail(AVR_ERR_ARG, "bad walks");
    if (n_walks > 0 && (!counts || !start_vertex || (max_depth > 0 && !points))) return fail(AVR_ERR_ARG, "null buffer");
    for (long long w = 0; w < n_walks; ++w) {
        const int k = counts[w], sv = start_vertex[w];
        if (k < 0 || k > max_depth) return fail(AVR_ERR_ARG, "walk count out of range");
        if (sv < -1 || sv >= (long long)g->b.NumVertices()) return fail(AVR_ERR_ARG, "start vertex out of range");
        // with a starting vertex the path holds one vertex before the first scatter, so the
        // walk was traced with max_depth - 1 scatters
        const int cap = sv >= 0 ? max_depth - 1 : max_depth;
        if (k > cap) return fail(AVR_ERR_ARG, "walk count out of range");
        g->b.AddWalk(points + (size_t)w * max_depth * 3, k, k == cap, sv);
    }
    return AVR_OK;
}

}  // extern "C"

namespace {

// The walk arguments of the merge entries: counts and start vertices (NULL: none) in range as
// avr_graph_add_walks_from checks them; vertex_of_point is n_walks x max_depth
int merge_arguments(const avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                    const int *start_vertex, const int *vertex_of_point) {
    if (!g || n_walks < 0 || max_depth < 0) return fail(AVR_ERR_ARG, "bad walks");
    if (n_walks > 0 && (!counts || (max_depth > 0 && (!points || !vertex_of_point)))) return fail(AVR_ERR_ARG, "null buffer");
    for (long long w = 0; w < n_walks; ++w) {
        const int k = counts[w], sv = start_vertex ? start_vertex[w] : -1;
        if (k < 0 || k > max_depth) return fail(AVR_ERR_ARG, "walk count out of range");
        if (sv < -1 || sv >= (long long)g->b.NumVertices()) return fail(AVR_ERR_ARG, "start vertex out of range");
        if (k > (sv >= 0 ? max_depth - 1 : max_depth)) return fail(AVR_ERR_ARG, "walk count out of range");
    }
    return AVR_OK;
}

int merge_grid(const avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
               const int *start_vertex, avr::graph::MergeGrid *mg) {
    if (const char *msg = mg->Build(g->b.Radius(), g->b.NumVertices(), g->b.Vertices().data(), n_walks, max_depth, points,
                                    counts, start_vertex))
        return fail(AVR_ERR_ARG, msg);
    return AVR_OK;
}

// ids per point in seq order -> vertex_of_point (n_walks x max_depth, -1 past a walk's count)
void merge_scatter(const avr::graph::MergeGrid &mg, long long n_walks, int max_depth, const int *ids,
                   int *vertex_of_point) {
    const std::vector<int> &first = mg.WalkFirst();
    for (long long w = 0; w < n_walks; ++w) {
        const int k = first[(size_t)w + 1] - first[(size_t)w];
        int *row = vertex_of_point + (size_t)w * max_depth;
        for (int j = 0; j < max_depth; ++j) row[j] = j < k ? ids[first[(size_t)w] + j] : -1;
    }
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Rounds with at most this many open points run one wave per point (k_graph_merge_round_wave).
// Measured (tools/graph_merge_profile.py, radius modifier 20, 262 k points, ms of rounds): one
// lane per point throughout 82.2, one wave per point throughout 141.2, this threshold 64.9.
#ifndef AVR_MERGE_WAVE_BELOW
#define AVR_MERGE_WAVE_BELOW 32768
#endif
constexpr int kMergeWaveBelow = AVR_MERGE_WAVE_BELOW;

// The rounds and the id scan on the device over an uploaded copy of `mg`: ids per point in
// seq order. *ms_upload: the allocation and the upload, which the caller counts with the sort.
int merge_assign_device(avr_context *c, const avr::graph::MergeGrid &mg, std::vector<int> *ids, int *rounds,
                        int *new_vertices, double *ms_upload) {
    const avr::graph::MergeView h = mg.View();
    const int n = h.n;
    const size_t E = (size_t)h.v0 + (size_t)n, cells = mg.NumCells(), nw = ((size_t)n + 63) / 64;
    ids->assign((size_t)n, 0);
    *rounds = 0;
    *new_vertices = 0;
    *ms_upload = 0;
    if (n == 0) return AVR_OK;
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipSetDevice(c->device));
    constexpr int kCtr = 256;   // one counter per round, zeroed kCtr at a time; the last takes the scan's total
    Arena<> scratch(c->stream);
    const auto rRec = scratch.reserve<avr::graph::MergeRec>(E), rEnt = scratch.reserve<avr::graph::MergeRec>(E);
    const auto rMask = scratch.reserve<unsigned long long>(nw);
    const auto rStart = scratch.reserve<int>(cells + 1), rPrev = scratch.reserve<int>((size_t)n);
    const auto rState = scratch.reserve<int>((size_t)n);
    const auto rWork0 = scratch.reserve<int>((size_t)n), rWork1 = scratch.reserve<int>((size_t)n);
    const auto rIds = scratch.reserve<int>((size_t)n), rCnt = scratch.reserve<int>(nw), rCtr = scratch.reserve<int>(kCtr);
    HIP_TRY(scratch.commit());
    avr::graph::MergeRec *dRec = scratch.get(rRec), *dEnt = scratch.get(rEnt);
    unsigned long long *dMask = scratch.get(rMask);
    int *dStart = scratch.get(rStart), *dPrev = scratch.get(rPrev), *dState = scratch.get(rState);
    int *dWork[2] = {scratch.get(rWork0), scratch.get(rWork1)};
    int *dIds = scratch.get(rIds), *dCnt = scratch.get(rCnt), *dCtr = scratch.get(rCtr);
    HIP_TRY(hipMemcpyAsync(dRec, h.rec, E * sizeof(avr::graph::MergeRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dEnt, h.ent, E * sizeof(avr::graph::MergeRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dStart, h.cell_start, (cells + 1) * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dPrev, h.prev, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dWork[0], mg.Work().data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(dState, 0xff, (size_t)n * 4, c->stream));   // kMergeUndecided
    HIP_TRY(hipStreamSynchronize(c->stream));
    *ms_upload = ms_since(t0);
    avr::graph::MergeView dv = h;
    dv.rec = dRec;
    dv.ent = dEnt;
    dv.cell_start = dStart;
    dv.prev = dPrev;
    // one sweep per launch over the points still open; the host reads the count after each
    int left = n, r = 0, cur = 0;
    while (left > 0) {
        int now = 0;
        int *ctr = dCtr + r % (kCtr - 1);
        if (r % (kCtr - 1) == 0) HIP_TRY(hipMemsetAsync(dCtr, 0, kCtr * 4, c->stream));
        if (left <= kMergeWaveBelow)
            hipLaunchKernelGGL(avr::k_graph_merge_round_wave, dim3(blocks_for(left, 4, 256 * 64)), dim3(256), 0, c->stream,
                               dv, dState, dWork[cur], left, dWork[cur ^ 1], ctr);
        else
            hipLaunchKernelGGL(avr::k_graph_merge_round, dim3(blocks_for(left, 256, 256 * 64)), dim3(256), 0, c->stream, dv,
                               dState, dWork[cur], left, dWork[cur ^ 1], ctr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&now, ctr, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        ++r;
        // a round must finalise a point: never loop on a bug
        if (now < 0 || now >= left) return fail(AVR_ERR_INTERNAL, "graph merge: a round finalised no point");
        left = now;
        cur ^= 1;
    }
    int news = 0;
    hipLaunchKernelGGL(avr::k_graph_merge_flags, dim3(blocks_for(n, 256, 256 * 64)), dim3(256), 0, c->stream, h.v0, n,
                       dState, dMask, dCnt);
    hipLaunchKernelGGL(avr::k_graph_merge_scan, dim3(1), dim3(256), 0, c->stream, (int)nw, dCnt, dCtr + kCtr - 1);
    hipLaunchKernelGGL(avr::k_graph_merge_ids, dim3(blocks_for(n, 256, 256 * 64)), dim3(256), 0, c->stream, h.v0, n,
                       dState, dMask, dCnt, dIds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ids->data(), dIds, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&news, dCtr + kCtr - 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *rounds = r;
    *new_vertices = news;
    return AVR_OK;
}

// The ids of walk w's points: row w of vertex_of_point (first == null), or the compact ids in
// seq order from MergeGrid::WalkFirst
const int *merge_row(const int *ids, int max_depth, const int *first, long long w) {
    return first ? ids + first[w] : ids + (size_t)w * max_depth;
}

// Ids as avr_graph_add_walks_assigned takes them: every id at most the vertex count at its turn
int merge_ids_valid(const avr_graph *g, long long n_walks, int max_depth, const int *counts, const int *ids,
                    const int *first) {
    long long nv = (long long)g->b.NumVertices();
    for (long long w = 0; w < n_walks; ++w) {
        const int *row = merge_row(ids, max_depth, first, w);
        for (int j = 0; j < counts[w]; ++j) {
            if (row[j] < 0 || row[j] > nv) return fail(AVR_ERR_ARG, "vertex id out of range at its turn");
            nv += row[j] == nv;
        }
    }
    return AVR_OK;
}

void merge_replay(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                  const int *start_vertex, const int *ids, const int *first) {
    for (long long w = 0; w < n_walks; ++w) {
        const int k = counts[w], sv = start_vertex ? start_vertex[w] : -1;
        const int cap = sv >= 0 ? max_depth - 1 : max_depth;
        g->b.AddWalkAssigned(points + (size_t)w * max_depth * 3, merge_row(ids, max_depth, first, w), k, k == cap, sv);
    }
}

}  // namespace

extern "C" {

int avr_graph_merge_assign(const avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                           const int *start_vertex, int *vertex_of_point, int *rounds) {
    int rc = merge_arguments(g, n_walks, max_depth, points, counts, start_vertex, vertex_of_point);
    if (rc) return rc;
    avr::graph::MergeGrid mg;
    rc = merge_grid(g, n_walks, max_depth, points, counts, start_vertex, &mg);
    if (rc) return rc;
    std::vector<int> state, ids((size_t)mg.NumPoints());
    int r = 0;
    if (!mg.Assign(&state, &r)) return fail(AVR_ERR_INTERNAL, "graph merge: a round finalised no point");
    avr::graph::merge_ids(state.data(), mg.NumExisting(), mg.NumPoints(), ids.data());
    merge_scatter(mg, n_walks, max_depth, ids.data(), vertex_of_point);
    if (rounds) *rounds = r;
    return AVR_OK;
}

int avr_graph_merge_assign_device(avr_context *c, const avr_graph *g, long long n_walks, int max_depth,
                                  const float *points, const int *counts, const int *start_vertex, int *vertex_of_point,
                                  int *rounds) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    int rc = merge_arguments(g, n_walks, max_depth, points, counts, start_vertex, vertex_of_point);
    if (rc) return rc;
    avr::graph::MergeGrid mg;
    rc = merge_grid(g, n_walks, max_depth, points, counts, start_vertex, &mg);
    if (rc) return rc;
    std::vector<int> ids;
    int r = 0, news = 0;
    double msUp = 0;
    rc = merge_assign_device(c, mg, &ids, &r, &news, &msUp);
    if (rc) return rc;
    merge_scatter(mg, n_walks, max_depth, ids.data(), vertex_of_point);
    if (rounds) *rounds = r;
    return AVR_OK;
}

int avr_graph_add_walks_assigned(avr_graph *g, long long n_walks, int max_depth, const float *points, const int *counts,
                                 const int *start_vertex, const int *vertex_of_point) {
    int rc = merge_arguments(g, n_walks, max_depth, points, counts, start_vertex, vertex_of_point);
    if (rc) return rc;
    rc = merge_ids_valid(g, n_walks, max_depth, counts, vertex_of_point, nullptr);
    if (rc) return rc;
    merge_replay(g, n_walks, max_depth, points, counts, start_vertex, vertex_of_point, nullptr);
    return AVR_OK;
}

int avr_graph_add_walks_device(avr_context *c, avr_graph *g, long long n_walks, int max_depth, const float *points,
                               const int *counts, const int *start_vertex, avr_graph_merge_stats *stats) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    if (stats) *stats = avr_graph_merge_stats{};
    int dummy = 0;   // no vertex_of_point here: the replay takes the ids in seq order
    int rc = merge_arguments(g, n_walks, max_depth, points, counts, start_vertex, &dummy);
    if (rc) return rc;
    auto t0 = std::chrono::steady_clock::now();
    avr::graph::MergeGrid mg;
    rc = merge_grid(g, n_walks, max_depth, points, counts, start_vertex, &mg);
    if (rc) return rc;
    const double msGrid = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    std::vector<int> ids;
    int r = 0, news = 0;
    double msUp = 0;
    rc = merge_assign_device(c, mg, &ids, &r, &news, &msUp);
    if (rc) return rc;
    const double msDev = ms_since(t0);
    t0 = std::chrono::steady_clock::now();
    const int *first = mg.WalkFirst().data();
    rc = merge_ids_valid(g, n_walks, max_depth, counts, ids.data(), first);
    if (rc) return fail(AVR_ERR_INTERNAL, "graph merge: the device assignment is not a valid replay");
    merge_replay(g, n_walks, max_depth, points, counts, start_vertex, ids.data(), first);
    if (stats) {
        stats->rounds = r;
        stats->points = mg.NumPoints();
        stats->new_vertices = news;
        stats->ms_sort = msGrid + msUp;
        stats->ms_rounds = msDev - msUp;
        stats->ms_replay = ms_since(t0);
    }
    return AVR_OK;
}

int avr_graph_out_degrees(avr_graph *g, int *out) {
    if (!g || !out) return fail(AVR_ERR_ARG, "null buffer");
    g->b.OutDegrees(out);
    return AVR_OK;
}
int avr_graph_count_in_radius(avr_graph *g, int n, const int *vertex_ids, float radius, int *counts) {
    if (!g || n < 0 || !(radius > 0)) return fail(AVR_ERR_ARG, "bad radius query");
    if (n > 0 && (!vertex_ids || !counts)) return fail(AVR_ERR_ARG, "null buffer");
    for (int i = 0; i < n; ++i) {
        if (vertex_ids[i] < 0 || vertex_ids[i] >= (long long)g->b.NumVertices()) return fail(AVR_ERR_ARG, "vertex id");
        counts[i] = g->b.CountInRadius(vertex_ids[i], radius);
    }
    return AVR_OK;
}
int avr_graph_size(avr_graph *g, long long *n_vertices, long long *n_edges) {
    if (!g) return fail(AVR_ERR_ARG, "null graph");
    if (n_vertices) *n_vertices = (long long)g->b.NumVertices();
    if (n_edges) *n_edges = (long long)g->b.NumEdges();
    return AVR_OK;
}
int avr_graph_vertices(avr_graph *g, float *xyz, int *samples) {
    if (!g) return fail(AVR_ERR_ARG, "null graph");
    if (xyz) std::copy(g->b.Vertices().begin(), g->b.Vertices().end(), xyz);
    if (samples) std::copy(g->b.VertexSamples().begin(), g->b.VertexSamples().end(), samples);
    return AVR_OK;
}
int avr_graph_edges(avr_graph *g, int *from, int *to, int *samples) {
    if (!g) return fail(AVR_ERR_ARG, "null graph");
    if (from) std::copy(g->b.EdgeFrom().begin(), g->b.EdgeFrom().end(), from);
    if (to) std::copy(g->b.EdgeTo().begin(), g->b.EdgeTo().end(), to);
    if (samples) std::copy(g->b.EdgeSamples().begin(), g->b.EdgeSamples().end(), samples);
    return AVR_OK;
}
int avr_graph_transport(avr_graph *g, int *row_ptr, int *col, float *val) {
    if (!g || !row_ptr || (g->b.NumEdges() > 0 && (!col || !val))) return fail(AVR_ERR_ARG, "null buffer");
    g->b.Transport(row_ptr, col, val);
    return AVR_OK;
}
int avr_graph_in_node_path_length(avr_graph *g, float *average, long long *count) {
    if (!g) return fail(AVR_ERR_ARG, "null graph");
    // Averager::GetAverage over the added values (util.h:545-565); a double sum here
    if (average) *average = g->b.PathLengthCount() ? (float)(g->b.PathLengthSum() / g->b.PathLengthCount()) : 0.f;
    if (count) *count = g->b.PathLengthCount();
    return AVR_OK;
}

int avr_graph_index_create(long long n, const float *xyz, const float *light_scalar, const float *search_range,
                           float vertex_radius, avr_graph_index **out) {
    if (!out) return fail(AVR_ERR_ARG, "null out");
    *out = nullptr;
    auto *idx = new avr_graph_index();
    if (const char *msg = idx->ix.Build(n, xyz, light_scalar, search_range, vertex_radius)) {
        delete idx;
        return fail(AVR_ERR_ARG, msg);
    }
    idx->uid = ++g_index_uid;
    *out = idx;
    return AVR_OK;
}
int avr_graph_index_destroy(avr_graph_index *idx) {
    delete idx;
    return AVR_OK;
}
int avr_graph_index_connect(const avr_graph_index *idx, long long n, const float *points, float *light_out,
                            int *count_out) {
    if (!idx || n < 0) return fail(AVR_ERR_ARG, "bad connect arguments");
    if (n > 0 && !points) return fail(AVR_ERR_ARG, "null buffer");
    idx->ix.Connect(n, points, light_out, count_out);
    return AVR_OK;
}

int avr_graph_connect(avr_context *c, const avr_graph_index *idx, long long n, const float *points, float *light_out,
                      int *count_out) {
    if (!c || !idx || n < 0) return fail(AVR_ERR_ARG, "bad connect arguments");
    if (n == 0) return AVR_OK;
    if (!points || !light_out || !count_out) return fail(AVR_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_graph_index(c, idx);
    if (rc) return rc;
    Arena<> scratch(c->stream);
    const auto rP = scratch.reserve<float>(3 * (size_t)n), rL = scratch.reserve<float>((size_t)n);
    const auto rC = scratch.reserve<int>((size_t)n);
    HIP_TRY(scratch.commit());
    float *dP = scratch.get(rP), *dL = scratch.get(rL);
    int *dC = scratch.get(rC);
    HIP_TRY(hipMemcpyAsync(dP, points, rP.bytes(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_graph_connect, dim3(blocks_for(n, 256, 256 * 64)), dim3(256), 0, c->stream, c->gidx, n, dP,
                       dL, dC);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(light_out, dL, rL.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(count_out, dC, rC.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_index_coverage(const avr_graph_index *idx, long long n, const float *points, int *node, int *in_range,
                             float *range_sum) {
    if (!idx || n < 0) return fail(AVR_ERR_ARG, "bad coverage arguments");
    if (n > 0 && !points) return fail(AVR_ERR_ARG, "null buffer");
    idx->ix.Coverage(n, points, node, in_range, range_sum);
    return AVR_OK;
}

int avr_graph_coverage(avr_context *c, const avr_graph_index *idx, long long n, const float *points, int *node,
                       int *in_range, float *range_sum) {
    if (!c || !idx || n < 0) return fail(AVR_ERR_ARG, "bad coverage arguments");
    if (n == 0) return AVR_OK;
    if (!points || !node || !in_range || !range_sum) return fail(AVR_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_graph_index(c, idx);
    if (rc) return rc;
    Arena<> scratch(c->stream);
    const auto rP = scratch.reserve<float>(3 * (size_t)n);
    const auto rN = scratch.reserve<int>((size_t)n), rR = scratch.reserve<int>((size_t)n);
    const auto rS = scratch.reserve<float>((size_t)n);
    HIP_TRY(scratch.commit());
    float *dP = scratch.get(rP), *dS = scratch.get(rS);
    int *dN = scratch.get(rN), *dR = scratch.get(rR);
    HIP_TRY(hipMemcpyAsync(dP, points, rP.bytes(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_graph_coverage, dim3(blocks_for(n, 256, 256 * 64)), dim3(256), 0, c->stream, c->gidx, n, dP,
                       dN, dR, dS);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(node, dN, rN.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(in_range, dR, rR.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(range_sum, dS, rS.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

}  // extern "C"

namespace {

// k <= kConnectBuf - 1 (the vertex itself takes one buffer entry) and k <= n - 1
int knn_arguments(const avr_graph_index *idx, int k) {
    if (!idx) return fail(AVR_ERR_ARG, "null graph index");
    if (k < 1 || k > avr::graph::kConnectBuf - 1) return fail(AVR_ERR_ARG, "graph knn: k must be 1..15");
    if ((size_t)k > idx->ix.NumVertices() - 1)
        return fail(AVR_ERR_ARG, "graph knn: Graph does not contain enough vertices (k <= n - 1)");
    return AVR_OK;
}

// k_graph_knn (+ k_graph_range_average when `ranges`) over the context's index copy
int graph_knn_device(avr_context *c, const avr_graph_index *idx, int k, int *ids, float *d2, float *ranges) {
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_graph_index(c, idx);
    if (rc) return rc;
    const int n = (int)idx->ix.NumVertices();
    Arena<> scratch(c->stream);
    const auto rIds = scratch.reserve<int>((size_t)n * (size_t)k);
    const auto rD2 = scratch.reserve<float>((size_t)n * (size_t)k);
    const auto rAvg = scratch.reserve<float>((size_t)n), rRange = scratch.reserve<float>((size_t)n);
    HIP_TRY(scratch.commit());
    int *dIds = scratch.get(rIds);
    float *dD2 = scratch.get(rD2), *dAvg = scratch.get(rAvg), *dRange = scratch.get(rRange);
    const int blocks = blocks_for(n, 256, 256 * 64);
    // the kernels' times go to avr_stats: k_graph_knn to ms_medium, k_graph_range_average to ms_film
    EV_MARK(ev0);
    hipLaunchKernelGGL(avr::k_graph_knn, dim3(blocks), dim3(256), 0, c->stream, c->gidx, n, k, dIds, dD2,
                       ranges ? dAvg : nullptr);
    HIP_TRY(hipGetLastError());
    EV_MARK(ev1);
    c->timed.push_back({ev0, ev1, &avr_stats::ms_medium, true});
    if (ranges) {
        hipLaunchKernelGGL(avr::k_graph_range_average, dim3(blocks), dim3(256), 0, c->stream, n, k, dIds, dAvg, dRange);
        HIP_TRY(hipGetLastError());
        EV_MARK(ev2);
        c->timed.push_back({ev1, ev2, &avr_stats::ms_film, false});
    }
    if (ids) HIP_TRY(hipMemcpyAsync(ids, dIds, rIds.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (d2) HIP_TRY(hipMemcpyAsync(d2, dD2, rD2.bytes(), hipMemcpyDeviceToHost, c->stream));
    if (ranges) HIP_TRY(hipMemcpyAsync(ranges, dRange, rRange.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

}  // namespace

extern "C" {

int avr_graph_index_knn(const avr_graph_index *idx, int k, int *ids, float *d2) {
    int rc = knn_arguments(idx, k);
    if (rc) return rc;
    if (!ids && !d2) return fail(AVR_ERR_ARG, "null buffer");
    idx->ix.Knn(k, ids, d2);
    return AVR_OK;
}
int avr_graph_index_search_ranges(const avr_graph_index *idx, int k, float *ranges) {
    int rc = knn_arguments(idx, k);
    if (rc) return rc;
    if (!ranges) return fail(AVR_ERR_ARG, "null buffer");
    idx->ix.SearchRanges(k, ranges);
    return AVR_OK;
}
int avr_graph_knn(avr_context *c, const avr_graph_index *idx, int k, int *ids, float *d2) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    int rc = knn_arguments(idx, k);
    if (rc) return rc;
    if (!ids && !d2) return fail(AVR_ERR_ARG, "null buffer");
    return graph_knn_device(c, idx, k, ids, d2, nullptr);
}
int avr_graph_search_ranges(avr_context *c, const avr_graph_index *idx, int k, float *ranges) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    int rc = knn_arguments(idx, k);
    if (rc) return rc;
    if (!ranges) return fail(AVR_ERR_ARG, "null buffer");
    return graph_knn_device(c, idx, k, nullptr, nullptr, ranges);
}

}  // extern "C"

namespace {

// What ensure_paths allocates per path: the size policy of the wavefront path state, which
// the analysis' optional detail buffer may not exceed (max_paths paths at most)
constexpr size_t kPathStateBytes = 252;

// The pass loop of avr_render's wavefront organisation for the graph integrators: k_camera,
// then k_graph_render (or, with a uniform graph `uni`, k_graph_render_uniform<view>) and k_film
// (analyze_depth < 0), or k_graph_analyze and k_graph_analyze_reduce with the film left alone;
// passes of at most max_paths samples.
int graph_passes(avr_context *c, const avr_graph_index *idx, const float graph_from_render[16], int spp_begin,
                 int spp_end, int seed, int analyze_depth, int detail, const avr_graph_uniform *uni = nullptr, int view = 0,
                 float light_scale = 1.f) {
    const bool analyze = analyze_depth >= 0;
    static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float *gfr = graph_from_render ? graph_from_render : kIdentity;
    if (!affine(gfr)) return fail(AVR_ERR_ARG, "graph_from_render must be affine");
    avr::Xf xf;
    copy_xf(xf, gfr);
    avr::smp::ZSobolParams zs{};
    int rc = render_sampler(c, spp_end, seed, &zs);
    if (rc) return rc;
    rc = uni ? ensure_graph_uniform(c, uni) : ensure_graph_index(c, idx);
    if (rc) return rc;
    PassPlan plan;
    if ((rc = pass_plan(c, false, spp_begin, spp_end, &plan))) return rc;
    const long long P = plan.P, Smax = plan.Smax, need = plan.need;
    if (analyze && detail) {
        // asked for, never silent: pass samples x max_depth x 24 B, within the path state's policy
        const unsigned long long entries = (unsigned long long)need * (unsigned long long)std::max(analyze_depth, 1);
        const unsigned long long limit = (unsigned long long)std::max<long long>(c->max_paths, need) * kPathStateBytes;
        if (entries > limit / sizeof(avr::graph::AnalyzeDetail))
            return fail(AVR_ERR_ARG, "graph analyze: the detail buffer (" + std::to_string(need) + " pass samples x max_depth " +
                                         std::to_string(analyze_depth) + " x 24 B) exceeds the path state's " +
                                         std::to_string(limit) + " B (max_paths x 252 B): lower max_depth or max_paths, or pass detail = 0");
        HIP_TRY(c->d_adetail.reserve((size_t)entries, c->stream));
    }
    rc = ensure_paths(c, need);
    if (rc) return rc;
    // (queued kernels may still read the buffer a larger one replaces: grow drains the stream)
    HIP_TRY(analyze ? c->d_arec.reserve((size_t)need, c->stream) : c->d_gside.reserve((size_t)need, c->stream));
    if (analyze && !c->d_aacc) {
        HIP_TRY(c->d_aacc.alloc((size_t)P));
        HIP_TRY(hipMemsetAsync(c->d_aacc.get(), 0, (size_t)P * sizeof(avr::graph::AnalyzeAcc), c->stream));
    }
    EV_MARK(evStart);
    for (long long base = spp_begin; base < spp_end; base += Smax) {
        const int S = (int)std::min<long long>(Smax, spp_end - base);
        avr::Params p;
        pass_params(c, zs, seed, 1, P, base, S, &p);
        const long long n0 = P * S;
        // the record keeps the camera's own ray: the graph kernels solve the primitive once from
        // it (k_camera would move it to the interface entry, as the path kernels want it)
        avr::Params pc = p;
        pc.med.boundary = 0;
        int c1;
        if ((rc = launch_camera(c, pc, &c1))) return rc;
        // one lane per camera record, as many blocks as records up to 64 per CU's worth
        const int nb = blocks_for(n0, 256, 256 * 64);
        if (analyze) {
            avr::graph::AnalyzeDetail *det = detail ? c->d_adetail.get() : nullptr;
            AVR_GRAPH_LAUNCH_ZG(avr::k_graph_analyze, c->sampler_kind != 0, graph_interface(c), nb, p, c->gidx, xf,
                                analyze_depth, c->d_arec.get(), det);
        } else if (uni) {
            if (view) AVR_GRAPH_LAUNCH_ZGV(avr::k_graph_render_uniform, c->sampler_kind != 0, graph_interface(c), 1, nb, p,
                                           c->guni, xf, light_scale, c->d_gside.get());
            else AVR_GRAPH_LAUNCH_ZGV(avr::k_graph_render_uniform, c->sampler_kind != 0, graph_interface(c), 0, nb, p,
                                      c->guni, xf, light_scale, c->d_gside.get());
        } else {
            AVR_GRAPH_LAUNCH_ZG(avr::k_graph_render, c->sampler_kind != 0, graph_interface(c), nb, p, c->gidx, xf,
                                c->d_gside.get());
        }
        HIP_TRY(hipGetLastError());
        EV_MARK(m1);
        c->timed.push_back({c1, m1, &avr_stats::ms_medium, true});
        if (analyze) {
            hipLaunchKernelGGL(avr::k_graph_analyze_reduce, dim3(blocks_for(P)), dim3(256), 0, c->stream, (int)P, S,
                               c->d_arec.get(), c->d_aacc.get());
            HIP_TRY(hipGetLastError());
            EV_MARK(f1);
            c->timed.push_back({m1, f1, &avr_stats::ms_film, false});
        } else if ((rc = launch_film(c, p, false, m1))) {
            return rc;
        }
        LastPass lp = c->last.without_kpaths((int)base, S);
        lp.graph = !analyze; lp.analyze = analyze ? (detail ? 2 : 1) : 0; lp.analyze_depth = analyze_depth;
        c->last = lp;
    }
    EV_MARK(evEnd);
    c->timed.push_back({evStart, evEnd, &avr_stats::ms_total, false});
    return AVR_OK;
}

// What the graph renders require of the context (avr_graph_render, avr_graph_render_uniform)
int graph_render_state(avr_context *c, int spp_begin, int spp_end) {
    if (!c->has_medium || !c->has_camera || !c->has_film) return fail(AVR_ERR_STATE, "medium, camera and film required");
    if (spp_begin < 0 || spp_end < spp_begin) return fail(AVR_ERR_ARG, "bad sample range");
    // GraphIntegrator::Create takes the scene's one DistantLight (lightSpectrum, lightDir)
    if (c->lights.n != 1 || c->h_lights[0].type != 0)
        return fail(AVR_ERR_STATE, "graph render: exactly one distant light required");
    if (c->med.boundary != 0 && c->graph_geometry == 0)
        return fail(AVR_ERR_STATE, "graph render: the graph's geometry model is the medium's bounds box (no interface sphere or convex; avr_graph_set_geometry(ctx, 1) takes the interface as the primitive)");
    return AVR_OK;
}

}  // namespace

extern "C" {

int avr_graph_render(avr_context *c, const avr_graph_index *idx, const float graph_from_render[16], int spp_begin,
                     int spp_end, int seed) {
    if (!c || !idx) return fail(AVR_ERR_ARG, "null context or graph index");
    int rc = graph_render_state(c, spp_begin, spp_end);
    if (rc) return rc;
    return graph_passes(c, idx, graph_from_render, spp_begin, spp_end, seed, -1, 0);
}

int avr_graph_render_uniform(avr_context *c, const avr_graph_uniform *u, const float graph_from_render[16], int spp_begin,
                             int spp_end, int seed, int view, float light_scale) {
    if (!c || !u) return fail(AVR_ERR_ARG, "null context or uniform graph");
    if (view != 0 && view != 1) return fail(AVR_ERR_ARG, "graph render: view must be 0 (render) or 1 (voxel view)");
    if (!std::isfinite(light_scale)) return fail(AVR_ERR_ARG, "graph render: light_scale must be finite");
    int rc = graph_render_state(c, spp_begin, spp_end);
    if (rc) return rc;
    return graph_passes(c, nullptr, graph_from_render, spp_begin, spp_end, seed, -1, 0, u, view, light_scale);
}

int avr_graph_analyze(avr_context *c, const avr_graph_index *idx, const float graph_from_render[16], int spp_begin,
                      int spp_end, int seed, int max_depth, int detail) {
    if (!c || !idx) return fail(AVR_ERR_ARG, "null context or graph index");
    if (!c->has_medium || !c->has_camera || !c->has_film) return fail(AVR_ERR_STATE, "medium, camera and film required");
    if (spp_begin < 0 || spp_end < spp_begin) return fail(AVR_ERR_ARG, "bad sample range");
    if (max_depth < 0) return fail(AVR_ERR_ARG, "graph analyze: max_depth must not be negative");
    if (c->med.boundary != 0 && c->graph_geometry == 0)
        return fail(AVR_ERR_STATE, "graph analyze: the graph's geometry model is the medium's bounds box (no interface sphere or convex; avr_graph_set_geometry(ctx, 1) takes the interface as the primitive)");
    return graph_passes(c, idx, graph_from_render, spp_begin, spp_end, seed, max_depth, detail);
}

int avr_graph_analysis_clear(avr_context *c) {
    if (!c || !c->has_film) return fail(AVR_ERR_STATE, "no film");
    if (!c->d_aacc) return AVR_OK;   // nothing analysed on this film yet: the sums start at zero
    const size_t np = (size_t)c->film.bw * c->film.bh;
    HIP_TRY(hipMemsetAsync(c->d_aacc.get(), 0, np * sizeof(avr::graph::AnalyzeAcc), c->stream));
    return AVR_OK;
}

int avr_graph_analysis_read(avr_context *c, unsigned long long *total, unsigned long long *node,
                            unsigned long long *search, unsigned long long *in_range, double *range_sum) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film) return fail(AVR_ERR_STATE, "no film");
    const size_t np = (size_t)c->film.bw * c->film.bh;
    std::vector<avr::graph::AnalyzeAcc> h(np, avr::graph::AnalyzeAcc{0, 0, 0, 0, 0.0});
    if (c->d_aacc) HIP_TRY(hipMemcpy(h.data(), c->d_aacc.get(), np * sizeof(avr::graph::AnalyzeAcc), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < np; ++i) {
        if (total) total[i] = h[i].total;
        if (node) node[i] = h[i].node;
        if (search) search[i] = h[i].search;
        if (in_range) in_range[i] = h[i].in_range;
        if (range_sum) range_sum[i] = h[i].range;
    }
    return AVR_OK;
}

int avr_graph_analyze_last_pass(avr_context *c, float *o, float *d, int *counts, float *points, int *node,
                                int *in_range, float *range_sum, long long n_max, int max_depth) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film) return fail(AVR_ERR_ARG, "null arg");
    if (c->last.analyze != 2) return fail(AVR_ERR_STATE, "the last render was not avr_graph_analyze's with detail");
    const long long n = (long long)c->film.bw * c->film.bh * c->last.S;
    const int md = c->last.analyze_depth;
    if (n_max < n) return fail(AVR_ERR_ARG, "buffer too small for the last pass");
    if (max_depth != md) return fail(AVR_ERR_ARG, "max_depth differs from the analysis'");
    if (n == 0) return AVR_OK;
    if (o || d) {
        std::vector<float4> h((size_t)n);
        const float4 *src[2] = {c->ps.o, c->ps.d};
        float *dst[2] = {o, d};
        for (int k = 0; k < 2; ++k) {
            if (!dst[k]) continue;
            HIP_TRY(hipMemcpy(h.data(), src[k], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
            for (long long i = 0; i < n; ++i) {
                dst[k][3 * i] = h[(size_t)i].x;
                dst[k][3 * i + 1] = h[(size_t)i].y;
                dst[k][3 * i + 2] = h[(size_t)i].z;
            }
        }
    }
    std::vector<avr::graph::AnalyzeRec> rec((size_t)n);
    HIP_TRY(hipMemcpy(rec.data(), c->d_arec.get(), (size_t)n * sizeof(avr::graph::AnalyzeRec), hipMemcpyDeviceToHost));
    if (counts)
        for (long long i = 0; i < n; ++i) counts[i] = rec[(size_t)i].total;
    if (md == 0 || (!points && !node && !in_range && !range_sum)) return AVR_OK;
    const size_t entries = (size_t)n * (size_t)md;
    std::vector<avr::graph::AnalyzeDetail> det(entries);
    HIP_TRY(hipMemcpy(det.data(), c->d_adetail.get(), entries * sizeof(avr::graph::AnalyzeDetail), hipMemcpyDeviceToHost));
    for (long long i = 0; i < n; ++i)
        for (int k = 0; k < md; ++k) {
            const size_t e = (size_t)i * (size_t)md + (size_t)k;
            // entries past the sample's count were never written
            const bool set = k < rec[(size_t)i].total;
            const avr::graph::AnalyzeDetail z = set ? det[e] : avr::graph::AnalyzeDetail{0.f, 0.f, 0.f, 0, 0, 0.f};
            if (points) {
                points[3 * e] = z.x;
                points[3 * e + 1] = z.y;
                points[3 * e + 2] = z.z;
            }
            if (node) node[e] = z.node;
            if (in_range) in_range[e] = z.in_range;
            if (range_sum) range_sum[e] = z.range_sum;
        }
    return AVR_OK;
}

int avr_graph_last_pass(avr_context *c, float *o, float *d, float *points, int *counts, long long n_max) {
    AVR_QUIESCE(c);
    if (!c || !c->has_film) return fail(AVR_ERR_ARG, "null arg");
    if (!c->last.graph) return fail(AVR_ERR_STATE, "the last render was not avr_graph_render's");
    const long long n = (long long)c->film.bw * c->film.bh * c->last.S;
    if (n_max < n) return fail(AVR_ERR_ARG, "buffer too small for the last pass");
    if (n == 0) return AVR_OK;
    std::vector<float4> h((size_t)n);
    const float4 *src[3] = {c->ps.o, c->ps.d, c->d_gside.get()};
    float *dst[3] = {o, d, points};
    for (int k = 0; k < 3; ++k) {
        if (!dst[k] && !(k == 2 && counts)) continue;
        HIP_TRY(hipMemcpy(h.data(), src[k], (size_t)n * sizeof(float4), hipMemcpyDeviceToHost));
        for (long long i = 0; i < n; ++i) {
            if (dst[k]) {
                dst[k][3 * i] = h[(size_t)i].x;
                dst[k][3 * i + 1] = h[(size_t)i].y;
                dst[k][3 * i + 2] = h[(size_t)i].z;
            }
            if (k == 2 && counts) std::memcpy(&counts[i], &h[(size_t)i].w, sizeof(int));
        }
    }
    return AVR_OK;
}

int avr_graph_uniform_create(long long m, const int *coors, const float *light, float spacing, avr_graph_uniform **out) {
    if (!out) return fail(AVR_ERR_ARG, "null out");
    *out = nullptr;
    auto *u = new avr_graph_uniform();
    const std::string msg = u->u.Create(m, coors, light, spacing);
    if (!msg.empty()) {
        delete u;
        return fail(AVR_ERR_ARG, msg);
    }
    u->uid = ++g_index_uid;
    *out = u;
    return AVR_OK;
}
int avr_graph_uniform_from_points(long long n, const float *xyz, const float *light, float spacing, int reduce,
                                  int *vertex_of, avr_graph_uniform **out) {
    if (!out) return fail(AVR_ERR_ARG, "null out");
    *out = nullptr;
    auto *u = new avr_graph_uniform();
    const std::string msg = u->u.FromPoints(n, xyz, light, spacing, reduce, vertex_of);
    if (!msg.empty()) {
        delete u;
        return fail(AVR_ERR_ARG, msg);
    }
    u->uid = ++g_index_uid;
    *out = u;
    return AVR_OK;
}
int avr_graph_uniform_destroy(avr_graph_uniform *u) {
    delete u;
    return AVR_OK;
}
int avr_graph_uniform_size(const avr_graph_uniform *u, long long *n_vertices, float *spacing) {
    if (!u) return fail(AVR_ERR_ARG, "null uniform graph");
    if (n_vertices) *n_vertices = (long long)u->u.NumVertices();
    if (spacing) *spacing = u->u.Spacing();
    return AVR_OK;
}
int avr_graph_uniform_get(const avr_graph_uniform *u, int *coors, float *light) {
    if (!u) return fail(AVR_ERR_ARG, "null uniform graph");
    const size_t m = u->u.NumVertices();
    if (coors) std::memcpy(coors, u->u.Coors(), 3 * m * sizeof(int));
    if (light) std::memcpy(light, u->u.Light(), m * sizeof(float));
    return AVR_OK;
}
int avr_graph_uniform_lookup(const avr_graph_uniform *u, long long n, const float *points, int *id_out, float *light_out) {
    if (!u || n < 0) return fail(AVR_ERR_ARG, "bad uniform lookup arguments");
    if (n > 0 && !points) return fail(AVR_ERR_ARG, "null buffer");
    u->u.Lookup(n, points, id_out, light_out);
    return AVR_OK;
}
int avr_graph_uniform_trace(const avr_graph_uniform *u, long long n, const float *o, const float *d, int *id_out,
                            float *hit0, float *hit1) {
    if (!u || n < 0) return fail(AVR_ERR_ARG, "bad uniform trace arguments");
    if (n > 0 && (!o || !d)) return fail(AVR_ERR_ARG, "null buffer");
    u->u.Trace(n, o, d, id_out, hit0, hit1);
    return AVR_OK;
}

int avr_graph_uniform_lookup_device(avr_context *c, const avr_graph_uniform *u, long long n, const float *points,
                                    int *id_out, float *light_out) {
    if (!c || !u || n < 0) return fail(AVR_ERR_ARG, "bad uniform lookup arguments");
    if (n == 0) return AVR_OK;
    if (!points || !id_out || !light_out) return fail(AVR_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_graph_uniform(c, u);
    if (rc) return rc;
    Arena<> scratch(c->stream);
    const auto rP = scratch.reserve<float>(3 * (size_t)n), rL = scratch.reserve<float>((size_t)n);
    const auto rI = scratch.reserve<int>((size_t)n);
    HIP_TRY(scratch.commit());
    float *dP = scratch.get(rP), *dL = scratch.get(rL);
    int *dI = scratch.get(rI);
    HIP_TRY(hipMemcpyAsync(dP, points, rP.bytes(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_graph_uniform_lookup, dim3(blocks_for(n, 256, 256 * 64)), dim3(256), 0, c->stream, c->guni, n,
                       dP, dI, dL);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(light_out, dL, rL.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(id_out, dI, rI.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_uniform_trace_device(avr_context *c, const avr_graph_uniform *u, long long n, const float *o, const float *d,
                                   int *id_out, float *hit0, float *hit1) {
    if (!c || !u || n < 0) return fail(AVR_ERR_ARG, "bad uniform trace arguments");
    if (n == 0) return AVR_OK;
    if (!o || !d || !id_out || !hit0 || !hit1) return fail(AVR_ERR_ARG, "null buffer");
    HIP_TRY(hipSetDevice(c->device));
    int rc = ensure_graph_uniform(c, u);
    if (rc) return rc;
    Arena<> scratch(c->stream);
    const auto rO = scratch.reserve<float>(3 * (size_t)n), rD = scratch.reserve<float>(3 * (size_t)n);
    const auto rI = scratch.reserve<int>((size_t)n);
    const auto rH0 = scratch.reserve<float>((size_t)n), rH1 = scratch.reserve<float>((size_t)n);
    HIP_TRY(scratch.commit());
    float *dO = scratch.get(rO), *dD = scratch.get(rD), *dH0 = scratch.get(rH0), *dH1 = scratch.get(rH1);
    int *dI = scratch.get(rI);
    HIP_TRY(hipMemcpyAsync(dO, o, rO.bytes(), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dD, d, rD.bytes(), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(avr::k_graph_uniform_trace, dim3(blocks_for(n, 256, 256 * 64)), dim3(256), 0, c->stream, c->guni, n,
                       dO, dD, dI, dH0, dH1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(id_out, dI, rI.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hit0, dH0, rH0.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(hit1, dH1, rH1.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return AVR_OK;
}

int avr_graph_capture(avr_context *c, int n_bundles, const float *origin, const float *dir, const float *xvec,
                      const float *yvec, int num_steps, float *out_points4, long long *n_captured) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    if (n_bundles < 1 || num_steps < 0) return fail(AVR_ERR_ARG, "bad capture arguments");
    if (!origin || !dir || !xvec || !yvec || !out_points4 || !n_captured) return fail(AVR_ERR_ARG, "null buffer");
    const long long side = 2ll * num_steps + 1;
    if (side > 0x7fffffffll / side || side * side > 0x7fffffffll / n_bundles)
        return fail(AVR_ERR_ARG, "capture: more than 2^31 - 1 rays");
    if (!c->has_medium) return fail(AVR_ERR_STATE, "medium required");
    for (int b = 0; b < n_bundles; ++b) {
        bool finite = true;
        for (int k = 0; k < 3; ++k)
            finite = finite && std::isfinite(origin[3 * b + k]) && std::isfinite(dir[3 * b + k]) &&
                     std::isfinite(xvec[3 * b + k]) && std::isfinite(yvec[3 * b + k]);
        if (!finite || (dir[3 * b] == 0 && dir[3 * b + 1] == 0 && dir[3 * b + 2] == 0))
            return fail(AVR_ERR_ARG, "capture: bundle " + std::to_string(b) + ": finite vectors and a direction other than 0 required");
    }
    HIP_TRY(hipSetDevice(c->device));
    const long long n = side * side * n_bundles;
    const size_t szB = (size_t)n_bundles * 3 * sizeof(float);
    int nCap = 0;   // (before the arena: copied into until the arena's drain)
    Arena<> scratch(c->stream);
    const auto rOut = scratch.reserve<float4>((size_t)n);
    const auto rB = scratch.reserve<float>((size_t)12 * n_bundles);   // origin | dir | xvec | yvec
    const auto rN = scratch.reserve<int>(1);
    HIP_TRY(scratch.commit());
    float4 *dOut = scratch.get(rOut);
    float *dB = scratch.get(rB);
    int *dN = scratch.get(rN);
    const float *src[4] = {origin, dir, xvec, yvec};
    HIP_TRY(hipMemsetAsync(dN, 0, sizeof(int), c->stream));
    for (int k = 0; k < 4; ++k)
        HIP_TRY(hipMemcpyAsync(dB + (size_t)k * 3 * n_bundles, src[k], szB, hipMemcpyHostToDevice, c->stream));
    AVR_GRAPH_LAUNCH_G(avr::k_graph_capture, graph_interface(c), blocks_for(n, 256, 256 * 64), c->med, n, num_steps, dB,
                       dB + (size_t)3 * n_bundles, dB + (size_t)6 * n_bundles, dB + (size_t)9 * n_bundles, dOut, dN);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_points4, dOut, rOut.bytes(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(&nCap, dN, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *n_captured = nCap;
    return AVR_OK;
}

}  // extern "C"

namespace {

// Uniform::FromPoints(reduce 0) on the device: the number of distinct voxels and, when
// vertex_of is given, every point's vertex id (ids in the order of first appearance)
int uniform_points_device(avr_context *c, long long n, const float *xyz, float spacing, long long *count, int *vertex_of) {
    if (!c) return fail(AVR_ERR_ARG, "null context");
    // the host routine's checks, in its order
    if (!(spacing > 0) || !std::isfinite(spacing)) return fail(AVR_ERR_ARG, "graph uniform: spacing must be positive and finite");
    if (n < 1 || n > 0x3fffffff || !xyz) return fail(AVR_ERR_ARG, "graph uniform: at least one vertex required");
    HIP_TRY(hipSetDevice(c->device));
    size_t cap = 16;
    while (cap < 2 * (size_t)n) cap *= 2;
    const size_t nw = ((size_t)n + 63) / 64;
    const size_t N = (size_t)n, szK = cap * 8, szF = cap * 4;
    int scal[3] = {0x7fffffff, 0, 0};   // bad, count, total (before the arena: copied into until its drain)
    Arena<> scratch(c->stream);
    const auto rKeys = scratch.reserve<unsigned long long>(cap), rMask = scratch.reserve<unsigned long long>(nw);
    const auto rX = scratch.reserve<float>(3 * N);
    const auto rFirst = scratch.reserve<int>(cap), rSlot = scratch.reserve<int>(N), rState = scratch.reserve<int>(N);
    const auto rIds = scratch.reserve<int>(N), rCnt = scratch.reserve<int>(nw), rScal = scratch.reserve<int>(3);
    HIP_TRY(scratch.commit());
    unsigned long long *dKeys = scratch.get(rKeys), *dMask = scratch.get(rMask);
    float *dX = scratch.get(rX);
    int *dFirst = scratch.get(rFirst), *dSlot = scratch.get(rSlot), *dState = scratch.get(rState);
    int *dIds = scratch.get(rIds), *dCnt = scratch.get(rCnt), *dScal = scratch.get(rScal);
    HIP_TRY(hipMemsetAsync(dKeys, 0xff, szK, c->stream));
    HIP_TRY(hipMemsetAsync(dFirst, 0x7f, szF, c->stream));   // 0x7f7f7f7f: above every index
    HIP_TRY(hipMemcpyAsync(dScal, scal, sizeof scal, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dX, xyz, N * 12, hipMemcpyHostToDevice, c->stream));
    const int blocks = blocks_for(n, 256, 256 * 64);
    hipLaunchKernelGGL(avr::k_graph_uniform_insert, dim3(blocks), dim3(256), 0, c->stream, n, dX, spacing, dKeys,
                       (uint32_t)(cap - 1), dFirst, dSlot, dScal);
    hipLaunchKernelGGL(avr::k_graph_uniform_first, dim3(blocks), dim3(256), 0, c->stream, n, dFirst, dSlot, dState,
                       dScal + 1);
    if (vertex_of) {
        hipLaunchKernelGGL(avr::k_graph_merge_flags, dim3(blocks), dim3(256), 0, c->stream, 0, (int)n, dState, dMask, dCnt);
        hipLaunchKernelGGL(avr::k_graph_merge_scan, dim3(1), dim3(256), 0, c->stream, (int)nw, dCnt, dScal + 2);
        hipLaunchKernelGGL(avr::k_graph_merge_ids, dim3(blocks), dim3(256), 0, c->stream, 0, (int)n, dState, dMask, dCnt,
                           dIds);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(scal, dScal, sizeof scal, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    // an invalid point has no vertex: its id would be read from outside the scan
    if (vertex_of && scal[0] == 0x7fffffff) HIP_TRY(hipMemcpy(vertex_of, dIds, N * 4, hipMemcpyDeviceToHost));
    if (scal[0] != 0x7fffffff)
        return fail(AVR_ERR_ARG, "graph uniform: vertex " + std::to_string(scal[0]) + ": coordinate outside +-2^20");
    *count = scal[1];
    return AVR_OK;
}

// One flood on the device (k_graph_voxels_level), level by level from the frontier the host
// state starts with; the state is uploaded before and read back after
int voxels_flood_device(avr_context *c, avr::graph::Voxels &vx, bool fill, const std::vector<int> &start, int *levels) {
    HIP_TRY(hipSetDevice(c->device));
    const avr::graph::VoxelDims d = vx.Dims();
    const size_t szS = vx.StateBytes();
    int nFront = (int)start.size(), lv = 0, cur = 0;   // (nFront before the arena: copied into until its drain)
    Arena<> scratch(c->stream);
    const auto rState = scratch.reserve<unsigned char>(szS);
    const auto rQ0 = scratch.reserve<int>((size_t)d.cells), rQ1 = scratch.reserve<int>((size_t)d.cells);
    const auto rN = scratch.reserve<int>(1);
    HIP_TRY(scratch.commit());
    unsigned *dState = (unsigned *)scratch.get(rState);
    int *dQ[2] = {scratch.get(rQ0), scratch.get(rQ1)};
    int *dN = scratch.get(rN);
    HIP_TRY(hipMemcpyAsync(dState, vx.State(), szS, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(dQ[0], start.data(), start.size() * 4, hipMemcpyHostToDevice, c->stream));
    long long seen = nFront;
    // each cell joins a frontier at most once, so the levels cannot outnumber the cells
    while (nFront > 0 && lv < d.cells) {
        ++lv;
        HIP_TRY(hipMemsetAsync(dN, 0, sizeof(int), c->stream));
        const int blocks = blocks_for(nFront, 256, 256 * 64);
        if (fill)
            hipLaunchKernelGGL((avr::k_graph_voxels_level<1>), dim3(blocks), dim3(256), 0, c->stream, d, dState, dQ[cur], nFront,
                               dQ[cur ^ 1], dN);
        else
            hipLaunchKernelGGL((avr::k_graph_voxels_level<0>), dim3(blocks), dim3(256), 0, c->stream, d, dState, dQ[cur], nFront,
                               dQ[cur ^ 1], dN);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&nFront, dN, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        cur ^= 1;
        seen += nFront;
        if (nFront < 0 || seen > d.cells) return fail(AVR_ERR_HIP, "graph voxels: frontier count out of range");
    }
    HIP_TRY(hipMemcpy(vx.State(), dState, szS, hipMemcpyDeviceToHost));
    if (levels) *levels = lv;
    return AVR_OK;
}

}  // namespace

struct avr_graph_voxels {
    avr::graph::Voxels v;
};

extern "C" {

int avr_graph_uniform_count_device(avr_context *c, long long n, const float *xyz, float spacing, long long *count) {
    if (!count) return fail(AVR_ERR_ARG, "null out");
    return uniform_points_device(c, n, xyz, spacing, count, nullptr);
}

int avr_graph_uniform_from_points_device(avr_context *c, long long n, const float *xyz, float spacing,
                                         avr_graph_uniform **out, int *vertex_of) {
    if (!out) return fail(AVR_ERR_ARG, "null out");
    *out = nullptr;
    std::vector<int> own;
    if (!vertex_of && n >= 1 && n <= 0x3fffffff) {
        own.resize((size_t)n);
        vertex_of = own.data();
    }
    long long m = 0;
    const int rc = uniform_points_device(c, n, xyz, spacing, &m, vertex_of);
    if (rc) return rc;
    // ids follow the first appearance: the point that brings id `next` is that vertex's first
    std::vector<int> coors((size_t)m * 3);
    long long next = 0;
    for (long long i = 0; i < n && next < m; ++i)
        if (vertex_of[i] == next) {
            (void)avr::graph::uniform_coors(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], spacing, coors.data() + 3 * next);
            ++next;
        }
    if (next != m) return fail(AVR_ERR_HIP, "graph uniform from points: device ids are not in order of first appearance");
    const std::vector<float> light((size_t)m, 0.f);
    auto *u = new avr_graph_uniform();
    const std::string msg = u->u.Create(m, coors.data(), light.data(), spacing);
    if (!msg.empty()) {
        delete u;
        return fail(AVR_ERR_ARG, msg);
    }
    u->uid = ++g_index_uid;
    *out = u;
    return AVR_OK;
}

int avr_graph_voxels_create(const float pmin[3], const float pmax[3], float spacing, long long m, const int *coors,
                            avr_graph_voxels **out) {
    if (!out) return fail(AVR_ERR_ARG, "null out");
    *out = nullptr;
    auto *v = new avr_graph_voxels();
    const std::string msg = v->v.Create(pmin, pmax, spacing, m, coors);
    if (!msg.empty()) {
        delete v;
        return fail(AVR_ERR_ARG, msg);
    }
    *out = v;
    return AVR_OK;
}
int avr_graph_voxels_destroy(avr_graph_voxels *v) {
    delete v;
    return AVR_OK;
}
int avr_graph_voxels_single_layer(avr_context *c, avr_graph_voxels *v, int *levels) {
    if (!v) return fail(AVR_ERR_ARG, "null voxels");
    if (!c) {
        v->v.SingleLayer(levels);
        return AVR_OK;
    }
    std::vector<int> start;
    v->v.BeginSingleLayer(&start);
    const int rc = voxels_flood_device(c, v->v, false, start, levels);
    if (rc == AVR_OK) v->v.SetSingleDone();
    return rc;
}
int avr_graph_voxels_fill(avr_context *c, avr_graph_voxels *v, int start, int *levels) {
    if (!v) return fail(AVR_ERR_ARG, "null voxels");
    if (!v->v.SingleDone()) {   // FillInside runs the single layer first when it has not run (:184-186)
        const int rc = avr_graph_voxels_single_layer(c, v, nullptr);
        if (rc) return rc;
    }
    if (!c) {
        const std::string msg = v->v.Fill(start, levels);
        return msg.empty() ? AVR_OK : fail(AVR_ERR_ARG, msg);
    }
    std::vector<int> seeds;
    const std::string msg = v->v.BeginFill(start, &seeds);
    if (!msg.empty()) return fail(AVR_ERR_ARG, msg);
    return voxels_flood_device(c, v->v, true, seeds, levels);
}
int avr_graph_voxels_state(const avr_graph_voxels *v, int lo[3], int n[3], unsigned char *state, long long capacity) {
    if (!v) return fail(AVR_ERR_ARG, "null voxels");
    const avr::graph::VoxelDims &d = v->v.Dims();
    for (int a = 0; a < 3; ++a) {
        if (lo) lo[a] = d.lo[a];
        if (n) n[a] = d.n[a];
    }
    if (state) {
        if (capacity < d.cells) return fail(AVR_ERR_ARG, "graph voxels: state buffer shorter than the cell count");
        std::memcpy(state, v->v.State(), (size_t)d.cells);
    }
    return AVR_OK;
}
int avr_graph_voxels_visited(const avr_graph_voxels *v, long long *visited, long long *cast, long long *single_layer,
                             long long *filled) {
    if (!v) return fail(AVR_ERR_ARG, "null voxels");
    if (visited) *visited = v->v.Count(avr::graph::kVoxOutside);
    if (cast) *cast = v->v.Count(avr::graph::kVoxCast);
    if (single_layer) *single_layer = v->v.Count(avr::graph::kVoxSingle);
    if (filled) *filled = v->v.Count(avr::graph::kVoxFilled);
    return AVR_OK;
}

}  // extern "C"
