// avr_graph_index.h — the free graph's vertex index and GraphIntegrator::ConnectToGraph
// (graph_integrator.cpp:24-81 Initialize, :249-280 ConnectToGraph, graph/util.h:529-568
// Averager) over it. One search routine, compiled for the host (avr_graph_index_connect) and
// for the device (k_graph_connect, k_graph_render): the semantics below are the contract of
// both.
//
// Layout: a uniform cell grid over the vertices' bounding box, vertices counting-sorted by
// cell (ascending vertex id within a cell), one 16-B record {x, y, z, lightScalar} per vertex;
// the vertex ids and, when search ranges were given, their squares as parallel arrays in the
// same order. The cell edge is the vertex radius, doubled until the grid holds at most
// kIndexCellBudget = 2^21 cells (8 MiB of cell offsets).
//
// Connect: nanoflann's radiusSearch keeps vertices with L2_Simple_Adaptor's distance
// d2 = ((qx-vx)² + (qy-vy)²) + (qz-vz)² (float, no contraction) strictly below the squared
// radius and sorts them by distance; ties go to the lower vertex id here (nanoflann leaves
// them unspecified). Stage 0 searches Sqr(vertexRadius); with search ranges and an empty
// stage 0, stage 1 searches the 99th-percentile squared range and stage 2 (stage 1 still
// empty) the largest, both dropping vertices with d2 > Sqr(range[v]). The Averager then sums
// light * (1 / d2) and 1 / d2 in result order, in float; d2 == 0 gives an infinite weight and
// the reference's NaN. The ordered sum is exact for any neighbour count: the kConnectBuf
// nearest are kept sorted while the cells are scanned, and when more qualify the cells are
// scanned again for the next kConnectBuf above the last key summed.
//
// The cell range of a search comes from double arithmetic on a radius widened by 1e-6
// relative (the float d2 of a vertex that qualifies exceeds its exact distance by a few ulp
// at most), with the monotone cell function the vertices were sorted by: no vertex whose
// computed d2 qualifies is outside the cells visited, for queries outside the box and radii
// beyond it too.
//
// k nearest neighbours: FreeGraphBuilder::ComputeSearchRanges (free_graph_builder.cpp:473-548)
// over the same cells, buffer and key order: index_knn, for the host (avr_graph_index_knn,
// avr_graph_index_search_ranges) and for the device (k_graph_knn), and the two Averager
// levels that turn the distances into renderSearchRange.
//
// Coverage: IntegrationAnalyzer's Analyze (graph/analysis/integration_analyzer.cpp:56-83) for
// a point in graph space: index_coverage, for the host (avr_graph_index_coverage) and for the
// device (k_graph_coverage, k_graph_analyze). node: radiusSearch(Sqr(vertexRadius)) returned a
// vertex (d2 < r2). in_range: the vertices of radiusSearch(maxSquaredSearchRange) left after
// those with d2 > Sqr(range[v]) are dropped, stage 2's search and filter; range_sum: the float
// sum from 0 of sqrtf(d2) over them in ascending (d2, id), exact for any count by the same
// rescans as Connect. An index without search ranges gives in_range = 0 and range_sum = 0 (the
// reference would search maxSquaredSearchRange as Initialize left it, unset, there).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#ifndef AVR_HD
#define AVR_HD inline
#endif

namespace avr {
namespace graph {

constexpr long long kIndexCellBudget = 1ll << 21;
constexpr int kConnectBuf = 16;

struct alignas(16) IndexRec { float x, y, z, light; };

// What a query reads: the host index's arrays, or their device copies
struct IndexView {
    const IndexRec *rec;      // vertices sorted by cell
    const int *id;            // vertex id per sorted slot
    const float *range2;      // Sqr(renderSearchRange) per sorted slot, or null
    const int *cell_start;    // dim[0] * dim[1] * dim[2] + 1 offsets into rec
    double bmin[3], inv_cell;
    int dim[3];
    float r2, perc99, max_r2; // Sqr(vertexRadius), perc99 / maxSquaredSearchRange
};

// The cell coordinate along one axis, before clamping: monotone in x
AVR_HD double index_cell_coord(double x, double bmin, double inv) { return std::floor((x - bmin) * inv); }

// Cells [lo, hi] of one axis that can hold a vertex within r of q; false: none
AVR_HD bool index_cell_range(double q, double r, double bmin, double inv, int dim, int *lo, int *hi) {
    const double a = index_cell_coord(q - r, bmin, inv), b = index_cell_coord(q + r, bmin, inv);
    if (!(a <= (double)(dim - 1)) || !(b >= 0.0)) return false;   // also a NaN query
    *lo = a < 0.0 ? 0 : (int)a;
    *hi = b > (double)(dim - 1) ? dim - 1 : (int)b;
    return true;
}

// Scan the cells around q for vertices with d2 < r2 (and, with `filter`, not beyond their own
// squared range) whose key (d2, id) is above (lastD2, lastId); keep the kConnectBuf smallest
// keys sorted in buf (*kept of them) and return how many qualified.
template <typename Buf>
AVR_HD int index_collect(const IndexView &ix, float qx, float qy, float qz, float r2, bool filter, float lastD2,
                         int lastId, Buf &buf, int *kept) {
    *kept = 0;
    const double r = std::sqrt((double)r2) * (1.0 + 1e-6) + 1e-22;
    int lo[3], hi[3];
    if (!index_cell_range((double)qx, r, ix.bmin[0], ix.inv_cell, ix.dim[0], &lo[0], &hi[0]) ||
        !index_cell_range((double)qy, r, ix.bmin[1], ix.inv_cell, ix.dim[1], &lo[1], &hi[1]) ||
        !index_cell_range((double)qz, r, ix.bmin[2], ix.inv_cell, ix.dim[2], &lo[2], &hi[2]))
        return 0;
    auto before = [&](float da, int sa, float db, int sb) { return da < db || (da == db && ix.id[sa] < ix.id[sb]); };
    int total = 0, m = 0;
    for (int z = lo[2]; z <= hi[2]; ++z)
        for (int y = lo[1]; y <= hi[1]; ++y) {
            // the cells of one x run are contiguous in the sorted records
            const long long row = ((long long)z * ix.dim[1] + y) * ix.dim[0];
            const int s0 = ix.cell_start[row + lo[0]], s1 = ix.cell_start[row + hi[0] + 1];
            for (int s = s0; s < s1; ++s) {
                const IndexRec v = ix.rec[s];
                const float dx = qx - v.x, dy = qy - v.y, dz = qz - v.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (!(d2 < r2)) continue;
                if (filter && d2 > ix.range2[s]) continue;
                if (!(d2 > lastD2 || (d2 == lastD2 && ix.id[s] > lastId))) continue;
                ++total;
                if (m == kConnectBuf && !before(d2, s, buf.d2(m - 1), buf.slot(m - 1))) continue;
                int j = m < kConnectBuf ? m++ : kConnectBuf - 1;
                for (; j > 0 && before(d2, s, buf.d2(j - 1), buf.slot(j - 1)); --j) {
                    buf.d2(j) = buf.d2(j - 1);
                    buf.slot(j) = buf.slot(j - 1);
                }
                buf.d2(j) = d2;
                buf.slot(j) = s;
            }
        }
    *kept = m;
    return total;
}

// ConnectToGraph for a point in graph space: the weighted light average, the number of
// vertices averaged and the stage (0, 1, 2) that found them.
template <typename Buf>
AVR_HD float index_connect(const IndexView &ix, float qx, float qy, float qz, Buf &buf, int *count, int *stage) {
    float r2 = ix.r2;
    bool filter = false;
    int m = 0, st = 0;
    int total = index_collect(ix, qx, qy, qz, r2, filter, -1.f, -1, buf, &m);
    if (total == 0 && ix.range2) {
        st = 1;
        r2 = ix.perc99;
        filter = true;
        total = index_collect(ix, qx, qy, qz, r2, filter, -1.f, -1, buf, &m);
        if (total == 0) {
            st = 2;
            r2 = ix.max_r2;
            total = index_collect(ix, qx, qy, qz, r2, filter, -1.f, -1, buf, &m);
        }
    }
    *count = total;
    *stage = st;
    float average = 0.f, totalWeight = 0.f;
    for (int left = total; left > 0;) {
        for (int i = 0; i < m; ++i) {
            const float weight = 1.f / buf.d2(i);
            average += ix.rec[buf.slot(i)].light * weight;
            totalWeight += weight;
        }
        left -= m;
        if (left <= 0 || m == 0) break;
        const float lastD2 = buf.d2(m - 1);
        const int lastId = ix.id[buf.slot(m - 1)];
        (void)index_collect(ix, qx, qy, qz, r2, filter, lastD2, lastId, buf, &m);
    }
    if (total == 0 || totalWeight == 0) return 0.f;
    return average / totalWeight;
}

// IntegrationAnalyzer's Analyze (integration_analyzer.cpp:56-83) for a point in graph space:
// *node = 1 when a vertex lies within the vertex radius; returns the number of vertices within
// the largest search range that are not beyond their own, and in *range_sum the float sum of
// their distances sqrtf(d2) in ascending key (d2, id). Without search ranges: 0 and 0.
template <typename Buf>
AVR_HD int index_coverage(const IndexView &ix, float qx, float qy, float qz, Buf &buf, int *node, float *range_sum) {
    int m = 0;
    *node = index_collect(ix, qx, qy, qz, ix.r2, false, -1.f, -1, buf, &m) > 0 ? 1 : 0;
    *range_sum = 0.f;
    if (!ix.range2) return 0;
    const int total = index_collect(ix, qx, qy, qz, ix.max_r2, true, -1.f, -1, buf, &m);
    float sum = 0.f;
    for (int left = total; left > 0;) {
        for (int i = 0; i < m; ++i) sum += __builtin_sqrtf(buf.d2(i));
        left -= m;
        if (left <= 0 || m == 0) break;
        const float lastD2 = buf.d2(m - 1);
        const int lastId = ix.id[buf.slot(m - 1)];
        (void)index_collect(ix, qx, qy, qz, ix.max_r2, true, lastD2, lastId, buf, &m);
    }
    *range_sum = sum;
    return total;
}

// FreeGraphBuilder::GetNClosest (free_graph_builder.cpp:473-496) for the vertex in sorted
// slot `slot`: its k <= kConnectBuf - 1 nearest other vertices in ascending key (d2, id), ids
// to ids_out[0..k) and squared distances to d2_out[0..k) (either may be null). The reference
// queries k + 1, sorts and drops item 0, the vertex itself; here the vertex is left out by
// id, which is the same unless another vertex coincides with it. The radius starts at the
// cell edge and doubles until k + 1 vertices (the vertex included) have d2 < r2: every vertex
// outside that radius is then farther than all of them, ties included. The loop ends when r2
// overflows to +inf, where every finite d2 qualifies: an isolated vertex costs one scan per
// doubling, and a radius beyond the grid's box scans the whole grid. Returns the neighbours
// found: k, or fewer when squared distances overflow float (the rest: id -1, d2 +inf).
template <typename Buf>
AVR_HD int index_knn(const IndexView &ix, int slot, int k, Buf &buf, int *ids_out, float *d2_out) {
    const IndexRec q = ix.rec[slot];
    const int self = ix.id[slot];
    const float edge = (float)(1.0 / ix.inv_cell);
    float r2 = edge * edge;
    if (!(r2 >= 1.17549435e-38f)) r2 = 1.17549435e-38f;   // a square that underflowed must still double
    int m = 0;
    while (true) {
        (void)index_collect(ix, q.x, q.y, q.z, r2, false, -1.f, -1, buf, &m);
        if (m >= k + 1 || !(r2 < INFINITY)) break;
        r2 *= 4.f;
    }
    int found = 0;
    for (int i = 0; i < m && found < k; ++i) {
        const int id = ix.id[buf.slot(i)];
        if (id == self) continue;
        if (ids_out) ids_out[found] = id;
        if (d2_out) d2_out[found] = buf.d2(i);
        ++found;
    }
    for (int i = found; i < k; ++i) {
        if (ids_out) ids_out[i] = -1;
        if (d2_out) d2_out[i] = INFINITY;
    }
    return found;
}

// ComputeSearchRanges' first Averager level (free_graph_builder.cpp:521-529, graph/util.h:
// 551-568): the float sum from 0 of sqrt(d2[i]), i ascending, over (float)k
AVR_HD float index_knn_average(const float *d2, int k) {
    float sum = 0.f;
    for (int i = 0; i < k; ++i) sum += __builtin_sqrtf(d2[i]);
    return sum / (float)k;
}

// ... and its second (:533-544): avg[v], then avg of v's neighbours in result order, over
// (float)(k + 1). A neighbour that was not found (id -1) counts as +inf.
AVR_HD float index_range_average(const float *avg, int v, const int *nb, int k) {
    float sum = 0.f;
    sum += avg[v];
    for (int i = 0; i < k; ++i) sum += nb[i] >= 0 ? avg[nb[i]] : INFINITY;
    return sum / (float)(k + 1);
}

// The sorted-key buffer in ordinary memory (the host's; the device keeps it in LDS)
struct ConnectBufLocal {
    float d[kConnectBuf];
    int s[kConnectBuf];
    AVR_HD float &d2(int i) { return d[i]; }
    AVR_HD int &slot(int i) { return s[i]; }
};

// The host index (avr_graph_index_*). Build() returns a message on a bad argument, else null.
class Index {
  public:
    const char *Build(long long n, const float *xyz, const float *light, const float *range, float radius) {
        if (n < 1 || n > 0x7fffffff || !xyz || !light) return "graph index: at least one vertex required";
        if (!(radius > 0) || !std::isfinite(radius)) return "graph index: vertex radius must be positive and finite";
        double bmin[3], bmax[3];
        for (int a = 0; a < 3; ++a) bmin[a] = bmax[a] = xyz[a];
        for (long long v = 0; v < n; ++v) {
            for (int a = 0; a < 3; ++a) {
                const float x = xyz[3 * v + a];
                if (!std::isfinite(x)) return "graph index: non-finite vertex coordinate";
                bmin[a] = std::min(bmin[a], (double)x);
                bmax[a] = std::max(bmax[a], (double)x);
            }
            if (range && (!(range[v] >= 0) || !std::isfinite(range[v])))
                return "graph index: search range must be non-negative and finite";
        }
        double cell = (double)radius;
        long long dim[3];
        while (true) {
            bool fits = true;
            long long cells = 1;
            inv_ = 1.0 / cell;
            for (int a = 0; a < 3 && fits; ++a) {
                const double d = index_cell_coord(bmax[a], bmin[a], inv_) + 1.0;   // the last vertex's cell + 1
                fits = d <= (double)kIndexCellBudget;
                dim[a] = fits ? (long long)d : 0;
                cells *= dim[a];
                fits = fits && cells <= kIndexCellBudget;
            }
            if (fits) break;
            cell *= 2.0;
        }
        for (int a = 0; a < 3; ++a) {
            bmin_[a] = bmin[a];
            dim_[a] = (int)dim[a];
        }
        const size_t cells = (size_t)dim_[0] * dim_[1] * dim_[2];
        std::vector<int> cellOf((size_t)n);
        start_.assign(cells + 1, 0);
        for (long long v = 0; v < n; ++v) {
            int c[3];
            for (int a = 0; a < 3; ++a) {
                const double k = index_cell_coord((double)xyz[3 * v + a], bmin_[a], inv_);
                c[a] = k < 0.0 ? 0 : (k > (double)(dim_[a] - 1) ? dim_[a] - 1 : (int)k);
            }
            cellOf[(size_t)v] = (c[2] * dim_[1] + c[1]) * dim_[0] + c[0];
            ++start_[(size_t)cellOf[(size_t)v] + 1];
        }
        for (size_t c = 0; c < cells; ++c) start_[c + 1] += start_[c];
        std::vector<int> fill(start_.begin(), start_.end() - 1);
        rec_.resize((size_t)n);
        id_.resize((size_t)n);
        range2_.clear();
        if (range) range2_.resize((size_t)n);
        for (long long v = 0; v < n; ++v) {
            const int s = fill[(size_t)cellOf[(size_t)v]]++;
            rec_[(size_t)s] = {xyz[3 * v], xyz[3 * v + 1], xyz[3 * v + 2], light[v]};
            id_[(size_t)s] = (int)v;
            if (range) range2_[(size_t)s] = range[v] * range[v];   // Sqr(renderSearchRange)
        }
        r2_ = radius * radius;   // Sqr(GetVertexRadius())
        perc99_ = max_r2_ = 0.f;
        if (range) {
            std::vector<float> sorted(range2_);
            std::sort(sorted.begin(), sorted.end());
            max_r2_ = sorted.back();
            perc99_ = sorted[sorted.size() * 99 / 100];
        }
        return nullptr;
    }

    IndexView View() const {
        IndexView v{};
        v.rec = rec_.data();
        v.id = id_.data();
        v.range2 = range2_.empty() ? nullptr : range2_.data();
        v.cell_start = start_.data();
        for (int a = 0; a < 3; ++a) {
            v.bmin[a] = bmin_[a];
            v.dim[a] = dim_[a];
        }
        v.inv_cell = inv_;
        v.r2 = r2_;
        v.perc99 = perc99_;
        v.max_r2 = max_r2_;
        return v;
    }

    void Connect(long long n, const float *points, float *light, int *count) const {
        const IndexView v = View();
        for (long long i = 0; i < n; ++i) {
            ConnectBufLocal buf;
            int cnt = 0, stage = 0;
            const float l = index_connect(v, points[3 * i], points[3 * i + 1], points[3 * i + 2], buf, &cnt, &stage);
            if (light) light[i] = l;
            if (count) count[i] = cnt;
        }
    }

    void Coverage(long long n, const float *points, int *node, int *in_range, float *range_sum) const {
        const IndexView v = View();
        for (long long i = 0; i < n; ++i) {
            ConnectBufLocal buf;
            int nd = 0;
            float sum = 0.f;
            const int cnt = index_coverage(v, points[3 * i], points[3 * i + 1], points[3 * i + 2], buf, &nd, &sum);
            if (node) node[i] = nd;
            if (in_range) in_range[i] = cnt;
            if (range_sum) range_sum[i] = sum;
        }
    }

    // GetNClosest for every vertex: row v of ids / d2 (k each) holds vertex v's neighbours
    void Knn(int k, int *ids, float *d2) const {
        const IndexView v = View();
        const int n = (int)rec_.size();
        for (int s = 0; s < n; ++s) {
            ConnectBufLocal buf;
            const size_t row = (size_t)id_[(size_t)s] * (size_t)k;
            (void)index_knn(v, s, k, buf, ids ? ids + row : nullptr, d2 ? d2 + row : nullptr);
        }
    }

    // ComputeSearchRanges (free_graph_builder.cpp:498-548): renderSearchRange per vertex id
    void SearchRanges(int k, float *ranges) const {
        const size_t n = rec_.size();
        std::vector<int> nb(n * (size_t)k);
        std::vector<float> d2(n * (size_t)k), avg(n);
        Knn(k, nb.data(), d2.data());
        for (size_t v = 0; v < n; ++v) avg[v] = index_knn_average(&d2[v * (size_t)k], k);
        for (size_t v = 0; v < n; ++v) ranges[v] = index_range_average(avg.data(), (int)v, &nb[v * (size_t)k], k);
    }

    size_t NumVertices() const { return rec_.size(); }
    size_t NumCells() const { return start_.size() - 1; }

  private:
    std::vector<IndexRec> rec_;
    std::vector<int> id_, start_;
    std::vector<float> range2_;
    double bmin_[3] = {0, 0, 0}, inv_ = 1;
    int dim_[3] = {1, 1, 1};
    float r2_ = 0, perc99_ = 0, max_r2_ = 0;
};

}  // namespace graph
}  // namespace avr
